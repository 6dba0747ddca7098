// LayerNorm forward and backward for the AVSR hot path (declarations and reference call sites
// in include/avsr_hip.h). HBM-bound: 16-byte vector loads/stores, fp32 statistics, one pass per
// tensor.
#include <algorithm>

#include "common.h"

namespace {

struct LnArgs {
  int rows, N; float eps;
  const void* x; int64_t ldx; void* y; int64_t ldy;
  const float* gamma; const float* beta; float* mean; float* rstd;
  const void* dy; int64_t lddy; void* dx; int64_t lddx; const void* dres; int64_t lddres;
  float* dgamma; float* dbeta; float* ws;
  void* g; int64_t ldg; float drop_p; uint64_t seed; bool db;   // fused ew_bwd (see avsr_layernorm_params)
};

// one wave per row; lane owns vectors lane, lane+64, ... (VPL of them)
template <typename T, int VPL>
__global__ __launch_bounds__(256) void ln_fwd_kernel(LnArgs a) {
  constexpr int VE = VecW<T>::VE;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (row >= a.rows) return;
  const T* x = (const T*)a.x + (int64_t)row * a.ldx;
  float v[VPL][VE];
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < VPL; ++i) {
    const int c = (lane + i * 64) * VE;
    if (c < a.N) ldv(x + c, v[i]);
    else
#pragma unroll
      for (int j = 0; j < VE; ++j) v[i][j] = 0.f;
#pragma unroll
    for (int j = 0; j < VE; ++j) s += v[i][j];
  }
  const float mean = wave_sum(s) / a.N;
  float q = 0.f;
#pragma unroll
  for (int i = 0; i < VPL; ++i) {
    const int c = (lane + i * 64) * VE;
    if (c < a.N)
#pragma unroll
      for (int j = 0; j < VE; ++j) { const float d = v[i][j] - mean; q += d * d; }
  }
  const float rstd = rsqrtf(wave_sum(q) / a.N + a.eps);
  T* y = (T*)a.y + (int64_t)row * a.ldy;
#pragma unroll
  for (int i = 0; i < VPL; ++i) {
    const int c = (lane + i * 64) * VE;
    if (c < a.N) {
      float o[VE];
#pragma unroll
      for (int j = 0; j < VE; ++j) o[j] = (v[i][j] - mean) * rstd * a.gamma[c + j] + a.beta[c + j];
      stv(y + c, o);
    }
  }
  if (lane == 0) { a.mean[row] = mean; a.rstd[row] = rstd; }
}

// grid-stride over rows, W waves per block, each wave R rows at a time with all their loads
// (x, dy, dres) issued together; dgamma/dbeta accumulated per lane in registers, summed over
// the block's waves in LDS (dynamic, W*N floats) and written as one partial row per block
// (colsum_finalize adds the blocks)
template <typename T, int VPL, int W, int R>
__global__ __launch_bounds__(64 * W) void ln_bwd_kernel(LnArgs a) {
  constexpr int VE = VecW<T>::VE;
  const int lane = threadIdx.x & 63;
  const int nw = gridDim.x * W;
  float dg[VPL][VE], db[VPL][VE], gm[VPL][VE], gb[VPL][VE];
#pragma unroll
  for (int i = 0; i < VPL; ++i) {
    const int c = (lane + i * 64) * VE;
#pragma unroll
    for (int j = 0; j < VE; ++j) {
      dg[i][j] = 0.f; db[i][j] = 0.f; gb[i][j] = 0.f; gm[i][j] = c < a.N ? a.gamma[c + j] : 0.f;
    }
  }
  for (int row0 = blockIdx.x * W + (threadIdx.x >> 6); row0 < a.rows; row0 += R * nw) {
    float xv[R][VPL][VE], dv[R][VPL][VE], rv[R][VPL][VE];
    float mean[R], rstd[R];
    bool live[R];
#pragma unroll
    for (int u = 0; u < R; ++u) {
      const int row = min(row0 + u * nw, a.rows - 1);
      live[u] = row0 + u * nw < a.rows;
      const T* x = (const T*)a.x + (int64_t)row * a.ldx;
      const T* dy = (const T*)a.dy + (int64_t)row * a.lddy;
      const T* dr = a.dres ? (const T*)a.dres + (int64_t)row * a.lddres : nullptr;
      mean[u] = a.mean[row]; rstd[u] = a.rstd[row];
#pragma unroll
      for (int i = 0; i < VPL; ++i) {
        const int c = min((lane + i * 64) * VE, a.N - VE);
        ldv(x + c, xv[u][i]);
        ldv(dy + c, dv[u][i]);
        if (dr) ldv(dr + c, rv[u][i]);
        else
#pragma unroll
          for (int j = 0; j < VE; ++j) rv[u][i][j] = 0.f;
      }
    }
#pragma unroll
    for (int u = 0; u < R; ++u) {
      float s1 = 0.f, s2 = 0.f;
#pragma unroll
      for (int i = 0; i < VPL; ++i) {
        const bool cok = (lane + i * 64) * VE < a.N && live[u];
#pragma unroll
        for (int j = 0; j < VE; ++j) {
          const float xh = (xv[u][i][j] - mean[u]) * rstd[u];
          const float g = cok ? dv[u][i][j] * gm[i][j] : 0.f;
          s1 += g;
          s2 += g * xh;
          dg[i][j] += cok ? dv[u][i][j] * xh : 0.f;
          db[i][j] += cok ? dv[u][i][j] : 0.f;
          xv[u][i][j] = xh;             // keep xhat and g for the output pass
          dv[u][i][j] = g;
        }
      }
      s1 = wave_sum(s1) / a.N;
      s2 = wave_sum(s2) / a.N;
      if (live[u]) {
        T* dx = (T*)a.dx + (int64_t)(row0 + u * nw) * a.lddx;
#pragma unroll
        for (int i = 0; i < VPL; ++i) {
          const int c = (lane + i * 64) * VE;
          if (c < a.N) {
            float o[VE];
#pragma unroll
            for (int j = 0; j < VE; ++j) o[j] = rv[u][i][j] + rstd[u] * (dv[u][i][j] - s1 - xv[u][i][j] * s2);
            stv(dx + c, o);
            if (a.g) {
              // the fused ew_bwd: dropout backward of dx AS STORED (rounded to T), same mask
              // stream and column sums as ew_bwd_kernel
              float d[VE];
#pragma unroll
              for (int j = 0; j < VE; ++j) d[j] = to_f(from_f<T>(o[j]));
              if (a.drop_p > 0.f) {
                const uint64_t i0 = (uint64_t)(row0 + u * nw) * a.N + c;
                if constexpr (VE == 8) drop8(a.drop_p, a.seed, i0, d);
                else {
#pragma unroll
                  for (int j = 0; j < VE; ++j) d[j] *= drop_scale(a.drop_p, a.seed, i0 + j);
                }
              }
#pragma unroll
              for (int j = 0; j < VE; ++j) gb[i][j] += d[j];
              stv((T*)a.g + (int64_t)(row0 + u * nw) * a.ldg + c, d);
            }
          }
        }
      }
    }
  }
  if (!a.dgamma) return;
  // per-block column partials (the block's waves summed in LDS) -> ws[block][2 or 3][N]
  extern __shared__ __attribute__((aligned(16))) float red[];   // [W][N]
  const int w = threadIdx.x >> 6;
  const int nq = a.db ? 3 : 2;
  for (int q = 0; q < nq; ++q) {
    __syncthreads();
#pragma unroll
    for (int i = 0; i < VPL; ++i) {
      const int c = (lane + i * 64) * VE;
      if (c < a.N) {
        // 16-byte stores of the lane's VE consecutive columns (scalar stores at a VE-float lane
        // stride were 4-8-way bank conflicts: 78 % of the kernel's LDS cycles, profiles/r05_sq_counters.txt)
        float* dst = red + w * a.N + c;
#pragma unroll
        for (int j = 0; j < VE; j += 4)
          *(f32x4*)(dst + j) = q == 0 ? f32x4{dg[i][j], dg[i][j + 1], dg[i][j + 2], dg[i][j + 3]}
                             : q == 1 ? f32x4{db[i][j], db[i][j + 1], db[i][j + 2], db[i][j + 3]}
                                      : f32x4{gb[i][j], gb[i][j + 1], gb[i][j + 2], gb[i][j + 3]};
      }
    }
    __syncthreads();
    for (int c = threadIdx.x; c < a.N; c += 64 * W) {
      float t = 0.f;
#pragma unroll
      for (int v = 0; v < W; ++v) t += red[v * a.N + c];
      a.ws[((int64_t)blockIdx.x * nq + q) * a.N + c] = t;
    }
  }
}

// LayerNorm backward launch shape, the only one instantiated: 4 waves per block, one row in
// flight per wave. In isolation 6000 x 1024 takes 18.3-20.1 us with 4-8 waves (2 waves: 26 us;
// 16 waves: 38 us), 8-16 waves lose 2x at N = 2048, and in the step 4,1 beats 2,x and 8,x by
// 0.5-1 % (profiles/r02_ln_bwd_shape_ab.txt). The kernel keeps W and R as template parameters:
// written out for this one shape it compiles to other code.
constexpr int LN_BWD_WAVES = 4, LN_BWD_ROWS = 1;

template <typename T, int VPL>
void ln_launch_vpl(bool bwd, int blocks, hipStream_t st, const LnArgs& a) {
  if (bwd)
    hipLaunchKernelGGL((ln_bwd_kernel<T, VPL, LN_BWD_WAVES, LN_BWD_ROWS>), dim3(blocks), dim3(64 * LN_BWD_WAVES),
                       (size_t)LN_BWD_WAVES * a.N * sizeof(float), st, a);
  else
    hipLaunchKernelGGL((ln_fwd_kernel<T, VPL>), dim3(blocks), dim3(256), 0, st, a);
}

template <typename T>
int ln_launch(const avsr_layernorm_params* p, bool bwd, hipStream_t st) {
  constexpr int VE = VecW<T>::VE;
  LnArgs a;
  a.rows = p->rows; a.N = p->N; a.eps = p->eps;
  a.x = p->x; a.ldx = p->ldx; a.y = p->y; a.ldy = p->ldy; a.gamma = p->gamma; a.beta = p->beta;
  a.mean = p->mean; a.rstd = p->rstd; a.dy = p->dy; a.lddy = p->lddy; a.dx = p->dx; a.lddx = p->lddx;
  a.dres = p->dres; a.lddres = p->lddres; a.dgamma = p->dgamma; a.dbeta = p->dbeta; a.ws = p->ws;
  a.g = bwd ? p->g : nullptr; a.ldg = p->ldg; a.drop_p = p->drop_p; a.seed = p->seed; a.db = bwd && p->db != nullptr;
  if (a.db && (!a.g || !p->dgamma)) return AVSR_E_ARG;     // the bias partials ride on the dgamma workspace
  if (bwd && p->dgamma && (!p->ws || p->N > 2048)) return AVSR_E_ARG;
  const int vpl = (p->N / VE + 63) / 64;
  const int blocks = bwd ? std::min((p->rows + LN_BWD_WAVES - 1) / LN_BWD_WAVES, AVSR_LN_BLOCKS) : (p->rows + 3) / 4;
  if (vpl <= 1) ln_launch_vpl<T, 1>(bwd, blocks, st, a);
  else if (vpl <= 2) ln_launch_vpl<T, 2>(bwd, blocks, st, a);
  else if (vpl <= 4) ln_launch_vpl<T, 4>(bwd, blocks, st, a);
  else if (vpl <= 8) ln_launch_vpl<T, 8>(bwd, blocks, st, a);
  else return AVSR_E_SHAPE;
  AVSR_CHECK_LAUNCH();
  if (!bwd || !p->dgamma) return 0;
  const int nq = a.db ? 3 : 2;
  const int rc = colsum_launch((const float*)p->ws, blocks, (int64_t)nq * p->N, 2 * p->N, p->dgamma, p->N, p->dbeta, st);
  if (rc || !a.db) return rc;
  return colsum_launch((const float*)p->ws + 2 * p->N, blocks, (int64_t)3 * p->N, p->N, p->db, 0, nullptr, st);
}

template <typename T>
int ln_check(const avsr_layernorm_params* p) {
  constexpr int VE = VecW<T>::VE;
  if (p->N % VE || p->ldx % VE || p->ldy % VE) return AVSR_E_ALIGN;
  return 0;
}

int ln_entry(const avsr_layernorm_params* p, bool bwd, void* stream) {
  if (!p) return AVSR_E_ARG;
  return avsr_by_dtype(p->dtype, [&](auto t) -> int {
    using T = decltype(t);
    const int rc = ln_check<T>(p);
    if (rc) return rc;
    if (p->rows == 0) return 0;
    return ln_launch<T>(p, bwd, (hipStream_t)stream);
  });
}

}  // namespace

extern "C" int avsr_layernorm_fwd(const avsr_layernorm_params* p, void* stream) { return ln_entry(p, false, stream); }
extern "C" int avsr_layernorm_bwd(const avsr_layernorm_params* p, void* stream) { return ln_entry(p, true, stream); }
