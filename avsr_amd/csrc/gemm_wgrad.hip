// The weight-gradient kernel of avsr_gemm (two wave groups per block, gemm.hip chooses it) and
// its grouped form (C-ABI avsr_gemm_wgrad_group). Mainloop: gemm_glds.h.
#include "gemm_dense.h"

using namespace gemmd;

namespace {

// Weight-gradient GEMM (both operands r-contiguous, fp32 out, plain epilogue) with an in-block
// K split: 8 waves = two groups of 4, each group a 128x128 Cfg tile over its own half of the
// block's K range with its own LDS ring (2 x 2 x 32 KiB), both groups in lockstep. Group 0 stages
// its accumulators in LDS, group 1 adds its own (fp32 addition commutes: fixed result), then all
// 8 waves write the tile: C = alpha*sum + beta*C, or the raw partial into split `sp`'s slab when
// the block grid also splits K (out-proj: 64 tiles x 4 splits). Two groups per block replace the
// two-blocks-per-CU split-K of the plain core without a slab round trip through HBM.
// With arrival counters (a.cnt) the grid split reduces in the kernel: a tile's splits are adjacent
// block ids (one XCD, one L2), each writes its partial slab write-through (sc1: relaxed agent-scope
// atomic stores), drains its stores (s_waitcnt vmcnt(0)) before the barrier that precedes its
// counter add, and the last of the tile's splits to arrive sums the slabs in split order (its own
// from LDS, the others with sc1 loads), writes C = alpha*sum + beta*C — the arithmetic of
// slab_reduce_kernel, which this replaces — and resets the counter (cdna_hip_programming.md
// Guideline 16, counter form).
template <class CF, bool FR>     // FR: the in-kernel slab reduction (its own register budget)
__device__ __forceinline__ void wgrad_dual_body(const DenseArgs& a, int tiles_m, int tiles_n, int id, char* smem) {
  static_assert(CF::BM * (CF::BN + 4) * 4 <= 2 * CF::S * CF::STAGE, "reduction tile exceeds the two rings");
  if (a.stamp != nullptr && threadIdx.x == 0) atomicMin(a.stamp, (unsigned long long)__builtin_amdgcn_s_memrealtime());
  int tm, tn, sp;
  if (a.cnt) {                                      // splits innermost: a tile's splits share an XCD
    int z;
    gemmg::tile_of(id / a.splits, tiles_m, tiles_n, tm, tn, z);
    sp = id % a.splits;
  } else {
    gemmg::tile_of(id, tiles_m, tiles_n, tm, tn, sp);
  }
  const int m0 = tm * CF::BM, n0 = tn * CF::BN;
  const int kbeg = sp * a.kchunk, kend = min(a.K, kbeg + a.kchunk);
  const int lane = threadIdx.x & 63;
  const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int grp = wv >> 2, wave = wv & 3;
  const int ntile = (kend - kbeg + gemmg::GBK - 1) / gemmg::GBK;
  const int nk = (ntile + 1) >> 1;                  // per group; group 1's last tile may be empty (zeros)
  const int gbeg = kbeg + grp * nk * gemmg::GBK, gend = min(kend, gbeg + nk * gemmg::GBK);
  f32x4 acc[CF::TM][CF::TN];
  char* ring = smem + grp * (CF::S * CF::STAGE);
  if (a.a_bytes) {
    gemmg::BDenseR<CF::BM, CF::NW> la; la.init((const bf16*)a.A, a.a_bytes, a.lda, m0, a.M, gend, wave, lane);
    gemmg::BDenseR<CF::BN, CF::NW> lb; lb.init((const bf16*)a.B, a.b_bytes, a.ldb, n0, a.N, gend, wave, lane);
    gemmg::mainloop_glds<CF>(la, lb, gbeg, nk, acc, ring, wave);
  } else {
    gemmg::GDenseR<CF::BM, CF::NW> la; la.init((const bf16*)a.A, a.lda, m0, a.M, gend, wave, lane);
    gemmg::GDenseR<CF::BN, CF::NW> lb; lb.init((const bf16*)a.B, a.ldb, n0, a.N, gend, wave, lane);
    gemmg::mainloop_glds<CF>(la, lb, gbeg, nk, acc, ring, wave);
  }
  // (mainloop_glds ends with a barrier: both rings are free)
  constexpr int LDR = CF::BN + 4;
  float* st = (float*)smem;
  const int wm = wave / CF::WN, wn = wave % CF::WN;
#pragma unroll
  for (int i = 0; i < CF::TM; ++i)
#pragma unroll
    for (int j = 0; j < CF::TN; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = wm * 32 * CF::FM + 16 * i + 4 * (lane >> 4) + r, col = wn * 32 * CF::FN + 16 * j + (lane & 15);
        if (grp == 0) st[row * LDR + col] = acc[i][j][r];
      }
  __syncthreads();
#pragma unroll
  for (int i = 0; i < CF::TM; ++i)
#pragma unroll
    for (int j = 0; j < CF::TN; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = wm * 32 * CF::FM + 16 * i + 4 * (lane >> 4) + r, col = wn * 32 * CF::FN + 16 * j + (lane & 15);
        if (grp == 1) st[row * LDR + col] += acc[i][j][r];
      }
  __syncthreads();
  const bool slab = a.sSplit != 0;
  constexpr int Q = CF::BN / 4;                      // float4 per tile row
  if constexpr (FR) {
    // 16-byte write-through (sc1) buffer stores / loads: the vector form of the agent-scope
    // relaxed atomic store / load (global_store_dword ... sc1), one instruction per 4 columns
    float* W = (float*)a.e.C;                        // slab 0; split q's at W + q * sSplit
    const int64_t ldw = a.e.ldc;
    const __amdgpu_buffer_rsrc_t rs = gemmg::make_rsrc(W, (uint32_t)((int64_t)a.splits * a.sSplit * 4));
    for (int c = threadIdx.x; c < CF::BM * Q; c += 2 * CF::NTH) {
      const int lr = c / Q, lc = (c % Q) * 4, row = m0 + lr, col = n0 + lc;
      if (row >= a.M || col >= a.N) continue;        // N % 4 == 0 in slab mode (host-checked)
      const f32x4 v = *(const f32x4*)(st + lr * LDR + lc);
      const uint32_t off = (uint32_t)((sp * a.sSplit + (int64_t)row * ldw + col) * 4);
      __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(v4i32, v), rs, off, 0, 16 /* sc1 */);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // every storing wave: its partial is out
    __shared__ int last;
    __syncthreads();
    const int tile = tm * tiles_n + tn;
    if (threadIdx.x == 0)
      last = __hip_atomic_fetch_add(&a.cnt[tile], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == (unsigned)a.splits - 1;
    __syncthreads();
    if (last) {
      // every load of the tail in flight at once (the tile's NI vectors per thread x the other
      // splits, and C for beta), then the sums in split order
      constexpr int NI = CF::BM * Q / (2 * CF::NTH), SMAX = 4;
      static_assert(NI * 2 * CF::NTH == CF::BM * Q, "tile vectors per thread");
      if (a.splits <= SMAX) {
        f32x4 pv[NI][SMAX], cv[NI];
#pragma unroll
        for (int i = 0; i < NI; ++i) {
          const int c = threadIdx.x + i * 2 * CF::NTH;
          const int lr = c / Q, lc = (c % Q) * 4, row = m0 + lr, col = n0 + lc;
          const bool ok = row < a.M && col < a.N;
          const int64_t w = (int64_t)row * ldw + col;
#pragma unroll
          for (int q = 0; q < SMAX; ++q)
            if (ok && q < a.splits && q != sp)
              pv[i][q] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(
                             rs, (uint32_t)((q * a.sSplit + w) * 4), 0, 16 /* sc1 */));
          if (ok && a.fbeta != 0.f) cv[i] = *(const f32x4*)(a.fC + (int64_t)row * a.fldc + col);
        }
#pragma unroll
        for (int i = 0; i < NI; ++i) {
          const int c = threadIdx.x + i * 2 * CF::NTH;
          const int lr = c / Q, lc = (c % Q) * 4, row = m0 + lr, col = n0 + lc;
          if (row >= a.M || col >= a.N) continue;
          const f32x4 own = *(const f32x4*)(st + lr * LDR + lc);
          f32x4 sum = sp == 0 ? own : pv[i][0];
#pragma unroll
          for (int q = 1; q < SMAX; ++q)
            if (q < a.splits) sum += (q == sp ? own : pv[i][q]);
          f32x4 y = sum * a.falpha;
          if (a.fbeta != 0.f) y += cv[i] * a.fbeta;
          *(f32x4*)(a.fC + (int64_t)row * a.fldc + col) = y;
        }
      } else {
        for (int c = threadIdx.x; c < CF::BM * Q; c += 2 * CF::NTH) {
          const int lr = c / Q, lc = (c % Q) * 4, row = m0 + lr, col = n0 + lc;
          if (row >= a.M || col >= a.N) continue;
          const int64_t w = (int64_t)row * ldw + col;
          const f32x4 own = *(const f32x4*)(st + lr * LDR + lc);
          f32x4 sum;
          for (int q = 0; q < a.splits; ++q) {
            f32x4 v;
            if (q == sp) v = own;
            else v = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(
                         rs, (uint32_t)((q * a.sSplit + w) * 4), 0, 16 /* sc1 */));
            if (q == 0) sum = v; else sum += v;
          }
          float* o = a.fC + (int64_t)row * a.fldc + col;
          f32x4 y = sum * a.falpha;
          if (a.fbeta != 0.f) y += *(const f32x4*)o * a.fbeta;
          *(f32x4*)o = y;
        }
      }
      if (threadIdx.x == 0) __hip_atomic_store(&a.cnt[tile], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    if (a.stamp != nullptr) {
      __syncthreads();
      if (threadIdx.x == 0) atomicMax(a.stamp + 1, (unsigned long long)__builtin_amdgcn_s_memrealtime());
    }
    return;
  }
  float* C = slab ? (float*)a.e.C + sp * a.sSplit : (float*)a.e.C;
  const int64_t ldc = a.e.ldc;
  const float alpha = slab ? 1.f : a.e.alpha, beta = slab ? 0.f : a.e.beta;
  for (int c = threadIdx.x; c < CF::BM * Q; c += 2 * CF::NTH) {
    const int lr = c / Q, lc = (c % Q) * 4, row = m0 + lr, col = n0 + lc;
    if (row >= a.M || col >= a.N) continue;
    const f32x4 v = *(const f32x4*)(st + lr * LDR + lc);
    float* o = C + (int64_t)row * ldc + col;
    if (col + 4 <= a.N) {
      f32x4 y = v * alpha;
      if (beta != 0.f) y += *(const f32x4*)o * beta;
      *(f32x4*)o = y;
    } else {
      for (int q = 0; q < a.N - col; ++q) o[q] = beta != 0.f ? alpha * v[q] + beta * o[q] : alpha * v[q];
    }
  }
  if (a.stamp != nullptr) {
    __syncthreads();
    if (threadIdx.x == 0) atomicMax(a.stamp + 1, (unsigned long long)__builtin_amdgcn_s_memrealtime());
  }
}

template <class CF, bool FR = false>
__global__ __launch_bounds__(2 * CF::NTH, 1) void wgrad_dual_kernel(DenseArgs a, int tiles_m, int tiles_n) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  wgrad_dual_body<CF, FR>(a, tiles_m, tiles_n, gemmg::xcd_remap(blockIdx.x, gridDim.x), smem);
}

// several weight-gradients in one grid (avsr_gemm_wgrad_group): block ids [start[q], start[q+1])
// are problem q's output tiles, each block the whole K range (no split). Two problems that leave
// part of the chip idle alone fill it together (encoder out-proj 64 + QKV 192 tiles = 256 = one
// block per CU).
constexpr int WG_MAX = 4;
struct WgGroup {
  DenseArgs a[WG_MAX];
  int tm[WG_MAX], tn[WG_MAX], start[WG_MAX + 1];
};
template <class CF>
__global__ __launch_bounds__(2 * CF::NTH, 1) void wgrad_group_kernel(WgGroup g) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int id = gemmg::xcd_remap(blockIdx.x, gridDim.x);
  int q = 0;
#pragma unroll
  for (int i = 1; i < WG_MAX; ++i) q += id >= g.start[i];
  q = __builtin_amdgcn_readfirstlane(q);
  wgrad_dual_body<CF, false>(g.a[q], g.tm[q], g.tn[q], id - g.start[q], smem);
}

using CfgDual = gemmg::GCfg<2, 2, 2, 2, 2>;       // per wave group of wgrad_dual_kernel (8 waves, 128 KiB)

template <class CF>
int launch_wgrad_dual(const DenseArgs& a, hipStream_t st) {
  const int tm = (a.M + CF::BM - 1) / CF::BM, tn = (a.N + CF::BN - 1) / CF::BN;
  const long nwg = (long)tm * tn * a.splits;
  if (nwg > 0x7fffffffL) return AVSR_E_SHAPE;
  const auto kernel = a.cnt ? wgrad_dual_kernel<CF, true> : wgrad_dual_kernel<CF, false>;
  hipLaunchKernelGGL(kernel, dim3((unsigned)nwg), dim3(2 * CF::NTH), 2 * CF::S * CF::STAGE, st, a, tm, tn);
  AVSR_CHECK_LAUNCH();
  return 0;
}

}  // namespace

// weight-gradient shape (dy^T x: both operands r-contiguous, fp32 C, plain epilogue, one batch):
// the in-block split-K kernel (AVSR_OPT_WGRAD_DUAL = 0 keeps the 4-wave core: A/B runs)
bool gemmd::wgrad_dual_ok(const avsr_gemm_params* p, int splits, bool slab) {
  const bool off = avsr_opt(AVSR_OPT_WGRAD_DUAL) == 0;
  return !off && !p->a_kmajor && !p->b_kmajor && p->c_f32 && p->batch == 1 && (splits == 1 || slab) && !p->bias &&
         !p->act && !p->preact && !p->res && !p->gate && p->drop_p == 0.f && !p->epi_bwd && !p->db &&
         (p->ldc % 4) == 0 && avsr_aligned16(p->C);
}

int gemmd::wgrad_dual_launch(const avsr_gemm_params* p, const DenseArgs& a, hipStream_t st, bool* reduced) {
  const int tiles = ((p->M + CfgDual::BM - 1) / CfgDual::BM) * ((p->N + CfgDual::BN - 1) / CfgDual::BN);
  *reduced = a.sSplit != 0 && p->slab_cnt && tiles <= AVSR_SLAB_CNT && (int64_t)a.splits * a.sSplit * 4 < (1ll << 31);
  if (!*reduced) return launch_wgrad_dual<CfgDual>(a, st);
  DenseArgs r = a;   // in-kernel slab reduction (no slab_reduce pass)
  r.cnt = p->slab_cnt; r.fC = (float*)p->C; r.fldc = p->ldc; r.falpha = p->alpha; r.fbeta = p->beta;
  return launch_wgrad_dual<CfgDual>(r, st);
}

// grouped weight-gradients: each problem must be the plain wgrad_dual shape (bf16 operands, both
// r-contiguous, fp32 C, no epilogue, no split); otherwise the problems run one by one
extern "C" int avsr_gemm_wgrad_group(const avsr_gemm_params* ps, int n, void* stream) {
  if (!ps || n < 1 || n > WG_MAX) return AVSR_E_ARG;
  bool grouped = true;
  for (int i = 0; i < n; ++i) {
    const avsr_gemm_params* p = ps + i;
    if (p->M <= 0 || p->N <= 0 || p->K <= 0 || p->batch != 1) return AVSR_E_SHAPE;
    grouped = grouped && glds_ok(p) && p->splitk <= 1 && !p->ws && !p->stamp && wgrad_dual_ok(p, 1, false) &&
              avsr_aligned16(p->A) && avsr_aligned16(p->B) && (p->lda % 8) == 0 && (p->ldb % 8) == 0;
  }
  if (!grouped) {
    for (int i = 0; i < n; ++i) {
      const int rc = avsr_gemm(ps + i, stream);
      if (rc) return rc;
    }
    return 0;
  }
  using CF = CfgDual;
  WgGroup g{};
  int total = 0;
  for (int i = 0; i < n; ++i) {
    const avsr_gemm_params* p = ps + i;
    g.a[i] = dense_args(p, 1, false);
    g.tm[i] = (p->M + CF::BM - 1) / CF::BM;
    g.tn[i] = (p->N + CF::BN - 1) / CF::BN;
    g.start[i] = total;
    total += g.tm[i] * g.tn[i];
  }
  for (int i = n; i <= WG_MAX; ++i) g.start[i] = total;
  hipLaunchKernelGGL(wgrad_group_kernel<CF>, dim3((unsigned)total), dim3(2 * CF::NTH), 2 * CF::S * CF::STAGE,
                     (hipStream_t)stream, g);
  AVSR_CHECK_LAUNCH();
  return 0;
}
