// BatchNorm (+PReLU, +residual) forward and backward for the ResNet frontends (declarations
// and reference call sites in include/avsr_hip.h). HBM-bound: 16-byte vector loads/stores, fp32
// statistics, one pass per tensor where the math allows.
#include "norm.h"

namespace {

// one block of BNF_THREADS per channel: Chan-merge of the conv epilogue's (count, mean, M2)
// tile partials (the stem has ~45 k tiles per channel: 1024 threads keep that under ~40 us)
constexpr int BNF_THREADS = 1024;
__global__ __launch_bounds__(BNF_THREADS) void bn_finalize_kernel(avsr_bn_finalize_params a) {
  const int c = blockIdx.x;
  __shared__ double sn[BNF_THREADS], sm[BNF_THREADS], sq[BNF_THREADS];
  double n = 0, mean = 0, m2 = 0;
  if (a.training) {
    const float* pp = a.partials + (int64_t)c * a.tiles * 3;
    for (int t = threadIdx.x; t < a.tiles; t += blockDim.x) {
      const double nb = pp[t * 3 + 0], mb = pp[t * 3 + 1], qb = pp[t * 3 + 2];
      if (nb > 0) {
        const double nn = n + nb, d = mb - mean;
        mean += d * nb / nn;
        m2 += qb + d * d * n * nb / nn;
        n = nn;
      }
    }
    sn[threadIdx.x] = n; sm[threadIdx.x] = mean; sq[threadIdx.x] = m2;
    __syncthreads();
    for (int o = blockDim.x / 2; o > 0; o >>= 1) {     // blockDim.x: 256 or 1024
      if (threadIdx.x < o) {
        const double na = sn[threadIdx.x], nb = sn[threadIdx.x + o];
        if (nb > 0) {
          const double nn = na + nb, d = sm[threadIdx.x + o] - sm[threadIdx.x];
          sm[threadIdx.x] += d * nb / nn;
          sq[threadIdx.x] += sq[threadIdx.x + o] + d * d * na * nb / nn;
          sn[threadIdx.x] = nn;
        }
      }
      __syncthreads();
    }
  }
  if (threadIdx.x == 0) {
    double mu, var;
    if (a.training) {
      n = sn[0]; mu = sm[0]; var = n > 0 ? sq[0] / n : 0.0;
      if (a.running_mean) {
        const double unb = n > 1 ? sq[0] / (n - 1) : var;
        a.running_mean[c] = (float)((1.0 - a.momentum) * a.running_mean[c] + a.momentum * mu);
        a.running_var[c] = (float)((1.0 - a.momentum) * a.running_var[c] + a.momentum * unb);
      }
    } else {
      mu = a.running_mean[c]; var = a.running_var[c];
    }
    const float inv = (float)(1.0 / sqrt(var + (double)a.eps));
    const float g = a.gamma ? a.gamma[c] : 1.f, b = a.beta ? a.beta[c] : 0.f;
    a.mean[c] = (float)mu; a.invstd[c] = inv;
    a.scale[c] = g * inv; a.shift[c] = b - (float)mu * g * inv;
  }
}

struct BnArgs {
  int M, C;
  const void* h; const float* scale; const float* shift;
  const void* res; const float* scale2; const float* shift2;
  const float* prelu; void* y;
  const void* dy; void* dz;
  const float* mean; const float* invstd; const float* mean2; const float* invstd2;
  float* sums; float* dprelu; float* dgamma; float* dbeta; float* dgamma2; float* dbeta2;
  void* dh; void* dh2; float beta_acc; float* ws;
};

// y = PReLU(h*scale + shift [+ res*scale2 + shift2 | + res]); two vectors per iteration so
// each wave keeps two independent 16-byte loads (x2 with the residual) in flight.
template <typename T>
__global__ __launch_bounds__(256) void bn_act_fwd_kernel(BnArgs a) {
  constexpr int VE = VecW<T>::VE;
  const int cpv = a.C / VE;
  const int64_t nv = (int64_t)a.M * cpv, stride = (int64_t)gridDim.x * 256;
  const int64_t t0 = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int c0 = (int)(t0 % cpv) * VE;
  float sc[VE], sh[VE], pw[VE], sc2[VE], sh2[VE];
  chan_load(a.scale, c0, sc); chan_load(a.shift, c0, sh); chan_load(a.prelu, c0, pw);
  chan_load(a.scale2, c0, sc2); chan_load(a.shift2, c0, sh2);
  const bool res = a.res != nullptr, res_bn = a.scale2 != nullptr;
  for (int64_t v = t0; v < nv; v += 2 * stride) {
    const bool two = v + stride < nv;
    float h[2][VE], r[2][VE];
    ldv((const T*)a.h + v * VE, h[0]);
    if (two) ldv((const T*)a.h + (v + stride) * VE, h[1]);
    if (res) {
      ldv((const T*)a.res + v * VE, r[0]);
      if (two) ldv((const T*)a.res + (v + stride) * VE, r[1]);
    }
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      if (u == 1 && !two) break;
      float o[VE];
#pragma unroll
      for (int j = 0; j < VE; ++j) {
        float z = h[u][j] * sc[j] + sh[j];
        if (res) z += res_bn ? r[u][j] * sc2[j] + sh2[j] : r[u][j];
        o[j] = z > 0.f ? z : z * pw[j];
      }
      stv((T*)a.y + (v + u * stride) * VE, o);
    }
  }
}

// block-level reduction of per-thread channel partials (a thread's channel group is fixed:
// the grid stride is a multiple of C/VE) -> ws[block][q][C] (plain stores)
template <int VE>
__device__ void block_chan_partial(const float (&q)[VE], float* lds, int cpv, float* ws_row) {
#pragma unroll
  for (int j = 0; j < VE; ++j) lds[threadIdx.x * VE + j] = q[j];
  __syncthreads();
  if ((int)threadIdx.x < cpv) {
    float acc[VE];
#pragma unroll
    for (int j = 0; j < VE; ++j) acc[j] = 0.f;
    for (int t = threadIdx.x; t < 256; t += cpv)
#pragma unroll
      for (int j = 0; j < VE; ++j) acc[j] += lds[t * VE + j];
#pragma unroll
    for (int j = 0; j < VE; ++j) ws_row[threadIdx.x * VE + j] = acc[j];
  }
  __syncthreads();
}

// per channel: S_q = sum over blocks; sums[c][0..2] = S0..S2 (set); grads accumulate
__global__ __launch_bounds__(256) void bn_grad_finalize_kernel(const float* ws, int nb, int C, float* sums,
                                                               float* dbeta, float* dgamma, float* dbeta2,
                                                               float* dgamma2, float* dprelu) {
  const int c = blockIdx.x;
  __shared__ float sh[4][4];
  float s[4] = {0.f, 0.f, 0.f, 0.f};
  for (int b = threadIdx.x; b < nb; b += 256)
#pragma unroll
    for (int q = 0; q < 4; ++q) s[q] += ws[((int64_t)b * 4 + q) * C + c];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const float v = wave_sum(s[q]);
    if ((threadIdx.x & 63) == 0) sh[q][threadIdx.x >> 6] = v;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    float t[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) t[q] = sh[q][0] + sh[q][1] + sh[q][2] + sh[q][3];
    if (sums) { sums[c * 3 + 0] = t[0]; sums[c * 3 + 1] = t[1]; sums[c * 3 + 2] = t[2]; }
    if (dbeta) dbeta[c] += t[0];
    if (dgamma) dgamma[c] += t[1];
    if (dbeta2) dbeta2[c] += t[0];
    if (dgamma2) dgamma2[c] += t[2];
    if (dprelu) dprelu[c] += t[3];
  }
}

// dz = prelu'(z)*dy with z recomputed; per-block channel partials of sum dz, sum dz*xhat,
// sum dz*xhat2 and the PReLU-weight sum dy*z*[z<=0] -> ws[block][4][C]. Two vectors per
// iteration (independent 16-byte loads in flight).
template <typename T>
__global__ __launch_bounds__(256) void bn_bwd_reduce_kernel(BnArgs a) {
  constexpr int VE = VecW<T>::VE;
  __shared__ float lds[256 * VE];
  const int cpv = a.C / VE;
  const int64_t nv = (int64_t)a.M * cpv, stride = (int64_t)gridDim.x * 256;
  float s0[VE], s1[VE], s2[VE], s3[VE];
#pragma unroll
  for (int j = 0; j < VE; ++j) { s0[j] = s1[j] = s2[j] = s3[j] = 0.f; }
  const int64_t t0 = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int c0 = (int)(t0 % cpv) * VE;
  float sc[VE], sh[VE], pw[VE], mu[VE], is[VE], sc2[VE], sh2[VE], mu2[VE], is2[VE];
  chan_load(a.scale, c0, sc); chan_load(a.shift, c0, sh); chan_load(a.prelu, c0, pw);
  chan_load(a.mean, c0, mu); chan_load(a.invstd, c0, is);
  chan_load(a.scale2, c0, sc2); chan_load(a.shift2, c0, sh2); chan_load(a.mean2, c0, mu2); chan_load(a.invstd2, c0, is2);
  const bool res = a.res != nullptr, res_bn = a.scale2 != nullptr;
  for (int64_t v = t0; v < nv; v += 2 * stride) {
    const bool two = v + stride < nv;
    float h[2][VE], r[2][VE], d[2][VE];
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      if (u == 1 && !two) break;
      const int64_t w = v + u * stride;
      ldv((const T*)a.h + w * VE, h[u]);
      ldv((const T*)a.dy + w * VE, d[u]);
      if (res) ldv((const T*)a.res + w * VE, r[u]);
    }
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      if (u == 1 && !two) break;
      float dzo[VE];
#pragma unroll
      for (int j = 0; j < VE; ++j) {
        float z = h[u][j] * sc[j] + sh[j];
        if (res) z += res_bn ? r[u][j] * sc2[j] + sh2[j] : r[u][j];
        const bool pos = z > 0.f;
        const float dz = pos ? d[u][j] : d[u][j] * pw[j];
        s3[j] += pos ? 0.f : d[u][j] * z;
        dzo[j] = dz;
        s0[j] += dz;
        s1[j] += dz * (h[u][j] - mu[j]) * is[j];
        if (res_bn) s2[j] += dz * (r[u][j] - mu2[j]) * is2[j];
      }
      stv((T*)a.dz + (v + u * stride) * VE, dzo);
    }
  }
  // channel partials of this block -> ws[block][q][C]; bn_grad_finalize sums the blocks
  float* wsb = a.ws + (int64_t)blockIdx.x * 4 * a.C;
  block_chan_partial<VE>(s0, lds, cpv, wsb + 0 * a.C);
  block_chan_partial<VE>(s1, lds, cpv, wsb + 1 * a.C);
  block_chan_partial<VE>(s2, lds, cpv, wsb + 2 * a.C);
  block_chan_partial<VE>(s3, lds, cpv, wsb + 3 * a.C);
}

// ws[nb][4][C] -> ws2[slices][4][C]: one wave per (channel group of 64, slice of BN_FOLD_PER
// block rows), four rows per iteration (16 independent 256-byte coalesced loads in flight per
// lane), no LDS. Single-wave blocks: the fold runs on the main stream while the side stream's
// persistent weight-gradient blocks (conv_wgrad_patch, one 4-wave block per CU with up to 152 KB
// of LDS) hold every CU, and the former 8-wave / 8 KB-LDS blocks found no room beside them
// (6 us alone, 180 us in the step: they waited for the weight-gradient tail).
constexpr int BN_FOLD_PER = 16;
__global__ __launch_bounds__(64) void bn_ws_fold_kernel(const float* ws, int nb, int C, float* ws2) {
  const int c = blockIdx.x * 64 + threadIdx.x, sl = blockIdx.y;
  const int b0 = sl * BN_FOLD_PER, b1 = min(nb, b0 + BN_FOLD_PER);
  if (c >= C) return;
  float s[4][4] = {};
  int b = b0;
  for (; b + 3 < b1; b += 4)
#pragma unroll
    for (int u = 0; u < 4; ++u)
#pragma unroll
      for (int q = 0; q < 4; ++q) s[u][q] += ws[((int64_t)(b + u) * 4 + q) * C + c];
  for (; b < b1; ++b)
#pragma unroll
    for (int q = 0; q < 4; ++q) s[0][q] += ws[((int64_t)b * 4 + q) * C + c];
#pragma unroll
  for (int q = 0; q < 4; ++q) ws2[((int64_t)sl * 4 + q) * C + c] = (s[0][q] + s[1][q]) + (s[2][q] + s[3][q]);
}

template <typename T>
__global__ __launch_bounds__(256) void bn_bwd_apply_kernel(BnArgs a) {
  constexpr int VE = VecW<T>::VE;
  const int cpv = a.C / VE;
  const int64_t nv = (int64_t)a.M * cpv, stride = (int64_t)gridDim.x * 256;
  const int64_t t0 = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int c0 = (int)(t0 % cpv) * VE;
  const float invM = 1.f / (float)a.M;
  // dh = scale*(dz - S0/M - xh*S1/M) with xh = (h-mean)*invstd  ==  A*dz + B*(h-mean) + Cc
  float ka[VE], kb[VE], kc[VE], km[VE], ka2[VE], kb2[VE], kc2[VE], km2[VE];
#pragma unroll
  for (int j = 0; j < VE; ++j) {
    const int c = c0 + j;
    const float s0 = a.sums[c * 3 + 0] * invM, s1 = a.sums[c * 3 + 1] * invM;
    ka[j] = a.scale[c];
    kb[j] = -a.scale[c] * s1 * a.invstd[c];
    kc[j] = -a.scale[c] * s0;
    km[j] = a.mean[c];
    if (a.dh2) {
      const float s2 = a.sums[c * 3 + 2] * invM;
      ka2[j] = a.scale2[c];
      kb2[j] = -a.scale2[c] * s2 * a.invstd2[c];
      kc2[j] = -a.scale2[c] * s0;
      km2[j] = a.mean2[c];
    }
  }
  const bool acc = a.beta_acc != 0.f;
  // U grid-stride vectors per iteration with every load issued first (memory-level
  // parallelism: one vector in flight per thread left this pass at ~65 % of HBM bandwidth)
  constexpr int U = 4;
  for (int64_t v0 = t0; v0 < nv; v0 += U * stride) {
    float dz[U][VE], h[U][VE], o[U][VE], r[U][VE];
    bool ok[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int64_t v = v0 + u * stride;
      ok[u] = v < nv;
      const int64_t vv = ok[u] ? v : v0;
      ldv((const T*)a.dz + vv * VE, dz[u]);
      ldv((const T*)a.h + vv * VE, h[u]);
      if (acc) ldv((const T*)a.dh + vv * VE, o[u]);
      if (a.dh2) ldv((const T*)a.res + vv * VE, r[u]);
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      if (!ok[u]) break;
      const int64_t v = v0 + u * stride;
      float g[VE];
#pragma unroll
      for (int j = 0; j < VE; ++j) {
        const float gg = ka[j] * dz[u][j] + kb[j] * (h[u][j] - km[j]) + kc[j];
        g[j] = acc ? a.beta_acc * o[u][j] + gg : gg;
      }
      stv((T*)a.dh + v * VE, g);
      if (a.dh2) {
        float o2[VE];
#pragma unroll
        for (int j = 0; j < VE; ++j) o2[j] = ka2[j] * dz[u][j] + kb2[j] * (r[u][j] - km2[j]) + kc2[j];
        stv((T*)a.dh2 + v * VE, o2);
      }
    }
  }
}

BnArgs bn_args(const avsr_bn_act_params* p) {
  BnArgs a;
  a.M = p->M; a.C = p->C; a.h = p->h; a.scale = p->scale; a.shift = p->shift; a.res = p->res;
  a.scale2 = p->scale2; a.shift2 = p->shift2; a.prelu = p->prelu; a.y = p->y; a.dy = p->dy; a.dz = p->dz;
  a.mean = p->mean; a.invstd = p->invstd; a.mean2 = p->mean2; a.invstd2 = p->invstd2; a.sums = p->sums;
  a.dprelu = p->dprelu; a.dgamma = p->dgamma; a.dbeta = p->dbeta; a.dgamma2 = p->dgamma2; a.dbeta2 = p->dbeta2;
  a.dh = p->dh; a.dh2 = p->dh2; a.beta_acc = p->beta_acc; a.ws = p->ws;
  return a;
}

// C/VE channel vectors must be a power of two <= 256: the kernels' grid stride (blocks * 256)
// is then a multiple of it, which keeps every thread on one channel group
template <typename T>
int bn_check(const avsr_bn_act_params* p) {
  constexpr int VE = VecW<T>::VE;
  if (p->C % VE || (p->C / VE) > 256 || (256 % (p->C / VE))) return AVSR_E_SHAPE;
  return 0;
}

}  // namespace

extern "C" int avsr_bn_finalize(const avsr_bn_finalize_params* p, void* stream) {
  if (!p || p->C <= 0) return AVSR_E_ARG;
  if (p->training && !p->partials) return AVSR_E_ARG;
  if (!p->training && (!p->running_mean || !p->running_var)) return AVSR_E_ARG;
  hipLaunchKernelGGL(bn_finalize_kernel, dim3(p->C), dim3(p->training && p->tiles > 2048 ? BNF_THREADS : 256), 0,
                     (hipStream_t)stream, *p);
  AVSR_CHECK_LAUNCH();
  return 0;
}

extern "C" int avsr_bn_act_fwd(const avsr_bn_act_params* p, void* stream) {
  if (!p) return AVSR_E_ARG;
  return avsr_by_dtype(p->dtype, [&](auto t) -> int {
    using T = decltype(t);
    const int rc = bn_check<T>(p);
    if (rc) return rc;
    const int g = bn_grid((int64_t)p->M * p->C / VecW<T>::VE);
    hipLaunchKernelGGL(bn_act_fwd_kernel<T>, dim3(g), dim3(256), 0, (hipStream_t)stream, bn_args(p));
    AVSR_CHECK_LAUNCH();
    return 0;
  });
}

extern "C" int avsr_bn_act_bwd_reduce(const avsr_bn_act_params* p, void* stream) {
  if (!p) return AVSR_E_ARG;
  return avsr_by_dtype(p->dtype, [&](auto t) -> int {
    using T = decltype(t);
    const int rc = bn_check<T>(p);
    if (rc) return rc;
    if (!p->ws) return AVSR_E_ARG;
    const int g = bn_grid((int64_t)p->M * p->C / VecW<T>::VE);
    hipLaunchKernelGGL(bn_bwd_reduce_kernel<T>, dim3(g), dim3(256), 0, (hipStream_t)stream, bn_args(p));
    AVSR_CHECK_LAUNCH();
    return avsr_bn_bwd_finalize(p, g, stream);
  });
}

// ws[tiles][4][C] (from the reduce kernel or a data-grad BN epilogue) -> sums + parameter
// grads. More than 256 partial rows are first folded into ceil(tiles / 16) slices, stored after
// the partials (ws holds AVSR_BN_FIN_WS(tiles, C) floats).
extern "C" int avsr_bn_bwd_finalize(const avsr_bn_act_params* p, int tiles, void* stream) {
  if (!p || !p->ws || p->C <= 0 || tiles <= 0) return AVSR_E_ARG;
  const float* ws = p->ws;
  int nb = tiles;
  hipStream_t st = (hipStream_t)stream;
  if (tiles > 256) {
    const int SL = (tiles + BN_FOLD_PER - 1) / BN_FOLD_PER;
    if (SL > 65535) return AVSR_E_SHAPE;
    float* ws2 = p->ws + (int64_t)tiles * 4 * p->C;
    hipLaunchKernelGGL(bn_ws_fold_kernel, dim3((p->C + 63) / 64, SL), dim3(64), 0, st, (const float*)p->ws, tiles,
                       p->C, ws2);
    ws = ws2; nb = SL;
  }
  hipLaunchKernelGGL(bn_grad_finalize_kernel, dim3(p->C), dim3(256), 0, st, ws, nb, p->C, p->sums, p->dbeta,
                     p->dgamma, p->dbeta2, p->dgamma2, p->dprelu);
  AVSR_CHECK_LAUNCH();
  return 0;
}

extern "C" int avsr_bn_bwd_apply(const avsr_bn_act_params* p, void* stream) {
  if (!p) return AVSR_E_ARG;
  return avsr_by_dtype(p->dtype, [&](auto t) -> int {
    using T = decltype(t);
    const int rc = bn_check<T>(p);
    if (rc) return rc;
    if (!p->sums || !p->dz || !p->dh) return AVSR_E_ARG;
    const int g = bn_grid((int64_t)p->M * p->C / VecW<T>::VE);
    hipLaunchKernelGGL(bn_bwd_apply_kernel<T>, dim3(g), dim3(256), 0, (hipStream_t)stream, bn_args(p));
    AVSR_CHECK_LAUNCH();
    return 0;
  });
}
