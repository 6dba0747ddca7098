// Kernels over parameters and their gradients (declarations, reference call sites:
// include/avsr_hip.h): pos-conv weight norm forward and backward, the gradient sum of squares,
// and the fused clip-grad-norm + AdamW step. All HBM-bound, grid-stride loops.
#include "common.h"

namespace {

// norm[k] = ||v[:, k, :]||  (v stored [O][K][C]); one block per k
__global__ __launch_bounds__(256) void wn_norm_kernel(int O, int K, int C, const float* v, const float* dw,
                                                      float* out) {
  const int k = blockIdx.x;
  float s = 0.f;
  for (int i = threadIdx.x; i < O * C; i += 256) {
    const int o = i / C, c = i % C;
    const int64_t idx = ((int64_t)o * K + k) * C + c;
    s += dw ? dw[idx] * v[idx] : v[idx] * v[idx];
  }
  s = wave_sum(s);
  __shared__ float sh[4];
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    const float t = sh[0] + sh[1] + sh[2] + sh[3];
    out[k] = dw ? t : sqrtf(t);
  }
}

// same reduction with 16-byte loads and 16 waves per k (C % 4 == 0, v / dw 16-byte aligned):
// the 128 blocks of the pos-conv weight stream 256 KB each instead of one 4-byte load per thread
// and iteration behind a runtime division (125 -> ~15 us per call)
__global__ __launch_bounds__(1024) void wn_norm4_kernel(int O, int K, int C, const float* v, const float* dw,
                                                        float* out) {
  const int k = blockIdx.x, c4n = C >> 2, per = O * c4n;
  float s = 0.f;
#pragma unroll 4
  for (int i = threadIdx.x; i < per; i += 1024) {
    const int o = i / c4n, c4 = i - o * c4n;
    const int64_t idx = ((int64_t)o * K + k) * C + 4 * c4;
    const f32x4 a = *(const f32x4*)(v + idx);
    const f32x4 b = dw ? *(const f32x4*)(dw + idx) : a;
    s += a[0] * b[0] + a[1] * b[1] + a[2] * b[2] + a[3] * b[3];
  }
  s = wave_sum(s);
  __shared__ float sh[16];
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    float t = 0.f;
#pragma unroll
    for (int w = 0; w < 16; ++w) t += sh[w];
    out[k] = dw ? t : sqrtf(t);
  }
}

void wn_norm_launch(int O, int K, int C, const float* v, const float* dw, float* out, hipStream_t st) {
  if (C % 4 == 0 && avsr_aligned16(v) && (!dw || avsr_aligned16(dw)))
    hipLaunchKernelGGL(wn_norm4_kernel, dim3(K), dim3(1024), 0, st, O, K, C, v, dw, out);
  else
    hipLaunchKernelGGL(wn_norm_kernel, dim3(K), dim3(256), 0, st, O, K, C, v, dw, out);
}

template <typename T>
__global__ __launch_bounds__(256) void wn_apply_kernel(int O, int K, int C, const float* v, const float* g,
                                                       const float* norm, T* w) {
  const int64_t total = (int64_t)O * K * C;
  for (int64_t i = blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int k = (int)((i / C) % K);
    w[i] = from_f<T>(g[k] * v[i] / norm[k]);
  }
}

__global__ __launch_bounds__(256) void wn_bwd_kernel(int O, int K, int C, const float* v, const float* g,
                                                     const float* norm, const float* dw, const float* s,
                                                     float* dv) {
  const int64_t total = (int64_t)O * K * C;
  for (int64_t i = blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int k = (int)((i / C) % K);
    const float n = norm[k];
    dv[i] += g[k] / n * dw[i] - g[k] * s[k] / (n * n * n) * v[i];
  }
}

__global__ void wn_dg_kernel(int K, const float* s, const float* norm, float* dg) {
  const int k = blockIdx.x * 256 + threadIdx.x;
  if (k < K) dg[k] += s[k] / norm[k];
}

// sum of squares in two deterministic passes: per-block partials -> ws, then one block sums
// them in a fixed order and adds the total to *out
__global__ __launch_bounds__(256) void sumsq_kernel(const float* x, int64_t n, float* ws) {
  float s = 0.f;
  const int64_t n4 = n / 4;
  for (int64_t i = blockIdx.x * 256 + threadIdx.x; i < n4; i += (int64_t)gridDim.x * 256) {
    const f32x4 v = ((const f32x4*)x)[i];
    s += v[0] * v[0] + v[1] * v[1] + v[2] * v[2] + v[3] * v[3];
  }
  if (blockIdx.x == 0)
    for (int64_t i = n4 * 4 + threadIdx.x; i < n; i += 256) s += x[i] * x[i];
  s = wave_sum(s);
  __shared__ float sh[4];
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) ws[blockIdx.x] = (sh[0] + sh[1]) + (sh[2] + sh[3]);
}

__global__ __launch_bounds__(256) void sumsq_final_kernel(const float* ws, int nb, float* out) {
  float s = 0.f;
  for (int i = threadIdx.x; i < nb; i += 256) s += ws[i];
  s = wave_sum(s);
  __shared__ float sh[4];
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) *out += (sh[0] + sh[1]) + (sh[2] + sh[3]);
}

struct AdamCoef { float coef, step, rbc2, decay; };

AVSR_DEV AdamCoef adam_coef(const avsr_adamw_params& p) {
  AdamCoef c;
  c.coef = p.grad_scale;
  if (p.sumsq) {
    const float tn = sqrtf(*p.sumsq) * p.grad_scale;
    c.coef *= fminf(1.f, p.max_norm / (tn + 1e-6f));
  }
  c.step = p.lr / p.bias_corr1;
  c.rbc2 = 1.f / sqrtf(p.bias_corr2);
  c.decay = p.lr * p.weight_decay;
  return c;
}

// one element (torch.optim.AdamW arithmetic: decoupled decay, then the moment update)
AVSR_DEV float adam_elem(const avsr_adamw_params& p, const AdamCoef& c, float g, float w, float& m, float& v) {
  g *= c.coef;
  w -= c.decay * w;
  m = p.beta1 * m + (1.f - p.beta1) * g;
  v = p.beta2 * v + (1.f - p.beta2) * g * g;
  return w - c.step * m / (sqrtf(v) * c.rbc2 + p.eps);
}

// Four elements per thread and iteration with 16-byte loads / stores: elements [0, head) and
// [head + 4*nv, n) (fewer than 4 each, to reach / past the 16-byte boundary) by block 0.
template <typename S>
__global__ __launch_bounds__(256) void adamw_kernel(avsr_adamw_params p, int head, int64_t nv) {
  const AdamCoef c = adam_coef(p);
  if (blockIdx.x == 0 && threadIdx.x < 8) {
    const int t = threadIdx.x;
    const int64_t i = t < 4 ? t : head + 4 * nv + (t - 4);
    if ((t < 4 && t < head) || (t >= 4 && i < p.n)) {
      float m = p.exp_avg[i], v = p.exp_avg_sq[i];
      const float w = adam_elem(p, c, p.grad[i], p.param[i], m, v);
      p.exp_avg[i] = m; p.exp_avg_sq[i] = v; p.param[i] = w;
      if (p.shadow) ((S*)p.shadow)[i] = from_f<S>(w);
      if (p.grad_clear) p.grad_clear[i] = 0.f;
    }
  }
  float* P = p.param + head; const float* G = p.grad + head;
  float* M = p.exp_avg + head; float* V = p.exp_avg_sq + head;
  for (int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x; q < nv; q += (int64_t)gridDim.x * 256) {
    const f32x4 g = *(const f32x4*)(G + 4 * q);
    f32x4 w = *(const f32x4*)(P + 4 * q), m = *(const f32x4*)(M + 4 * q), v = *(const f32x4*)(V + 4 * q);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      float mj = m[j], vj = v[j];
      w[j] = adam_elem(p, c, g[j], w[j], mj, vj);
      m[j] = mj; v[j] = vj;
    }
    *(f32x4*)(P + 4 * q) = w; *(f32x4*)(M + 4 * q) = m; *(f32x4*)(V + 4 * q) = v;
    if (p.grad_clear) *(f32x4*)(p.grad_clear + head + 4 * q) = f32x4{0.f, 0.f, 0.f, 0.f};
    if (p.shadow) {
      S* sh = (S*)p.shadow + head + 4 * q;
      if constexpr (sizeof(S) == 2) {
        bf16x4 o;
#pragma unroll
        for (int j = 0; j < 4; ++j) o[j] = (bf16)w[j];
        *(bf16x4*)sh = o;
      } else {
        *(f32x4*)sh = w;
      }
    }
  }
}

}  // namespace

extern "C" int avsr_weightnorm_fwd(int dtype, int O, int K, int C, const float* v, const float* g, float* norm,
                                   void* w, void* stream) {
  return avsr_by_dtype(dtype, [&](auto t) -> int {
    using T = decltype(t);
    hipStream_t st = (hipStream_t)stream;
    wn_norm_launch(O, K, C, v, nullptr, norm, st);
    const int gr = avsr_grid((int64_t)O * K * C);
    hipLaunchKernelGGL(wn_apply_kernel<T>, dim3(gr), dim3(256), 0, st, O, K, C, v, g, norm, (T*)w);
    AVSR_CHECK_LAUNCH();
    return 0;
  });
}

extern "C" int avsr_weightnorm_bwd(int O, int K, int C, const float* v, const float* g, const float* norm,
                                   const float* dw, float* dv, float* dg, float* scratch, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  wn_norm_launch(O, K, C, v, dw, scratch, st);
  AVSR_CHECK_LAUNCH();
  hipLaunchKernelGGL(wn_dg_kernel, dim3((K + 255) / 256), dim3(256), 0, st, K, (const float*)scratch, norm, dg);
  AVSR_CHECK_LAUNCH();
  hipLaunchKernelGGL(wn_bwd_kernel, dim3(avsr_grid((int64_t)O * K * C)), dim3(256), 0, st, O, K, C, v, g, norm, dw,
                     (const float*)scratch, dv);
  AVSR_CHECK_LAUNCH();
  return 0;
}

extern "C" int avsr_sumsq(const float* x, int64_t n, float* out, float* ws, void* stream) {
  if (!avsr_aligned16(x)) return AVSR_E_ALIGN;
  if (!out || !ws) return AVSR_E_ARG;
  const int nb = avsr_grid(n / 4 + 1, 256, AVSR_SUMSQ_WS);
  hipLaunchKernelGGL(sumsq_kernel, dim3(nb), dim3(256), 0, (hipStream_t)stream, x, n, ws);
  AVSR_CHECK_LAUNCH();
  hipLaunchKernelGGL(sumsq_final_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, (const float*)ws, nb, out);
  AVSR_CHECK_LAUNCH();
  return 0;
}

extern "C" int avsr_adamw(const avsr_adamw_params* p, void* stream) {
  if (!p) return AVSR_E_ARG;
  return avsr_by_dtype(p->shadow_dtype, [&](auto t) -> int {
    using S = decltype(t);
    if (p->n == 0) return 0;
    // the four fp32 arrays share their offset modulo 16 bytes (one arena index); the shadow must
    // then be 8-byte (bf16) / 16-byte (fp32) aligned at the same element
    const uintptr_t a0 = (uintptr_t)p->param & 15;
    if ((((uintptr_t)p->grad & 15) != a0) || (((uintptr_t)p->exp_avg & 15) != a0) || (((uintptr_t)p->exp_avg_sq & 15) != a0) || (a0 & 3))
      return AVSR_E_ALIGN;
    int head = (int)(((16 - a0) & 15) / 4);
    if (head > p->n) head = (int)p->n;
    const int64_t nv = (p->n - head) / 4;
    if (p->shadow && (((uintptr_t)p->shadow + head * sizeof(S)) & (4 * sizeof(S) - 1))) return AVSR_E_ALIGN;
    if (p->max_blocks < 0) return AVSR_E_ARG;
    if (p->grad_clear && p->grad_clear != p->grad) return AVSR_E_ARG;
    const int g = avsr_grid(nv > 0 ? nv : 1, 256, p->max_blocks > 0 && p->max_blocks < 4096 ? p->max_blocks : 4096);
    hipLaunchKernelGGL(adamw_kernel<S>, dim3(g), dim3(256), 0, (hipStream_t)stream, *p, head, nv);
    AVSR_CHECK_LAUNCH();
    return 0;
  });
}
