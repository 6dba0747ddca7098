// avsr_ctc_neighbors (include/avsr_hip.h): the exact CTC log-likelihood of every one-edit
// neighbour of a label sequence -- y with slot l replaced by each vocabulary token, and y with
// slot l deleted -- from which avsr_amd/confidence.py forms token confidences. Three launches:
//   1. nb_alphabeta_kernel: alpha and beta of y, one workgroup per utterance, both recursions in
//      ONE loop of n steps (alpha walks forward while beta walks backward: they are independent,
//      so they share the step's barrier). States strided over the threads, the variables
//      ping-pong in LDS, emissions gathered into LDS a chunk of frames at a time, as loss.hip's
//      recursions. It also validates, and writes feasible, base and the deletion scores.
//   2. nb_sub_kernel: the substitution recurrences, the hot path: L * V recurrences of n steps.
//      Lanes over v, NB_SL slots per lane, sequential over t. Per step and slot everything but
//      e(t,v) and the lane's running a_t is the same for all v: the four alpha / beta
//      combinations a lane can need (with / without the skip transition on either side) are
//      computed once per (frame, slot) by the block into LDS, a chunk of frames at a time, and
//      read back as broadcasts; a lane picks by two flags fixed at its start (v == y_{l-1},
//      v == y_{l+1}). One coalesced load of e(t, v) serves the NB_SL slots, whose independent
//      chains also hide each other's exp / log latency. The sum over t runs as an online
//      (max, sum) pair: one exp per step, the log once at the end.
//   3. nb_norm_kernel (only when lz is asked for): lz = Z_l - base per slot, one workgroup per
//      row of sub, sums relative to the row maximum in a fixed tree.
// Unreachable is -inf (IEEE), never a large negative: an infeasible neighbour comes out -inf
// exactly. No atomics on floats anywhere; per (slot, v) the time order is fixed.
#include "common.h"

namespace {

constexpr float NINF = -__builtin_inff();
constexpr int NB_CHUNK = 4096;    // floats per LDS emission chunk (one for alpha, one for beta)
constexpr int NB_SL = 4;          // slots per lane in nb_sub_kernel
constexpr int NB_FR = 64;         // frames per chunk of uniform operands (NB_FR * NB_SL = 256 threads)
constexpr int NB_PF = 8;          // emission loads in flight per lane

// log(exp(a) + exp(b)); -inf only if both are. Hardware exp2 / log2 (v_exp_f32 / v_log_f32) as
// loss.hip's recursions: the larger term contributes exp(0) = 1 exactly.
AVSR_DEV float nb_lse2(float a, float b) {
  const float m = fmaxf(a, b), r = m + __logf(1.f + __expf(fminf(a, b) - m));
  return m == NINF ? NINF : r;
}
AVSR_DEV float nb_lse3(float a, float b, float c) {
  const float m = fmaxf(a, fmaxf(b, c));
  const float r = m + __logf(__expf(a - m) + __expf(b - m) + __expf(c - m));
  return m == NINF ? NINF : r;
}
// running log-sum-exp as (M, s) = (largest term so far, sum of exp(term - M)); M starts at a
// finite floor below every log-probability so that a -inf term adds exp(-inf) = 0
constexpr float NB_FLOOR = -1e30f;
AVSR_DEV void nb_acc(float& M, float& s, float x) {
  const float d = x - M, e = __expf(-fabsf(d));
  const bool gt = d > 0.f;
  s = gt ? fmaf(s, e, 1.f) : s + e;
  M = gt ? x : M;
}
AVSR_DEV float nb_fin(float M, float s) { return s > 0.f ? M + __logf(s) : NINF; }

template <typename T>
__global__ __launch_bounds__(256) void nb_alphabeta_kernel(avsr_ctc_neighbors_params p) {
  const int b = blockIdx.x, tid = threadIdx.x;
  const int L = p.label_len[b], n = min(p.in_len[b], p.T);
  const int SS = 2 * p.Lmax + 1;
  const int* lab = p.labels + (int64_t)b * p.Lmax;
  const T* X = (const T*)p.x + (int64_t)b * p.T * p.ldx;
  const float* LSE = p.lse + (int64_t)b * p.T;
  float* A = (float*)p.ws + (int64_t)b * p.T * SS;
  float* Bt = (float*)p.ws + (int64_t)p.B * p.T * SS + (int64_t)b * p.T * SS;
  float* DEL = p.del + (int64_t)b * p.Lmax;
  __shared__ float ab[2][2][1024];          // [alpha / beta][step parity][state]
  __shared__ float EA[NB_CHUNK], EB[NB_CHUNK];
  __shared__ int kl[1024];
  __shared__ unsigned char sk[1024];
  __shared__ int bad, rep;
  if (tid == 0) { bad = 0; rep = 0; }
  __syncthreads();
  const bool shape_ok = L >= 0 && L <= p.Lmax && n > 0;
  const int S = 2 * L + 1;
  if (shape_ok) {
    int r = 0;
    for (int s = tid; s < S; s += 256) {
      int k = p.blank;
      if (s & 1) {
        k = lab[s >> 1];
        if (k < 0 || k >= p.V || k == p.blank) { bad = 1; k = p.blank; }
        if (s >= 3 && k == lab[(s >> 1) - 1]) ++r;
      }
      kl[s] = k;
    }
    if (r) atomicAdd(&rep, r);              // an integer count: order does not matter
  }
  __syncthreads();
  if (!shape_ok || bad || n < L + rep) {
    for (int j = tid; j < p.Lmax; j += 256) DEL[j] = NINF;
    if (tid == 0) { p.base[b] = 0.f; p.feasible[b] = 0; }
    return;
  }
  for (int s = tid; s < S; s += 256) sk[s] = s >= 2 && (s & 1) && kl[s] != kl[s - 2];
  const int CH = max(1, min(64, NB_CHUNK / S));
  // EA[j * S + s] = e(i0 + j, s), EB[j * S + s] = e(n - 1 - i0 - j, s) for j < cn
  auto load = [&](int i0, int cn) {
    for (int i = tid; i < cn * S; i += 256) {
      const int j = i / S, s = i - j * S, ta = i0 + j, tb = n - 1 - i0 - j;
      const int k = kl[s];
      EA[i] = to_f(X[(int64_t)ta * p.ldx + k]) - LSE[ta];
      EB[i] = to_f(X[(int64_t)tb * p.ldx + k]) - LSE[tb];
    }
  };
  __syncthreads();
  int i0 = 0;
  load(0, min(CH, n));
  __syncthreads();
  for (int s = tid; s < S; s += 256) {
    const float a0 = s < 2 ? EA[s] : NINF, b0 = s >= S - 2 ? EB[s] : NINF;
    ab[0][0][s] = a0;
    ab[1][0][s] = b0;
    A[s] = a0;
    Bt[(int64_t)(n - 1) * SS + s] = b0;
  }
  __syncthreads();
  for (int i = 1; i < n; ++i) {
    if (i - i0 >= CH) {
      i0 = i;
      load(i0, min(CH, n - i0));
      __syncthreads();
    }
    const float* pa = ab[0][(i - 1) & 1];
    const float* pb = ab[1][(i - 1) & 1];
    float* ca = ab[0][i & 1];
    float* cb = ab[1][i & 1];
    const float* ea = EA + (i - i0) * S;
    const float* eb = EB + (i - i0) * S;
    float* ga = A + (int64_t)i * SS;
    float* gb = Bt + (int64_t)(n - 1 - i) * SS;
    for (int s = tid; s < S; s += 256) {
      const float a1 = s >= 1 ? pa[s - 1] : NINF;
      const float a2 = sk[s] ? pa[s - 2] : NINF;
      const float ra = nb_lse3(pa[s], a1, a2) + ea[s];
      const float b1 = s + 1 < S ? pb[s + 1] : NINF;
      const float b2 = (s + 2 < S && sk[s + 2]) ? pb[s + 2] : NINF;
      const float rb = nb_lse3(pb[s], b1, b2) + eb[s];
      ca[s] = ra; cb[s] = rb;
      ga[s] = ra; gb[s] = rb;
    }
    __syncthreads();
  }
  if (tid == 0) {
    const float* last = ab[0][(n - 1) & 1];
    p.base[b] = S > 1 ? nb_lse2(last[S - 1], last[S - 2]) : last[0];
    p.feasible[b] = 1;
  }
  // deletions: one slot per thread, a sum over the frames of alpha / beta as this block wrote
  // them (the loop's last barrier made them visible to the block)
  const float* AL = A + (int64_t)(n - 1) * SS;
  for (int j = tid; j < p.Lmax; j += 256) {
    const int l = j + 1;
    float r = NINF;
    if (j >= L) r = NINF;
    else if (L == 1) r = AL[0];
    else if (l == L) r = nb_lse2(AL[2 * L - 2], AL[2 * L - 3]);
    else {
      const bool skip = l > 1 && lab[j - 1] != lab[j + 1];
      float M = NB_FLOOR, s = 0.f;
      if (l == 1) nb_acc(M, s, Bt[3]);
      for (int t = 0; t + 1 < n; ++t) {
        const float* at = A + (int64_t)t * SS;
        float u = at[2 * l - 2];
        if (skip) u = nb_lse2(u, at[2 * l - 3]);
        nb_acc(M, s, u + Bt[(int64_t)(t + 1) * SS + 2 * l + 1]);
      }
      r = nb_fin(M, s);
    }
    DEL[j] = r;
  }
}

template <typename T>
__global__ __launch_bounds__(256) void nb_sub_kernel(avsr_ctc_neighbors_params p) {
  const int b = blockIdx.z, tid = threadIdx.x;
  const int j0 = blockIdx.y * NB_SL;                 // first slot of the block, 0-based
  const int v = blockIdx.x * 256 + tid;
  const int SS = 2 * p.Lmax + 1;
  const bool feas = p.feasible[b] != 0;
  const int L = feas ? p.label_len[b] : 0, n = min(p.in_len[b], p.T);
  float* SUB = p.sub + ((int64_t)b * p.Lmax + j0) * p.lds;
  if (j0 >= L) {                                     // nothing to compute: the fill rows
#pragma unroll
    for (int k = 0; k < NB_SL; ++k)
      if (j0 + k < p.Lmax && v < p.lds) SUB[(int64_t)k * p.lds + v] = NINF;
    return;
  }
  const int* lab = p.labels + (int64_t)b * p.Lmax;
  const T* X = (const T*)p.x + (int64_t)b * p.T * p.ldx + min(v, p.V - 1);
  const float* LSE = p.lse + (int64_t)b * p.T;
  const float* A = (const float*)p.ws + (int64_t)b * p.T * SS;
  const float* Bt = (const float*)p.ws + (int64_t)p.B * p.T * SS + (int64_t)b * p.T * SS;
  __shared__ f32x4 U[NB_FR][NB_SL];                  // (U0, U1, D0, D1) per (frame, slot)
  __shared__ float LS[NB_FR];
  bool skA[NB_SL], skB[NB_SL];
  float a[NB_SL], M[NB_SL], sm[NB_SL];
#pragma unroll
  for (int k = 0; k < NB_SL; ++k) {
    const int j = j0 + k;
    skA[k] = j >= 1 && j < L && v != lab[j - 1];
    skB[k] = j + 1 < L && v != lab[j + 1];
    a[k] = NINF; M[k] = NB_FLOOR; sm[k] = 0.f;
  }
  for (int t0 = 0; t0 < n; t0 += NB_FR) {
    const int cn = min(NB_FR, n - t0);
    __syncthreads();                                 // the chunk before is consumed
    {
      // thread (frame tt, slot k): with a' the lane's a_{t-1} and t = t0 + tt,
      //   a_t = e(t,v) + LSE(a', skA ? U1 : U0);  sub (+)= a_t + (skB ? D1 : D0)
      const int tt = tid / NB_SL, k = tid % NB_SL, j = j0 + k, t = t0 + tt;
      f32x4 u = {NINF, NINF, NINF, NINF};
      if (tt < cn && j < L) {
        if (t == 0) u[0] = u[1] = j == 0 ? 0.f : NINF;
        else {
          const float* at = A + (int64_t)(t - 1) * SS;
          u[0] = at[2 * j];
          u[1] = j >= 1 ? nb_lse2(u[0], at[2 * j - 1]) : u[0];
        }
        if (t == n - 1) u[2] = u[3] = j == L - 1 ? 0.f : NINF;
        else {
          const float* bt = Bt + (int64_t)(t + 1) * SS;
          u[2] = bt[2 * j + 2];
          u[3] = j + 1 < L ? nb_lse2(u[2], bt[2 * j + 3]) : u[2];
        }
      }
      U[tt][k] = u;
      if (tid < cn) LS[tid] = LSE[t0 + tid];
    }
    __syncthreads();
    for (int c0 = 0; c0 < cn; c0 += NB_PF) {
      float ev[NB_PF];
#pragma unroll
      for (int q = 0; q < NB_PF; ++q)                // clamped, not branched: NB_PF loads in flight
        ev[q] = to_f(X[(int64_t)(t0 + min(c0 + q, cn - 1)) * p.ldx]);
#pragma unroll
      for (int q = 0; q < NB_PF; ++q) {
        if (c0 + q < cn) {
          const float e = ev[q] - LS[c0 + q];
#pragma unroll
          for (int k = 0; k < NB_SL; ++k) {
            const f32x4 u = U[c0 + q][k];
            a[k] = e + nb_lse2(a[k], skA[k] ? u[1] : u[0]);
            nb_acc(M[k], sm[k], a[k] + (skB[k] ? u[3] : u[2]));
          }
        }
      }
    }
  }
  if (v < p.lds) {
    const bool off = v >= p.V || v == p.blank || v == p.eos;
#pragma unroll
    for (int k = 0; k < NB_SL; ++k)
      if (j0 + k < p.Lmax) SUB[(int64_t)k * p.lds + v] = (off || j0 + k >= L) ? NINF : nb_fin(M[k], sm[k]);
  }
}

// lz[b][l] = LSE(sub[b][l][allowed v], del[b][l]) - base[b], relative to the row's largest term
__global__ __launch_bounds__(256) void nb_norm_kernel(avsr_ctc_neighbors_params p) {
  const int j = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
  __shared__ float sh[4];
  float* out = p.lz + (int64_t)b * p.Lmax + j;
  const bool live = p.feasible[b] != 0 && j < p.label_len[b];
  if (!live) {
    if (tid == 0) *out = NINF;
    return;
  }
  const float* row = p.sub + ((int64_t)b * p.Lmax + j) * p.lds;
  const float d = p.del[(int64_t)b * p.Lmax + j];
  float m = NINF;
  for (int c = tid; c < p.V; c += 256) m = fmaxf(m, row[c]);
  m = wave_max(m);
  if ((tid & 63) == 0) sh[tid >> 6] = m;
  __syncthreads();
  m = fmaxf(fmaxf(fmaxf(sh[0], sh[1]), fmaxf(sh[2], sh[3])), d);   // finite: sub[l][y_l] is, unless
  __syncthreads();                                                 // y_l is the excluded eos
  if (m == NINF) {
    if (tid == 0) *out = NINF;
    return;
  }
  float s = 0.f;
  for (int c = tid; c < p.V; c += 256) s += expf(row[c] - m);
  s = wave_sum(s);
  if ((tid & 63) == 0) sh[tid >> 6] = s;
  __syncthreads();
  if (tid == 0) *out = (m - p.base[b]) + logf(((sh[0] + sh[1]) + (sh[2] + sh[3])) + expf(d - m));
}

}  // namespace

extern "C" int avsr_ctc_neighbors(const avsr_ctc_neighbors_params* p, void* stream) {
  if (!p || p->B < 0 || p->T < 0 || p->Lmax < 0 || p->V <= 0 || p->ldx < p->V || p->lds < p->V || p->blank < 0 ||
      p->blank >= p->V || p->eos < -1 || p->eos >= p->V)
    return AVSR_E_ARG;
  return avsr_by_dtype(p->dtype, [&](auto t) -> int {
    using T = decltype(t);
    if (2 * p->Lmax + 1 > 1024) return AVSR_E_SHAPE;
    if (p->B == 0) return 0;
    if (!p->label_len || !p->in_len || !p->base || !p->feasible || (p->Lmax > 0 && (!p->labels || !p->sub || !p->del)))
      return AVSR_E_ARG;
    if (p->T > 0 && (!p->x || !p->lse || !p->ws)) return AVSR_E_ARG;
    if ((uintptr_t)p->ws & 15) return AVSR_E_ALIGN;
    if (p->B > 65535 || (p->Lmax + NB_SL - 1) / NB_SL > 65535) return AVSR_E_SHAPE;
    const hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(nb_alphabeta_kernel<T>, dim3(p->B), dim3(256), 0, st, *p);
    AVSR_CHECK_LAUNCH();
    if (p->Lmax == 0) return 0;
    const dim3 grid((unsigned)((p->lds + 255) / 256), (p->Lmax + NB_SL - 1) / NB_SL, p->B);
    hipLaunchKernelGGL(nb_sub_kernel<T>, grid, dim3(256), 0, st, *p);
    AVSR_CHECK_LAUNCH();
    if (p->lz) {
      hipLaunchKernelGGL(nb_norm_kernel, dim3(p->Lmax, p->B), dim3(256), 0, st, *p);
      AVSR_CHECK_LAUNCH();
    }
    return 0;
  });
}
