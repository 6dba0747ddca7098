// CTC prefix scores of the beam search (declaration and avsr_ctc_prefix_params under "Joint CTC /
// attention beam search" in include/avsr_hip.h):
//   avsr_ctc_prefix        CTC prefix scores of the pre-beam tokens (T recursion)
// All fp32 math; one block per hypothesis, the T recursion sequential per scored token.
#include "decode.h"

namespace {

// torch.logsumexp of two finite values: m + log(exp(a-m) + exp(b-m)). One of the two terms is
// exp(0) = 1 exactly, so m + log(1 + exp(min - m)) is the same float computation with one
// transcendental less (bit-identical; the CTC prefix recursion's serial chain is two of these)
AVSR_DEV float lse2(float a, float b) {
  const float m = fmaxf(a, b);
  return m + logf(1.f + expf(fminf(a, b) - m));
}
// the same with the hardware exp2 / log2 (v_exp_f32 / v_log_f32, ~1 ulp): the CTC prefix
// recursion's dependent chain (two of these per frame, T frames in sequence), as in loss.hip's
// CTC recursion; the correction term is <= log 2, so the result differs from lse2 by a few ulp
// of that term
AVSR_DEV float lse2_fast(float a, float b) {
  const float m = fmaxf(a, b);
  return m + __logf(1.f + __expf(fminf(a, b) - m));
}

// CTCPrefixScoreTH.__call__ (ctc_prefix_score.py:65-187) for one utterance: block = one
// hypothesis, lane j = its j-th scored token; the T recursion is sequential per lane.
__global__ __launch_bounds__(64) void ctc_prefix_kernel(avsr_ctc_prefix_params p) {
  const int h = blockIdx.x, j = threadIdx.x;
  if (p.out_len_dev) p.out_len = p.out_len_dev[h * p.out_len_stride];
  const int V = p.V;
  const int u = p.uidx ? p.uidx[h] : 0;
  const int T = p.uidx ? p.tlen[u] : p.T;         // this utterance's frames
  const int TS = p.T;                              // row stride of r_prev / r_new
  if (p.uidx) p.logp += (int64_t)u * p.logp_ustride;
  const bool act = j < p.P;
  const int id = act ? p.ids[h * p.P + j] : 0;
  const bool same = act && id == p.last[h];
  // (per-row lengths: a row of length 0 is at its first step whatever the launch's r_prev holds)
  const bool first = !p.r_prev || (p.out_len_stride && p.out_len == 0);
  const float* rp = first ? nullptr : p.r_prev + (int64_t)h * TS * 2;
  float* rn = act ? p.r_new + ((int64_t)h * p.P + j) * TS * 2 : nullptr;
  // r_prev at the first step: (logzero, cumsum of blank log-probs)
  auto rprev = [&](int t, int q, float cum) -> float { return rp ? rp[t * 2 + q] : (q == 0 ? LOGZERO : cum); };
  const int start = min(max(p.out_len, 1), T);     // (a dead row past its frames stays inside them)
  // values of r for t < start
  float r0 = LOGZERO, r1 = LOGZERO;
  float cum = 0.f;          // running cumsum of logp[t][blank] (first step only)
  for (int t = 0; t < start; ++t) {
    const float xb = p.logp[(int64_t)t * V + p.blank];
    cum += xb;
    float a0 = LOGZERO;
    if (t == 0 && p.out_len == 0) a0 = act ? p.logp[id] : LOGZERO;
    if (act) { rn[t * 2 + 0] = a0; rn[t * 2 + 1] = LOGZERO; }
    if (t == start - 1) { r0 = a0; r1 = LOGZERO; }
  }
  // psi accumulates logsumexp over { phi(t-1) + x0(t) : t in [start, T) } U { r0(start-1) }
  float pm = r0;            // running max
  float ps = 1.f;           // sum of exp(. - pm)
  // phi(t-1) needs r_prev at t-1: carry the previous frame's values
  float prev_r0 = rprev(start - 1, 0, 0.f);
  float prev_r1 = rprev(start - 1, 1, cum);   // cum = cumsum of blank log-probs through start-1
  float cur_cum = cum;
  for (int t = start; t < T; ++t) {
    const float rsum_prev = lse2(prev_r0, prev_r1);
    const float phi = same ? prev_r1 : rsum_prev;
    const float x0 = act ? p.logp[(int64_t)t * V + id] : LOGZERO;
    const float xb = p.logp[(int64_t)t * V + p.blank];
    const float n0 = lse2_fast(r0, phi) + x0;
    const float n1 = lse2_fast(r0, r1) + xb;
    r0 = n0; r1 = n1;
    if (act) { rn[t * 2 + 0] = r0; rn[t * 2 + 1] = r1; }
    const float term = phi + x0;
    if (term > pm) { ps = ps * expf(pm - term) + 1.f; pm = term; }
    else ps += expf(term - pm);
    cur_cum += xb;
    prev_r0 = rprev(t, 0, 0.f);
    prev_r1 = rprev(t, 1, cur_cum);
  }
  // r_sum at the last frame (for eos): logsumexp of r_prev[T-1]
  const float rsum_last = lse2(prev_r0, prev_r1);
  float psi = pm + logf(ps);
  if (act) {
    if (id == p.blank) psi = LOGZERO;
    if (id == p.eos) psi = rsum_last;
    p.psi[h * (p.P + 1) + j] = psi;
  }
  if (j == 0) p.psi[h * (p.P + 1) + p.P] = rsum_last;
}

// The same recursion with its inputs staged in LDS first: the P scored tokens' and the blank's
// log-probs over all T frames ([T][P + 1], 4 independent gathers in flight per lane, the token
// ids read once) and phi(t) for both cases of a candidate ([T][2]: logsumexp(r_prev[t]) and
// r_prev[t][1] for a repeated label; at the first step the blank cumsum). Only the r recursion is
// sequential (wave 0, LDS reads issued ahead by the unrolled loop, hardware exp2 / log2 on the
// chain): psi = logsumexp({r0(start-1)} U {phi(t-1) + x0(t)}) does not depend on r, so waves 1-3
// reduce it meanwhile (a wave per candidate, lanes over t).
__global__ __launch_bounds__(256) void ctc_prefix_lds_kernel(avsr_ctc_prefix_params p) {
  extern __shared__ float sm[];
  __shared__ int sid[65];
  const int h = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int out_len = p.out_len_dev ? p.out_len_dev[h * p.out_len_stride] : p.out_len;
  const int V = p.V, P = p.P, W = P + 1;
  const int u = p.uidx ? p.uidx[h] : 0;
  const int T = p.uidx ? p.tlen[u] : p.T;
  const int TS = p.T;
  const float* __restrict__ logp = p.logp + (p.uidx ? (int64_t)u * p.logp_ustride : 0);
  float* xs = sm;                           // [T][W]: ids then blank
  float* ph = sm + (int64_t)TS * W;         // [T][2]: phi for a new label, phi for a repeated one
  const int* __restrict__ ids = p.ids + h * P;
  if (tid < P) sid[tid] = ids[tid];
  if (tid == P) sid[P] = p.blank;
  // (per-row lengths: a row of length 0 is at its first step whatever the launch's r_prev holds)
  const bool first = !p.r_prev || (p.out_len_stride && out_len == 0);
  const float* __restrict__ rp = first ? nullptr : p.r_prev + (int64_t)h * TS * 2;
  if (rp)
    for (int t = tid; t < T; t += 256) {
      const float a0 = rp[2 * t], a1 = rp[2 * t + 1];
      ph[2 * t] = lse2(a0, a1);
      ph[2 * t + 1] = a1;
    }
  __syncthreads();
  const int n = T * W;
  for (int base = tid; base < n; base += 4 * 256) {
    float v[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int idx = base + q * 256;
      if (idx < n) {
        const int t = idx / W, c = idx - t * W;
        v[q] = logp[(int64_t)t * V + sid[c]];
      }
    }
#pragma unroll
    for (int q = 0; q < 4; ++q)
      if (base + q * 256 < n) xs[base + q * 256] = v[q];
  }
  __syncthreads();
  if (!rp && tid == 0) {                    // first step: r_prev = (logzero, cumsum of blank)
    float cum = 0.f;
    for (int t = 0; t < T; ++t) {
      cum += xs[t * W + P];
      ph[2 * t] = lse2(LOGZERO, cum);
      ph[2 * t + 1] = cum;
    }
  }
  if (!rp) __syncthreads();
  const int start = max(out_len, 1);
  const float* __restrict__ pc = ph;
  if (w == 0) {
    const int j = lane;
    const bool act = j < P;
    const int id = act ? sid[j] : 0;
    const int q = (act && id == p.last[h]) ? 1 : 0;     // repeated label: phi = r_prev[t][1]
    float* __restrict__ rn = act ? p.r_new + ((int64_t)h * P + j) * TS * 2 : nullptr;
    const int jj = act ? j : 0;
    float r0 = LOGZERO, r1 = LOGZERO;
    for (int t = 0; t < min(start, T); ++t) {
      float a0 = LOGZERO;
      if (t == 0 && out_len == 0) a0 = act ? xs[jj] : LOGZERO;
      if (act) { rn[t * 2 + 0] = a0; rn[t * 2 + 1] = LOGZERO; }
      r0 = a0;
    }
#pragma unroll 4
    for (int t = start; t < T; ++t) {
      const float phi = pc[2 * (t - 1) + q];
      const float x0 = xs[t * W + jj];
      const float xb = xs[t * W + P];
      const float n0 = lse2_fast(r0, phi) + x0;
      const float n1 = lse2_fast(r0, r1) + xb;
      r0 = n0; r1 = n1;
      if (act) { rn[t * 2 + 0] = r0; rn[t * 2 + 1] = r1; }
    }
  }
  // psi of candidate j (waves 1-3, beside wave 0's recursion): logsumexp over {r0(start-1)} U
  // {phi(t-1) + x0(t), t in [start, T)}
  const float rsum_last = pc[2 * (T - 1)];          // logsumexp(r_prev[T-1]) (the eos score)
  for (int j = w - 1; w > 0 && j < P; j += 3) {
    const int id = sid[j];
    const int q = id == p.last[h] ? 1 : 0;
    const float r0i = (out_len == 0) ? xs[j] : LOGZERO;  // r0 at frame start - 1 (= 0 when out_len == 0)
    float m = lane == 0 ? r0i : -INFINITY;
    for (int t = start + lane; t < T; t += 64) m = fmaxf(m, pc[2 * (t - 1) + q] + xs[t * W + j]);
    m = wave_max(m);
    float sum = lane == 0 ? expf(r0i - m) : 0.f;
    for (int t = start + lane; t < T; t += 64) sum += expf(pc[2 * (t - 1) + q] + xs[t * W + j] - m);
    sum = wave_sum(sum);
    if (lane == 0) {
      float psi = m + logf(sum);
      if (id == p.blank) psi = LOGZERO;
      if (id == p.eos) psi = rsum_last;
      p.psi[h * (P + 1) + j] = psi;
    }
  }
  if (tid == 0) p.psi[h * (P + 1) + P] = rsum_last;
}

}  // namespace

extern "C" int avsr_ctc_prefix(const avsr_ctc_prefix_params* p, void* stream) {
  if (!p || p->n <= 0) return AVSR_E_ARG;
  if (p->P < 1 || p->P > 64 || p->T < 1) return AVSR_E_SHAPE;
  if (p->out_len_stride && !p->out_len_dev) return AVSR_E_ARG;
  const size_t lds = (size_t)p->T * (p->P + 1 + 2) * sizeof(float);
  if (lds <= 64 * 1024)
    hipLaunchKernelGGL(ctc_prefix_lds_kernel, dim3(p->n), dim3(256), lds, (hipStream_t)stream, *p);
  else
    hipLaunchKernelGGL(ctc_prefix_kernel, dim3(p->n), dim3(64), 0, (hipStream_t)stream, *p);
  AVSR_CHECK_LAUNCH();
  return 0;
}
