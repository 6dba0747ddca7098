// Loss kernels of the joint CTC / attention objective (include/avsr_hip.h):
// row log-sum-exp, label-smoothing KL (+argmax accuracy), CTC alpha/beta/occupancy and
// the logits gradients, plus the on-device loss combination. One 256-thread block per row
// for the V = 5049 row reductions; one block per utterance for the CTC recursions (the
// T-loop is sequential, states are spread over the block's threads, one barrier per step).
#include "common.h"

namespace {

constexpr float NEG = -1e30f;

AVSR_DEV float lse2(float a, float b) {
  const float m = fmaxf(a, b);
  return m <= NEG ? NEG : m + logf(expf(a - m) + expf(b - m));
}
AVSR_DEV float lse3(float a, float b, float c) {
  const float m = fmaxf(a, fmaxf(b, c));
  return m <= NEG ? NEG : m + logf(expf(a - m) + expf(b - m) + expf(c - m));
}

// CTC recursion step: hardware exp2 / log2 (v_exp_f32 / v_log_f32, ~1 ulp) instead of the
// libm sequences on the recursion's dependent chain (measured 408 -> 352 us per C2 batch);
// the max term contributes exp(0) = 1 exactly
AVSR_DEV float lse3_fast(float a, float b, float c) {
  const float m = fmaxf(a, fmaxf(b, c));
  return m <= NEG ? NEG : m + __logf(__expf(a - m) + __expf(b - m) + __expf(c - m));
}

// block-wide reductions (256 threads)
AVSR_DEV float block_max(float v, float* sh) {
  v = wave_max(v);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  v = fmaxf(fmaxf(sh[0], sh[1]), fmaxf(sh[2], sh[3]));
  __syncthreads();
  return v;
}
AVSR_DEV float block_sum(float v, float* sh) {
  v = wave_sum(v);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  v = sh[0] + sh[1] + sh[2] + sh[3];
  __syncthreads();
  return v;
}

// per-row statistics: max, sum exp (relative to max), sum x, argmax (first index)
template <typename T>
AVSR_DEV void row_stats(const T* x, int V, float* sh, float& mx, float& se, float& sx, int& amax) {
  constexpr int VE = VecW<T>::VE;
  float m = NEG, s = 0.f, t = 0.f, bv = NEG;
  int bi = 0x7fffffff;
  for (int c0 = threadIdx.x * VE; c0 < V; c0 += 256 * VE) {
    float v[VE];
    ldv(x + c0, v);
#pragma unroll
    for (int j = 0; j < VE; ++j) {
      if (c0 + j < V) {
        const float xv = v[j];
        if (xv > m) { s = s * expf(m - xv) + 1.f; m = xv; }
        else s += expf(xv - m);
        t += xv;
        if (xv > bv) { bv = xv; bi = c0 + j; }
      }
    }
  }
  mx = block_max(m, sh);
  se = block_sum(s * expf(m - mx), sh);
  sx = block_sum(t, sh);
  // argmax: max value, smallest index among ties
  const float gv = mx;
  int cand = bv == gv ? bi : 0x7fffffff;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) cand = min(cand, __shfl_xor(cand, o, 64));
  __shared__ int shi[4];
  if ((threadIdx.x & 63) == 0) shi[threadIdx.x >> 6] = cand;
  __syncthreads();
  amax = min(min(shi[0], shi[1]), min(shi[2], shi[3]));
  __syncthreads();
}

template <typename T, int MODE>  // MODE 0: lse only; 1: label smoothing fwd
__global__ __launch_bounds__(256) void xent_fwd_kernel(avsr_xent_params p) {
  __shared__ float sh[4];
  const int row = blockIdx.x;
  const T* x = (const T*)p.x + (int64_t)row * p.ldx;
  float mx, se, sx;
  int am;
  row_stats<T>(x, p.V, sh, mx, se, sx, am);
  const float lse = mx + logf(se);
  if (threadIdx.x == 0) {
    p.lse[row] = lse;
    if (MODE == 1) {
      const int tg = p.target[row];
      if (tg < 0) {
        p.row_loss[row] = 0.f;
        if (p.row_correct) p.row_correct[row] = -1;
      } else {
        const float V = (float)p.V, sm = p.smoothing;
        const float e = sm / (V - 1.f), conf = 1.f - sm;
        const float xt = to_f(x[tg]);
        const float cst = (e > 0.f ? (V - 1.f) * e * logf(e) : 0.f) + (conf > 0.f ? conf * logf(conf) : 0.f);
        p.row_loss[row] = cst + lse - (e * (sx - xt) + conf * xt);
        if (p.row_correct) p.row_correct[row] = am == tg ? 1 : 0;
      }
    }
  }
}

template <typename T>
__global__ __launch_bounds__(256) void lsm_bwd_kernel(avsr_xent_params p) {
  constexpr int VE = VecW<T>::VE;
  const int row = blockIdx.x;
  const T* x = (const T*)p.x + (int64_t)row * p.ldx;
  T* dx = (T*)p.dx + (int64_t)row * p.lddx;
  const int tg = p.target[row];
  const float scale = tg < 0 ? 0.f : (*p.dloss) * p.coef;
  const float lse = p.lse[row];
  const float e = p.smoothing / (float)(p.V - 1), conf = 1.f - p.smoothing;
  for (int c0 = threadIdx.x * VE; c0 < p.lddx; c0 += 256 * VE) {
    float v[VE], o[VE];
    if (c0 < p.V) ldv(x + c0, v);
#pragma unroll
    for (int j = 0; j < VE; ++j) {
      const int c = c0 + j;
      o[j] = c < p.V ? scale * (expf(v[j] - lse) - (c == tg ? conf : e)) : 0.f;
    }
    stv(dx + c0, o);
  }
}

// ------------------------------------------------------------------------------- CTC
AVSR_DEV int ext_label(const int* lab, int s) { return (s & 1) ? lab[s >> 1] : 0; }

// One block per utterance; the recursions are sequential in t, so every global access is
// taken off the per-step critical path: extended labels / skip flags live in LDS, and the
// emissions lp(t, s) = x[t][l'(s)] - lse[t] (and, for the beta pass, alpha) are gathered
// cooperatively into LDS in chunks of CH time steps -- one exposed memory latency per chunk
// instead of one per step.
constexpr int CTC_CHUNK = 6144;   // floats per LDS chunk buffer

template <typename T>
__global__ __launch_bounds__(256) void ctc_fwd_kernel(avsr_ctc_params p) {
  const int b = blockIdx.x, tid = threadIdx.x;
  const int L = p.label_len[b], Tb = min(p.in_len[b], p.T), S = 2 * L + 1;
  const int SS = 2 * p.Lmax + 1;
  const int* lab = p.labels + (int64_t)b * p.Lmax;
  const T* X = (const T*)p.x + (int64_t)b * p.T * p.ldx;
  const float* LSE = p.lse + (int64_t)b * p.T;
  float* A = p.alpha + (int64_t)b * p.T * SS;
  float* G = p.gamma + (int64_t)b * p.T * SS;
  __shared__ float buf[2][1024];
  __shared__ float E[CTC_CHUNK], AC[CTC_CHUNK];
  __shared__ int kl[1024];
  __shared__ unsigned char sk[1024];
  __shared__ float logp_s;
  if (S > 1024 || Tb <= 0) {   // unsupported label length or empty input: zero_infinity semantics
    for (int i = tid; i < p.T * SS; i += 256) G[i] = 0.f;
    if (tid == 0) p.nll[b] = 0.f;
    return;
  }
  const int CH = max(1, min(64, CTC_CHUNK / S));
  for (int s = tid; s < S; s += 256) kl[s] = ext_label(lab, s);
  __syncthreads();
  for (int s = tid; s < S; s += 256) sk[s] = s >= 2 && (s & 1) && kl[s] != kl[s - 2];
  // E[(t - t0) * S + s] = lp(t, s) for t in [t0, t0 + n); optionally AC = alpha of the same range
  auto load = [&](int t0, int n, bool with_alpha) {
    for (int i = tid; i < n * S; i += 256) {
      const int dt = i / S, s = i - dt * S, t = t0 + dt;
      E[i] = to_f(X[(int64_t)t * p.ldx + kl[s]]) - LSE[t];
      if (with_alpha) AC[i] = A[(int64_t)t * SS + s];
    }
  };
  __syncthreads();
  // alpha
  int t0 = 0;
  load(0, min(CH, Tb), false);
  __syncthreads();
  for (int s = tid; s < S; s += 256) {
    const float a0 = s < 2 ? E[s] : NEG;
    buf[0][s] = a0;
    A[s] = a0;
  }
  __syncthreads();
  for (int t = 1; t < Tb; ++t) {
    if (t - t0 >= CH) {
      t0 = t;
      load(t0, min(CH, Tb - t0), false);
      __syncthreads();
    }
    const float* prev = buf[(t - 1) & 1];
    float* cur = buf[t & 1];
    const float* e = E + (t - t0) * S;
    for (int s = tid; s < S; s += 256) {
      const float a1 = s >= 1 ? prev[s - 1] : NEG;
      const float a2 = sk[s] ? prev[s - 2] : NEG;
      const float v = lse3_fast(prev[s], a1, a2);
      const float r = v <= NEG ? NEG : v + e[s];
      cur[s] = r;
      A[(int64_t)t * SS + s] = r;
    }
    __syncthreads();
  }
  if (tid == 0) {
    const float* last = buf[(Tb - 1) & 1];
    logp_s = S > 1 ? lse2(last[S - 1], last[S - 2]) : last[S - 1];
  }
  __syncthreads();
  const float logp = logp_s;
  const bool feasible = logp > NEG * 0.5f;
  if (tid == 0) p.nll[b] = feasible ? -logp : 0.f;
  // beta (reuse buf), occupancy gamma_t(s) = exp(alpha + beta - lp - logP)
  for (int i = tid; i < p.T * SS; i += 256) {
    const int t = i / SS;
    if (t >= Tb || !feasible || (i % SS) >= S) G[i] = 0.f;
  }
  if (!feasible) return;
  __syncthreads();                       // alpha in global memory visible to the whole block
  t0 = max(0, Tb - CH);
  load(t0, Tb - t0, true);
  __syncthreads();
  for (int s = tid; s < S; s += 256) {
    const int i = (Tb - 1 - t0) * S + s;
    const float l = E[i];
    const float b0 = s >= S - 2 ? l : NEG;
    buf[(Tb - 1) & 1][s] = b0;
    const float a = AC[i];
    G[(int64_t)(Tb - 1) * SS + s] = (a <= NEG || b0 <= NEG) ? 0.f : expf(a + b0 - l - logp);
  }
  __syncthreads();
  for (int t = Tb - 2; t >= 0; --t) {
    if (t < t0) {
      t0 = max(0, t - CH + 1);
      load(t0, t + 1 - t0, true);
      __syncthreads();
    }
    const float* nxt = buf[(t + 1) & 1];
    float* cur = buf[t & 1];
    const int base = (t - t0) * S;
    for (int s = tid; s < S; s += 256) {
      const float b1 = s + 1 < S ? nxt[s + 1] : NEG;
      const float b2 = (s + 2 < S && sk[s + 2]) ? nxt[s + 2] : NEG;
      const float v = lse3_fast(nxt[s], b1, b2);
      const float l = E[base + s];
      const float r = v <= NEG ? NEG : v + l;
      cur[s] = r;
      const float a = AC[base + s];
      G[(int64_t)t * SS + s] = (a <= NEG || r <= NEG) ? 0.f : expf(a + r - l - logp);
    }
    __syncthreads();
  }
}

// Forced alignment: the max / argmax form of the alpha recursion above, same structure (one
// block per utterance, states strided over the threads, d ping-pongs in LDS, emissions gathered
// into LDS in chunks of frames). Each step stores one back-pointer byte per state (0, 1, 2 =
// came from s, s-1, s-2) to the caller's workspace. The backtrack is a T-long dependent chain
// on one lane: it reads its pointers from LDS (~50 cycles per dependent read, against ~200 for
// an L2 hit per step), which the whole block refills with dword loads, a chunk of frames at a
// time, and the block then writes the chunk's tokens together. Measured ~0.27 us per frame
// (B = 8, T = 375, L ~ 60: 114 us), whatever S <= 256 is: the step's two LDS round trips and
// its barrier, not the gathers.
constexpr int ALI_FRAMES = 256;   // frames per backtrack chunk (upper bound)

template <typename T>
__global__ __launch_bounds__(256) void ctc_align_kernel(avsr_ctc_align_params p) {
  const int b = blockIdx.x, tid = threadIdx.x;
  const int L = p.label_len[b], Tb = min(p.in_len[b], p.T), S = 2 * L + 1;
  const int SS = 2 * p.Lmax + 1;
  const int* lab = p.labels + (int64_t)b * p.Lmax;
  const T* X = (const T*)p.x + (int64_t)b * p.T * p.ldx;
  const float* LSE = p.lse + (int64_t)b * p.T;
  unsigned char* BP = p.ws + (int64_t)b * p.T * SS;
  int* ALI = p.ali + (int64_t)b * p.T;
  constexpr float NINF = -__builtin_inff();
  __shared__ float buf[2][1024 + 2];
  __shared__ float E[CTC_CHUNK];
  __shared__ int kl[1024];
  __shared__ unsigned char sk[1024];
  __shared__ int path[ALI_FRAMES];
  __shared__ int bad, fin_s;
  if (tid == 0) bad = 0;
  __syncthreads();
  const bool shape_ok = L >= 0 && L <= p.Lmax && Tb > 0;
  if (shape_ok) {
    for (int s = tid; s < S; s += 256) {
      int k = (s & 1) ? lab[s >> 1] : p.blank;
      if (k < 0 || k >= p.V) { bad = 1; k = p.blank; }
      kl[s] = k;
    }
  }
  __syncthreads();
  auto infeasible = [&]() {
    for (int t = tid; t < p.T; t += 256) ALI[t] = -1;
    if (tid == 0) { p.score[b] = 0.f; p.feasible[b] = 0; }
  };
  if (!shape_ok || bad) { infeasible(); return; }
  for (int s = tid; s < S; s += 256) sk[s] = s >= 2 && kl[s] != p.blank && kl[s] != kl[s - 2];
  const int CH = max(1, min(64, CTC_CHUNK / S));
  // The gathers of a chunk are issued into registers without a wait between them (indices
  // clamped instead of branched around) while the steps of the chunk before run: a step's
  // barrier waits for LDS only, so the loads stay in flight across it, and `stash` finds them
  // done when it moves them to LDS.
  constexpr int EPT = CTC_CHUNK / 256;
  float ex[EPT], el[EPT];
  const int q0 = tid / S, r0 = tid - q0 * S, qs = 256 / S, rs = 256 - qs * S;
  auto fetch = [&](int c0, int n) {
    int dt = q0, s = r0;              // element tid + 256 j is (frame c0 + dt, state s): no division per element
#pragma unroll
    for (int j = 0; j < EPT; ++j) {
      const bool in = dt < n;
      const int t = c0 + (in ? dt : n - 1), ss = in ? s : S - 1;
      ex[j] = to_f(X[(int64_t)t * p.ldx + kl[ss]]);
      el[j] = LSE[t];
      s += rs; dt += qs;
      if (s >= S) { s -= S; ++dt; }
    }
  };
  auto stash = [&](int n) {
#pragma unroll
    for (int j = 0; j < EPT; ++j)
      if (tid + 256 * j < n * S) E[tid + 256 * j] = ex[j] - el[j];
  };
  int t0 = 0, n_next = Tb > CH ? min(CH, Tb - CH) : 0;
  fetch(0, min(CH, Tb));
  stash(min(CH, Tb));
  if (n_next) fetch(CH, n_next);
  __syncthreads();
  // state s lives in cell s + 2: the two cells in front stay -inf, so s - 1 and s - 2 need no
  // branch and a step is one batch of LDS reads (three d, skip flag, emission), one wait
  if (tid < 2) buf[0][tid] = buf[1][tid] = NINF;
  for (int s = tid; s < S; s += 256) buf[0][s + 2] = s < 2 ? E[s] : NINF;
  __syncthreads();
  for (int t = 1; t < Tb; ++t) {
    if (t - t0 >= CH) {
      t0 = t;
      stash(n_next);                  // every thread is past the last step's barrier: E is free
      n_next = t0 + CH < Tb ? min(CH, Tb - t0 - CH) : 0;
      if (n_next) fetch(t0 + CH, n_next);
      __syncthreads();
    }
    const float* prev = buf[(t - 1) & 1];
    float* cur = buf[t & 1] + 2;
    const float* e = E + (t - t0) * S;
    unsigned char* bp = BP + (int64_t)t * SS;
    for (int s = tid; s < S; s += 256) {
      const float c0 = prev[s + 2], c1 = prev[s + 1], c2r = prev[s], es = e[s];
      const float c2 = sk[s] ? c2r : NINF;
      float m = c0;
      int k = 0;
      if (c1 > m) { m = c1; k = 1; }
      if (c2 > m) { m = c2; k = 2; }
      cur[s] = m + es;                // -inf stays -inf: an unreachable state never wins, no NaN
      bp[s] = (unsigned char)k;
    }
    __syncthreads();
  }
  if (tid == 0) {
    const float* last = buf[(Tb - 1) & 1] + 2;
    const int fs = S > 1 ? (last[S - 1] > last[S - 2] ? S - 1 : S - 2) : 0;
    const bool ok = last[fs] > NINF;
    fin_s = ok ? fs : -1;
    if (ok) { p.score[b] = last[fs]; p.feasible[b] = 1; }
  }
  __syncthreads();                    // also: every back-pointer store is visible to the block
  if (fin_s < 0) { infeasible(); return; }
  for (int t = Tb + tid; t < p.T; t += 256) ALI[t] = -1;
  // backtrack, latest chunk of frames first; the pointer rows [t0, t1] are copied as aligned
  // dwords (the workspace rows are SS bytes, so a chunk starts at any byte offset `off`)
  unsigned char* PB = (unsigned char*)E;
  uint32_t* PW = (uint32_t*)E;
  const int CB = min(ALI_FRAMES, (CTC_CHUNK * 4 - 8) / SS);
  int s = fin_s;
  for (int t1 = Tb - 1; t1 >= 0; t1 -= CB) {
    const int c0 = max(0, t1 - CB + 1), n = t1 - c0 + 1;
    const unsigned char* g = BP + (int64_t)c0 * SS;
    const int off = (int)((uintptr_t)g & 3);
    const uint32_t* g4 = (const uint32_t*)(g - off);
    const int nw = (off + n * SS + 3) >> 2;
    for (int i = tid; i < nw; i += 256) PW[i] = g4[i];
    __syncthreads();
    if (tid == 0) {
      for (int t = t1; t >= c0; --t) {
        path[t - c0] = s;
        if (t > 0) s = max(s - (PB[off + (t - c0) * SS + s] & 3), 0);   // frame 0 has no pointers
      }
    }
    __syncthreads();
    for (int i = tid; i < n; i += 256) ALI[c0 + i] = kl[path[i]];
  }
}

template <typename T>
__global__ __launch_bounds__(256) void ctc_bwd_kernel(avsr_ctc_params p) {
  constexpr int VE = VecW<T>::VE;
  const int row = blockIdx.x, b = row / p.T, t = row % p.T;
  const int L = p.label_len[b], Tb = min(p.in_len[b], p.T), S = 2 * L + 1;
  const int SS = 2 * p.Lmax + 1;
  const int* lab = p.labels + (int64_t)b * p.Lmax;
  const bool active = t < Tb && p.nll[b] != 0.f && S <= 1024;
  const float scale = active ? (*p.dloss) * p.coef : 0.f;
  const T* x = (const T*)p.x + (int64_t)row * p.ldx;
  T* dx = (T*)p.dx + (int64_t)row * p.lddx;
  const float lse = p.lse[row];
  const float* G = p.gamma + ((int64_t)b * p.T + t) * SS;
  __shared__ float gsum_blank;
  __shared__ float sh[4];
  // The stored fp32 lse is off by up to half an ulp of |lse| (5e-7 at lse ~ 12), and so is
  // exp(x - lse) where the posterior is near 1 -- there the occupancy is near 1 too and the
  // gradient is their small difference. Renormalising by the row's own sum of exp(x - lse)
  // takes the error of lse out (the row is re-read from cache; active rows only).
  float gb = 0.f, se = 0.f;
  if (active) {
    for (int s = threadIdx.x * 2; s < S; s += 512) gb += G[s];
    for (int c0 = threadIdx.x * VE; c0 < p.V; c0 += 256 * VE) {
      float v[VE];
      ldv(x + c0, v);
#pragma unroll
      for (int j = 0; j < VE; ++j)
        if (c0 + j < p.V) se += expf(v[j] - lse);
    }
  }
  gb = block_sum(gb, sh);
  se = block_sum(se, sh);
  if (threadIdx.x == 0) gsum_blank = gb;
  __syncthreads();
  const float inv = active ? 1.f / se : 1.f;
  for (int c0 = threadIdx.x * VE; c0 < p.lddx; c0 += 256 * VE) {
    float v[VE], o[VE];
    if (c0 < p.V) ldv(x + c0, v);
#pragma unroll
    for (int j = 0; j < VE; ++j) {
      const int c = c0 + j;
      o[j] = c < p.V ? scale * (expf(v[j] - lse) * inv - (c == 0 ? gsum_blank : 0.f)) : 0.f;
    }
    stv(dx + c0, o);
  }
  __syncthreads();
  if (!active) return;
  // label columns: softmax - sum of the occupancies of every state carrying that label
  for (int i = threadIdx.x; i < L; i += 256) {
    const int k = lab[i];
    float g = 0.f;
    for (int j = 0; j < L; ++j)
      if (lab[j] == k) g += G[2 * j + 1];
    const float sm = expf(to_f(x[k]) - lse) * inv;
    dx[k] = from_f<T>(scale * (sm - g));
  }
}

__global__ void loss_finalize_kernel(int B, const float* nll, int rows, const float* row_loss,
                                     const int* row_correct, float mtl, int per_token, float* out) {
  __shared__ float sh[4];
  float a = 0.f, c = 0.f, n = 0.f, v = 0.f;
  for (int i = threadIdx.x; i < B; i += 256) a += nll[i];
  for (int i = threadIdx.x; i < rows; i += 256) {
    c += row_loss[i];
    if (row_correct) { const int rc = row_correct[i]; if (rc >= 0) { v += 1.f; n += (float)rc; } }
  }
  a = block_sum(a, sh); c = block_sum(c, sh); n = block_sum(n, sh); v = block_sum(v, sh);
  if (threadIdx.x == 0) {
    const float lc = a / (float)B, la = c / (per_token ? fmaxf(v, 1.f) : (float)B);
    out[0] = mtl * lc + (1.f - mtl) * la;
    out[1] = lc; out[2] = la; out[3] = v > 0.f ? n / v : 0.f;
  }
}

}  // namespace

extern "C" int avsr_row_lse(const avsr_xent_params* p, void* stream) {
  if (!p || p->ldx % 8) return AVSR_E_ALIGN;
  if (p->rows == 0) return 0;
  if (p->dtype == AVSR_BF16) hipLaunchKernelGGL((xent_fwd_kernel<bf16, 0>), dim3(p->rows), dim3(256), 0, (hipStream_t)stream, *p);
  else hipLaunchKernelGGL((xent_fwd_kernel<float, 0>), dim3(p->rows), dim3(256), 0, (hipStream_t)stream, *p);
  AVSR_CHECK_LAUNCH();
  return 0;
}

extern "C" int avsr_lsm_fwd(const avsr_xent_params* p, void* stream) {
  if (!p || p->ldx % 8 || !p->target || !p->row_loss) return AVSR_E_ARG;
  if (p->rows == 0) return 0;
  if (p->dtype == AVSR_BF16) hipLaunchKernelGGL((xent_fwd_kernel<bf16, 1>), dim3(p->rows), dim3(256), 0, (hipStream_t)stream, *p);
  else hipLaunchKernelGGL((xent_fwd_kernel<float, 1>), dim3(p->rows), dim3(256), 0, (hipStream_t)stream, *p);
  AVSR_CHECK_LAUNCH();
  return 0;
}

extern "C" int avsr_lsm_bwd(const avsr_xent_params* p, void* stream) {
  if (!p || p->lddx % 8 || !p->dloss || !p->dx) return AVSR_E_ARG;
  if (p->rows == 0) return 0;
  if (p->dtype == AVSR_BF16) hipLaunchKernelGGL(lsm_bwd_kernel<bf16>, dim3(p->rows), dim3(256), 0, (hipStream_t)stream, *p);
  else hipLaunchKernelGGL(lsm_bwd_kernel<float>, dim3(p->rows), dim3(256), 0, (hipStream_t)stream, *p);
  AVSR_CHECK_LAUNCH();
  return 0;
}

extern "C" int avsr_ctc_fwd(const avsr_ctc_params* p, void* stream) {
  if (!p || p->ldx % 8) return AVSR_E_ARG;
  if (2 * p->Lmax + 1 > 1024) return AVSR_E_SHAPE;
  if (p->B == 0) return 0;
  if (p->dtype == AVSR_BF16) hipLaunchKernelGGL(ctc_fwd_kernel<bf16>, dim3(p->B), dim3(256), 0, (hipStream_t)stream, *p);
  else hipLaunchKernelGGL(ctc_fwd_kernel<float>, dim3(p->B), dim3(256), 0, (hipStream_t)stream, *p);
  AVSR_CHECK_LAUNCH();
  return 0;
}

extern "C" int avsr_ctc_bwd(const avsr_ctc_params* p, void* stream) {
  if (!p || p->lddx % 8 || !p->dloss || !p->dx) return AVSR_E_ARG;
  if (p->B * p->T == 0) return 0;
  if (p->dtype == AVSR_BF16) hipLaunchKernelGGL(ctc_bwd_kernel<bf16>, dim3(p->B * p->T), dim3(256), 0, (hipStream_t)stream, *p);
  else hipLaunchKernelGGL(ctc_bwd_kernel<float>, dim3(p->B * p->T), dim3(256), 0, (hipStream_t)stream, *p);
  AVSR_CHECK_LAUNCH();
  return 0;
}

extern "C" int avsr_ctc_align(const avsr_ctc_align_params* p, void* stream) {
  if (!p || p->B < 0 || p->T < 0 || p->Lmax < 0 || p->V <= 0 || p->ldx < p->V || p->blank < 0 || p->blank >= p->V)
    return AVSR_E_ARG;
  if (p->dtype != AVSR_F32 && p->dtype != AVSR_BF16) return AVSR_E_DTYPE;
  if (2 * p->Lmax + 1 > 1024) return AVSR_E_SHAPE;
  if (p->B == 0) return 0;
  if (!p->label_len || !p->in_len || !p->ali || !p->score || !p->feasible || (p->Lmax > 0 && !p->labels))
    return AVSR_E_ARG;
  if (p->T > 0 && (!p->x || !p->lse || !p->ws)) return AVSR_E_ARG;
  if ((uintptr_t)p->ws & 3) return AVSR_E_ALIGN;
  if (p->dtype == AVSR_BF16) hipLaunchKernelGGL(ctc_align_kernel<bf16>, dim3(p->B), dim3(256), 0, (hipStream_t)stream, *p);
  else hipLaunchKernelGGL(ctc_align_kernel<float>, dim3(p->B), dim3(256), 0, (hipStream_t)stream, *p);
  AVSR_CHECK_LAUNCH();
  return 0;
}

extern "C" int avsr_loss_finalize(int B, const float* nll, int rows, const float* row_loss, const int* row_correct,
                                  float mtlalpha, int att_per_token, float* out, void* stream) {
  if (att_per_token && !row_correct) return AVSR_E_ARG;
  hipLaunchKernelGGL(loss_finalize_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, B, nll, rows, row_loss,
                     row_correct, mtlalpha, att_per_token, out);
  AVSR_CHECK_LAUNCH();
  return 0;
}
