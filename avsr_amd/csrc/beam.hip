// Beam selection, the device-side bookkeeping of the search and the state gather (declarations
// under "Joint CTC / attention beam search" and "Device-side beam bookkeeping" in
// include/avsr_hip.h):
//   avsr_beam_select           weighted scores + flat top-beam over (hyps x V)
//   avsr_beam_step_prep[_rows] ancestry row and key length of the step (shared / per-row position)
//   avsr_beam_kv_put[_rows]    the step's self-attention K / V rows into the cache
//   avsr_beam_post             the new running state, back-pointers, end detection of the step
//   avsr_beam_slot_reset       one slot of a decode session back to a fresh utterance
//   avsr_gather_rows           reorder per-hypothesis state (K/V caches, CTC variables)
// (the hot-word bonus that avsr_beam_select / avsr_beam_post optionally carry comes from
//  avsr_hotword_step, hotword.hip; the n-gram LM scores from avsr_ngram_step, ngram.hip)
// All fp32 math (double for the score sums); latency-bound: no host round trip inside a step.
#include "decode.h"

namespace {

// ---------------------------------------------------------------- beam selection
// weighted[h][v] = w_dec * dec[h][v] + w_ctc * (psi[h][v] - s_prev[h]) + score[h]
// (psi = LOGZERO for tokens outside the pre-beam, r_sum[T-1] for eos; batch_beam_search.py
// :228-260), flat top-`beam` over h*V + v; ties -> smaller flat index.
// Tokens outside a row's pre-beam have psi = LOGZERO, i.e. a weighted score below
// w_ctc * (LOGZERO - s_prev[h]) + score[h] (dec <= 0). The selection first runs over the
// candidates only (each row's P pre-beam tokens and eos: <= 256 per segment) and keeps that
// result when its beam-th score is above that bound for every row of the segment — then no
// other token can enter the top beam and the result equals the full scan; otherwise (fewer
// than `beam` finite candidates) it scans all rows x V as before.
// With a hot-word bonus (p.bonus, added between the CTC term and score[h]) the candidates are the
// row's P columns, continuation columns included, and eos. The candidate-only pass stays exact:
// only a token of ids[h] can match a tree edge and earn a positive bonus; every other token takes
// the eos column's value -beta * pend <= 0, so its score stays below the same bound, and the
// bonus of a candidate (|b| <= beta * the deepest phrase, a few units) is far inside the 1e-3
// relative margin under |w_ctc * LOGZERO| ~ 1e9.
// With an n-gram LM / a length bonus (p.lm, p.w_len; scores from avsr_ngram_step, ngram.hip) the
// sum takes the reference's order: w_dec*dec + w_len + w_lm*lm + w_ctc*(psi - s_prev) [+ bonus] +
// score[h]. A token outside a row's candidates takes an LM term of 0: it sits at w_ctc * LOGZERO ~
// -1e9 * w_ctc, where one fp32 step (>= 64 * w_ctc) exceeds any LM score, so the term would round
// away had it been computed. The candidates-only pass stays exact: a non-candidate's score is at
// most w_len + w_lm * lm_hi + w_ctc * (LOGZERO - s_prev[h]) + score[h] (dec <= 0, its LM term 0 <=
// w_lm * max(0, any score) <= w_lm * lm_hi, a bonus <= 0 as above), which is the bound the pass
// compares its beam-th score with; with both off (lm NULL, w_len 0) the expressions of before run.
// Every per-column quantity of (row h, token v) comes from one lookup, c = cand_col(h, v): the
// first column of ids[h] that holds v, or -1. Each reads it by its own rule:
//   psi        eos: column P; blank or c < 0: LOGZERO
//   bonus/next eos, blank or c < 0: column P (the eos column)
//   lm/lm_next eos: column P; blank or c < 0: none (-1: an LM term of 0, a successor of -1)
//   out_col    c < 0: P - 1 (scoring_idmap == -1 -> python index -1), eos and blank like any token
__global__ __launch_bounds__(256) void beam_select_kernel(avsr_beam_select_params p) {
  __shared__ float shv[4];
  __shared__ int shi[4];
  __shared__ int use_full;
  float tv[KMAX];
  int ti[KMAX];
  // segment (utterance) of this block: rows [r0, r0 + nrow); flat ids are segment-local
  const int u = blockIdx.x;
  const int r0 = p.nseg ? p.seg[u] : 0, nrow = p.nseg ? p.seg[u + 1] - r0 : p.n;
  const int beam = min(p.beam, nrow * p.V);
  const int total = nrow * p.V;
  const int W = p.P + 1;
  auto cand_col = [&](int h, int v) -> int {
    for (int c = 0; c < p.P; ++c)
      if (p.ids[h * p.P + c] == v) return c;
    return -1;
  };
  auto psi_of = [&](int h, int v, int c) -> float {
    if (v == p.eos) return p.psi[h * W + p.P];
    return v != p.blank && c >= 0 ? p.psi[h * W + c] : LOGZERO;
  };
  auto bonus_col = [&](int v, int c) -> int { return v != p.eos && v != p.blank && c >= 0 ? c : p.P; };
  auto lm_col = [&](int v, int c) -> int { return v == p.eos ? p.P : (v != p.blank ? c : -1); };
  const bool fused = p.lm || p.w_len != 0.f;            // shallow fusion: the reference's summation order
  auto weighted = [&](int f) -> float {
    const int h = r0 + f / p.V, v = f - (f / p.V) * p.V;
    if (p.score[h] == -INFINITY) return -INFINITY;      // a dead row of the device-side search
    const int c = cand_col(h, v);
    const float psi = psi_of(h, v, c);
    float w = 0.f;
    w += p.w_dec * (p.dec[(int64_t)h * p.ld + v]);
    if (fused) {
      w += p.w_len;
      if (p.lm) {
        const int lc = lm_col(v, c);
        w += p.w_lm * (lc >= 0 ? p.lm[h * W + lc] : 0.f);
      }
    }
    w += p.w_ctc * (psi - p.s_prev[h]);
    if (p.bonus) w += p.bonus[h * W + bonus_col(v, c)];
    w += p.score[h];
    return w;
  };
  auto insert = [&](float val, int id) {
#pragma unroll
    for (int k = 0; k < KMAX; ++k) {
      if (k < beam && (val > tv[k] || (val == tv[k] && id < ti[k]))) {
        const float t = tv[k]; const int w = ti[k];
        tv[k] = val; ti[k] = id; val = t; id = w;
      }
    }
  };
  // top-beam of the block's per-thread lists (written to out_*); returns the beam-th score
  auto select = [&]() -> float {
    int head = 0;
    float last = INFINITY;
    for (int r = 0; r < beam; ++r) {
      float v = -INFINITY; int id = 0x7fffffff;
#pragma unroll
      for (int k = 0; k < KMAX; ++k) if (k == head) { v = tv[k]; id = ti[k]; }
      const int mine = id;
      block_argmax256(v, id, shv, shi);
      if (mine == id && id != 0x7fffffff) ++head;
      last = v;
      if (threadIdx.x == 0 && id != 0x7fffffff) {     // (fewer candidates than beam: left to the full scan)
        const int h = r0 + id / p.V, tok = id - (id / p.V) * p.V;
        const int c = cand_col(h, tok);
        const float psi = psi_of(h, tok, c);
        const int o = u * p.beam + r;
        p.out_prev[o] = h;
        p.out_tok[o] = tok;
        p.out_col[o] = c >= 0 ? c : p.P - 1;
        p.out_score[o] = v;
        p.out_dec[o] = p.dec[(int64_t)h * p.ld + tok];
        p.out_ctc[o] = psi - p.s_prev[h];
        p.out_s[o] = psi;
        if (p.bonus) {
          const int bc = bonus_col(tok, c);
          p.out_bonus[o] = p.bonus[h * W + bc];
          if (p.out_next) p.out_next[o] = p.next[h * W + bc];
        }
        if (p.lm) {
          const int lc = lm_col(tok, c);
          p.out_lm[o] = lc >= 0 ? p.lm[h * W + lc] : 0.f;
          p.out_lm_next[o] = lc >= 0 ? p.lm_next[h * W + lc] : -1;
        }
      }
    }
    return last;
  };
  auto reset = [&]() {
#pragma unroll
    for (int k = 0; k < KMAX; ++k) { tv[k] = -INFINITY; ti[k] = 0x7fffffff; }
  };
  bool full = !(nrow * W <= 256 && p.w_ctc > 0.f);     // block-uniform
  {   // a segment with no live row (a finished utterance of the device-side search): nothing to select
    bool any = false;
    for (int hl = 0; hl < nrow; ++hl) any |= p.score[r0 + hl] != -INFINITY;
    if (!any) {
      for (int r = threadIdx.x; r < p.beam; r += 256) {
        const int o = u * p.beam + r;
        p.out_prev[o] = r0; p.out_tok[o] = p.eos; p.out_col[o] = p.P - 1; p.out_score[o] = -INFINITY;
        p.out_dec[o] = 0.f; p.out_ctc[o] = 0.f; p.out_s[o] = 0.f;
        if (p.bonus) { p.out_bonus[o] = 0.f; if (p.out_next) p.out_next[o] = 0; }
        if (p.lm) { p.out_lm[o] = 0.f; p.out_lm_next[o] = -1; }
      }
      return;
    }
  }
  if (!full) {
    reset();
    const int c = threadIdx.x;
    if (c < nrow * W) {
      const int hl = c / W, k = c - hl * W, h = r0 + hl;
      const int v = k < p.P ? p.ids[h * p.P + k] : p.eos;
      // eos once per row: as the extra candidate, not again as a pre-beam id. With hot words the
      // unused continuation columns hold blank: each (row, token) must enter the lists once, and a
      // blank is below the bound anyway
      const bool pad = (p.bonus || p.lm) && k < p.P && v == p.blank;
      if (!(k < p.P && v == p.eos) && !pad) insert(weighted(hl * p.V + v), hl * p.V + v);
    }
    const float last = select();
    if (threadIdx.x == 0) {
      // bound on any non-candidate's score (dec <= 0), with a relative margin for rounding
      float bound = -INFINITY;
      for (int hl = 0; hl < nrow; ++hl) {
        const int h = r0 + hl;
        float b = p.w_ctc * (LOGZERO - p.s_prev[h]) + p.score[h];
        if (fused) b += p.w_len + (p.lm ? p.w_lm * p.lm_hi : 0.f);
        bound = fmaxf(bound, b);
      }
      use_full = !(last > bound + 1e-3f * fabsf(bound));
    }
    __syncthreads();
    full = use_full != 0;
  }
  if (full) {
    reset();
    for (int f = threadIdx.x; f < total; f += 256) insert(weighted(f), f);
    select();
  }
}

// ---------------------------------------------------------------- device-side bookkeeping
// ps = 0: one shared position pos_p[0]; ps = 1: one per row (a decode session's rowpos)
__global__ __launch_bounds__(256) void beam_step_prep_kernel(int R, int Lmax, const int* pos_p, int ps, int* anc,
                                                             int* klen) {
  for (int r = blockIdx.x * 256 + threadIdx.x; r < R; r += gridDim.x * 256) {
    const int pos = pos_p[r * ps];
    anc[(int64_t)r * Lmax + pos] = pos * R + r;
    klen[r] = pos + 1;
  }
}

template <typename T>
__global__ __launch_bounds__(256) void beam_kv_put_kernel(int R, int D, const T* qkv, int64_t ld, T* ck, T* cv,
                                                          const int* pos_p, int ps) {
  const int nv = D / VecW<T>::VE;
  for (int e = blockIdx.x * 256 + threadIdx.x; e < R * nv; e += gridDim.x * 256) {
    const int r = e / nv, c = (e - r * nv) * VecW<T>::VE;
    const int pos = pos_p[r * ps];
    const int64_t dst = ((int64_t)pos * R + r) * D + c;
    *(v16*)(ck + dst) = *(const v16*)(qkv + (int64_t)r * ld + D + c);
    *(v16*)(cv + dst) = *(const v16*)(qkv + (int64_t)r * ld + 2 * D + c);
  }
}

// one workgroup: rows of the step (R <= 1024), then one thread per utterance. With p.upos the
// position is per utterance slot (upos[u]); a slot done before the step keeps it, every other
// advances, and rowpos[r] = upos[r / beam] is rewritten.
__global__ __launch_bounds__(256) void beam_post_kernel(avsr_beam_post_params p) {
  extern __shared__ __attribute__((aligned(16))) char sm[];
  double* od = (double*)sm;                   // [R] old decoder sums
  double* oc = od + p.R;                      // [R] old CTC sums
  double* oh = oc + p.R;                      // [R] old hot-word bonus sums (with p.sel_bonus only)
  double* ol = oh + (p.sel_bonus ? p.R : 0);  // [R] old LM sums (with p.sel_lm only)
  double* on = ol + (p.sel_lm ? p.R : 0);     // [R] old scored-token counts (with p.slen only)
  int* ended = (int*)(on + (p.slen ? p.R : 0));        // [R] 0 running, 1 eos, 2 forced eos at maxlen
  const int pos0 = p.upos ? 0 : p.pos[0];
  for (int r = threadIdx.x; r < p.R; r += 256) {
    od[r] = p.sdec[r]; oc[r] = p.sctc[r];
    if (p.sel_bonus) oh[r] = p.shw[r];
    if (p.sel_lm) ol[r] = p.slm[r];
    if (p.slen) on[r] = p.slen[r];
  }
  __syncthreads();
  for (int r = threadIdx.x; r < p.R; r += 256) {
    const int u = r / p.beam;
    const int pos = p.upos ? p.upos[u] : pos0;
    const int64_t so = (int64_t)pos * p.R;
    ended[r] = 0;
    if (p.done[u]) {                          // finished before this step: stays dead
      p.score[r] = -INFINITY;
      p.src[r] = r; p.src[p.R + r] = r * p.P;
      p.bp_prev[so + r] = r; p.bp_tok[so + r] = p.eos; p.end_flag[so + r] = 0;
      if (p.sel_bonus) p.node_out[r] = 0;
      if (p.sel_lm) p.lm_state_out[r] = p.lm_start;
      continue;
    }
    const int h = p.sel_prev[r], t = p.sel_tok[r];
    const float sc = p.sel_score[r];
    const double nd = od[h] + (double)p.sel_dec[r], nc = oc[h] + (double)p.sel_ctc[r];
    const bool forced = pos == p.maxlen[u] - 1;   // eos appended to every hypothesis at the last step
    const int e = forced ? 2 : (t == p.eos ? 1 : 0);
    ended[r] = e;
    p.bp_prev[so + r] = h; p.bp_tok[so + r] = t; p.end_flag[so + r] = e;
    if (e) { p.end_score[so + r] = sc; p.end_dec[so + r] = nd; p.end_ctc[so + r] = nc; }
    p.tok[r] = t;
    p.score[r] = e ? -INFINITY : sc;
    p.sdec[r] = nd; p.sctc[r] = nc; p.s_prev[r] = p.sel_s[r];
    if (p.sel_bonus) {
      const double nh = oh[h] + (double)p.sel_bonus[r];
      if (e) p.end_hw[so + r] = nh;
      p.shw[r] = nh;
      p.node_out[r] = p.sel_next[r];
    }
    if (p.sel_lm) {
      const double nl = ol[h] + (double)p.sel_lm[r];
      if (e) p.end_lm[so + r] = nl;
      p.slm[r] = nl;
      p.lm_state_out[r] = p.sel_lm_next[r];
    }
    if (p.slen) {                              // the forced eos is appended unscored: one token per step
      const double nn = on[h] + 1.0;
      if (e) p.end_len[so + r] = nn;
      p.slen[r] = nn;
    }
    p.src[r] = h; p.src[p.R + r] = h * p.P + p.sel_col[r];
  }
  __syncthreads();
  const int LB = p.Lmax + 3;
  for (int u = threadIdx.x; u < p.U; u += 256) {
    if (p.done[u]) continue;
    const int pos = p.upos ? p.upos[u] : pos0;
    const int64_t so = (int64_t)pos * p.R;
    bool any_live = false;
    float* bl = p.best_len + (int64_t)u * LB;
    for (int k = 0; k < p.beam; ++k) {         // this step's ended hypotheses, in selection order
      const int r = u * p.beam + k;
      if (!ended[r]) { any_live = true; continue; }
      const int len = pos + 2 + (ended[r] == 2 ? 1 : 0);     // sos + pos+1 tokens (+ the forced eos)
      const float s = p.end_score[so + r];
      if (len < LB && s > bl[len]) bl[len] = s;
      if (s > p.best_end[u]) p.best_end[u] = s;
    }
    bool det = false;
    if (p.end_detect && p.best_end[u] != -INFINITY) {
      int count = 0;
      for (int m = 0; m < 3; ++m) {
        const int len = pos - m;
        if (len >= 0 && len < LB && bl[len] != -INFINITY && (double)bl[len] - (double)p.best_end[u] < p.d_end) ++count;
      }
      det = count == 3;
    }
    if (det || !any_live || pos >= p.maxlen[u] - 1) {
      p.done[u] = 1;
      for (int k = 0; k < p.beam; ++k) p.score[u * p.beam + k] = -INFINITY;
    }
    if (p.upos) p.upos[u] = pos + 1;
  }
  __syncthreads();
  if (p.upos)
    for (int r = threadIdx.x; r < p.R; r += 256) p.rowpos[r] = p.upos[r / p.beam];
  if (threadIdx.x == 0) {
    int n = 0;
    for (int u = 0; u < p.U; ++u) n += p.done[u];
    p.done[p.U] = n;
    if (!p.upos) p.pos[0] = pos0 + 1;
  }
}

// slot p.slot of a decode session back to the state of a fresh utterance (only its rows)
__global__ __launch_bounds__(256) void beam_slot_reset_kernel(avsr_beam_slot_reset_params p) {
  const int u = p.slot, r0 = u * p.beam;
  for (int k = threadIdx.x; k < p.beam; k += 256) {
    const int r = r0 + k;
    p.rowpos[r] = 0;
    p.tok[r] = p.sos;
    p.score[r] = k == 0 ? 0.f : -INFINITY;
    p.sdec[r] = 0.0; p.sctc[r] = 0.0; p.s_prev[r] = 0.f;
    p.klen_mem[r] = p.tlen;
  }
  float* bl = p.best_len + (int64_t)u * (p.Lmax + 3);
  for (int k = threadIdx.x; k < p.Lmax + 3; k += 256) bl[k] = -INFINITY;
  if (threadIdx.x == 0) {
    p.upos[u] = 0;
    p.best_end[u] = -INFINITY;
    p.maxlen_arr[u] = p.maxlen;
    p.tlen_arr[u] = p.tlen;
    int n = 0;
    for (int v = 0; v < p.U; ++v) n += v == u ? 0 : p.done[v];
    p.done[u] = 0;
    p.done[p.U] = n;
  }
}

// ---------------------------------------------------------------- state gather
template <typename W>
__global__ __launch_bounds__(256) void gather_rows_kernel(int groups, int n, int64_t vecs, const W* src,
                                                          int64_t sg, int64_t sr, W* dst, int64_t dg, int64_t dr,
                                                          const int* idx) {
  const int64_t total = (int64_t)groups * n * vecs;
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
    const int64_t v = e % vecs, gi = e / vecs;
    const int i = (int)(gi % n), g = (int)(gi / n);
    dst[g * dg + i * dr + v] = src[g * sg + (int64_t)idx[i] * sr + v];
  }
}

}  // namespace

extern "C" int avsr_beam_select(const avsr_beam_select_params* p, void* stream) {
  if (!p || p->n <= 0) return AVSR_E_ARG;
  if (p->beam < 1 || p->beam > KMAX || p->P < 1 || p->nseg < 0) return AVSR_E_SHAPE;
  if (!p->nseg && p->beam > p->n * p->V) return AVSR_E_SHAPE;
  if (p->nseg && !p->seg) return AVSR_E_ARG;
  if (p->bonus && (!p->out_bonus || (p->out_next && !p->next))) return AVSR_E_ARG;
  if (p->lm && (!p->lm_next || !p->out_lm || !p->out_lm_next)) return AVSR_E_ARG;
  if (!(p->w_lm >= 0.f) || !(p->w_len == p->w_len)) return AVSR_E_ARG;
  hipLaunchKernelGGL(beam_select_kernel, dim3(p->nseg ? p->nseg : 1), dim3(256), 0, (hipStream_t)stream, *p);
  AVSR_CHECK_LAUNCH();
  return 0;
}

static int beam_step_prep(int R, int Lmax, const int* pos, int ps, int* anc, int* klen, void* stream) {
  if (R <= 0 || Lmax <= 0 || !pos || !anc || !klen) return AVSR_E_ARG;
  hipLaunchKernelGGL(beam_step_prep_kernel, dim3((R + 255) / 256), dim3(256), 0, (hipStream_t)stream, R, Lmax, pos, ps,
                     anc, klen);
  AVSR_CHECK_LAUNCH();
  return 0;
}
extern "C" int avsr_beam_step_prep(int R, int Lmax, const int* pos, int* anc, int* klen, void* stream) {
  return beam_step_prep(R, Lmax, pos, 0, anc, klen, stream);
}
extern "C" int avsr_beam_step_prep_rows(int R, int Lmax, const int* rowpos, int* anc, int* klen, void* stream) {
  return beam_step_prep(R, Lmax, rowpos, 1, anc, klen, stream);
}

static int beam_kv_put(int dtype, int R, int D, const void* qkv, int64_t ldqkv, void* cache_k, void* cache_v,
                       const int* pos, int ps, void* stream) {
  return avsr_by_dtype(dtype, [&](auto t) -> int {
    using T = decltype(t);
    constexpr int ve = VecW<T>::VE;
    if (R <= 0 || D % ve || ldqkv % ve || !pos) return AVSR_E_ARG;
    if (!avsr_aligned16(qkv) || !avsr_aligned16(cache_k) || !avsr_aligned16(cache_v)) return AVSR_E_ALIGN;
    const int g = avsr_grid((int64_t)R * D / ve, 256, 1024);
    hipLaunchKernelGGL(beam_kv_put_kernel<T>, dim3(g), dim3(256), 0, (hipStream_t)stream, R, D, (const T*)qkv, ldqkv,
                       (T*)cache_k, (T*)cache_v, pos, ps);
    AVSR_CHECK_LAUNCH();
    return 0;
  });
}
extern "C" int avsr_beam_kv_put(int dtype, int R, int D, const void* qkv, int64_t ldqkv, void* cache_k, void* cache_v,
                                const int* pos, void* stream) {
  return beam_kv_put(dtype, R, D, qkv, ldqkv, cache_k, cache_v, pos, 0, stream);
}
extern "C" int avsr_beam_kv_put_rows(int dtype, int R, int D, const void* qkv, int64_t ldqkv, void* cache_k,
                                     void* cache_v, const int* rowpos, void* stream) {
  return beam_kv_put(dtype, R, D, qkv, ldqkv, cache_k, cache_v, rowpos, 1, stream);
}

extern "C" int avsr_beam_post(const avsr_beam_post_params* p, void* stream) {
  if (!p || p->U <= 0 || p->beam <= 0 || p->R != p->U * p->beam || p->R > 2048) return AVSR_E_ARG;
  if (p->upos ? !p->rowpos : !p->pos) return AVSR_E_ARG;
  if (p->sel_bonus && (!p->sel_next || !p->shw || !p->end_hw || !p->node_out)) return AVSR_E_ARG;
  if (p->sel_lm && (!p->sel_lm_next || !p->slm || !p->end_lm || !p->lm_state_out)) return AVSR_E_ARG;
  if (p->slen && !p->end_len) return AVSR_E_ARG;
  const int sums = 2 + (p->sel_bonus ? 1 : 0) + (p->sel_lm ? 1 : 0) + (p->slen ? 1 : 0);
  const size_t lds = (size_t)p->R * (sums * sizeof(double) + sizeof(int));
  if (lds > 64 * 1024) return AVSR_E_SHAPE;
  hipLaunchKernelGGL(beam_post_kernel, dim3(1), dim3(256), lds, (hipStream_t)stream, *p);
  AVSR_CHECK_LAUNCH();
  return 0;
}

extern "C" int avsr_beam_slot_reset(const avsr_beam_slot_reset_params* p, void* stream) {
  if (!p || p->U <= 0 || p->beam <= 0 || p->R != p->U * p->beam || p->slot < 0 || p->slot >= p->U) return AVSR_E_ARG;
  if (p->maxlen < 1 || p->maxlen >= p->Lmax || p->tlen < 1) return AVSR_E_SHAPE;
  hipLaunchKernelGGL(beam_slot_reset_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, *p);
  AVSR_CHECK_LAUNCH();
  return 0;
}

extern "C" int avsr_gather_rows(int groups, int n, int64_t row_bytes, const void* src, int64_t src_gstride,
                                int64_t src_rstride, void* dst, int64_t dst_gstride, int64_t dst_rstride,
                                const int* idx, void* stream) {
  if (groups <= 0 || n <= 0 || row_bytes <= 0) return 0;
  const int64_t all = row_bytes | src_gstride | src_rstride | dst_gstride | dst_rstride;
  if (all % 16 == 0 && avsr_aligned16(src) && avsr_aligned16(dst)) {   // 16-byte words
    const int64_t vecs = row_bytes / 16;
    const int g = avsr_grid((int64_t)groups * n * vecs, 256, 2048);
    hipLaunchKernelGGL(gather_rows_kernel<uint4>, dim3(g), dim3(256), 0, (hipStream_t)stream, groups, n, vecs,
                       (const uint4*)src, src_gstride / 16, src_rstride / 16, (uint4*)dst, dst_gstride / 16,
                       dst_rstride / 16, idx);
  } else if (all % 4 == 0 && ((uintptr_t)src & 3) == 0 && ((uintptr_t)dst & 3) == 0) {   // 4-byte words
    const int64_t vecs = row_bytes / 4;
    const int g = avsr_grid((int64_t)groups * n * vecs, 256, 2048);
    hipLaunchKernelGGL(gather_rows_kernel<uint32_t>, dim3(g), dim3(256), 0, (hipStream_t)stream, groups, n, vecs,
                       (const uint32_t*)src, src_gstride / 4, src_rstride / 4, (uint32_t*)dst, dst_gstride / 4,
                       dst_rstride / 4, idx);
  } else {
    return AVSR_E_ALIGN;
  }
  AVSR_CHECK_LAUNCH();
  return 0;
}
