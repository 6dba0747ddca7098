// N-gram LM shallow fusion (declaration and contract: include/avsr_hip.h avsr_ngram_step /
// avsr_ngram_score_seqs; host side and the scoring rule: avsr_amd/ngram_lm.py).
//   avsr_ngram_step        one wave per hypothesis row, once per search step after the pre-beam
//                          (and the hot-word widening): lane c scores column c of the row's P ids
//                          columns and eos from the row's LM state
//   avsr_ngram_score_seqs  one thread per complete hypothesis (the two-pass decoder)
// Both walk the backoff automaton with ngram_lookup below. Integer logic, a binary search per
// context level and at most order - 1 fp32 additions per token; latency-bound like the other
// bookkeeping kernels: plain loads and stores, no LDS.
#include "common.h"

namespace {

// score and successor of token v (0 <= v < V) at node n: the rule of avsr_amd/ngram_lm.py. The
// backoff weights add up in fp32 in the order the contexts are left, then the entry's logp.
AVSR_DEV void ngram_lookup(const avsr_ngram_lm& m, int n, int v, float& score, int& next) {
  float acc = 0.f;
  for (int d = 0; d < AVSR_NGRAM_MAX_ORDER && n != 0; ++d) {   // (a context has at most order - 1 tokens)
    int lo = m.child_off[n];
    const int end = m.child_off[n + 1];
    int hi = end;
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (m.tok[mid] < v) lo = mid + 1; else hi = mid;
    }
    if (lo < end && m.tok[lo] == v) { score = acc + m.logp[lo]; next = m.next[lo]; return; }
    acc += m.backoff[n];
    n = m.fail[n];
  }
  score = acc + m.uni_logp[v];
  next = m.uni_next[v];
}

AVSR_DEV int ngram_state(const avsr_ngram_lm& m, int n) {
  return (unsigned)n < (unsigned)m.nodes ? n : m.start;      // (a row no search step has written yet)
}

__global__ __launch_bounds__(64) void ngram_step_kernel(avsr_ngram_params p) {
  const int r = blockIdx.x, c = threadIdx.x, W = p.P + 1;
  if (c >= W) return;
  const int n = ngram_state(p.lm, p.state[r]);
  const int v = c < p.P ? p.ids[r * p.P + c] : p.eos;
  float s = 0.f;
  int nx = n;
  // a blank column is padding of the hot-word widening: never selected
  if (v != p.blank && (unsigned)v < (unsigned)p.lm.V) ngram_lookup(p.lm, n, v, s, nx);
  p.out[r * W + c] = s;
  p.out_next[r * W + c] = nx;
}

__global__ __launch_bounds__(64) void ngram_score_seqs_kernel(avsr_ngram_seq_params p) {
  const int b = blockIdx.x * 64 + threadIdx.x;
  if (b >= p.n) return;
  const int L1 = p.L + 1;
  int n = p.lm.start;
  bool ended = false;
  for (int j = 0; j < L1; ++j) {
    float s = 0.f;
    if (!ended) {
      int v = j < p.L ? p.tokens[(int64_t)b * p.L + j] : p.eos;
      if (v < 0) v = p.eos;                                // -1 padding: the hypothesis ends here
      ended = v == p.eos;
      int nx = n;
      if ((unsigned)v < (unsigned)p.lm.V) ngram_lookup(p.lm, n, v, s, nx);
      n = nx;
    }
    p.out[(int64_t)b * L1 + j] = s;
  }
}

int check_lm(const avsr_ngram_lm& m) {
  if (m.order < 1 || m.order > AVSR_NGRAM_MAX_ORDER || m.nodes < 1 || m.V < 1) return AVSR_E_SHAPE;
  if ((unsigned)m.start >= (unsigned)m.nodes) return AVSR_E_SHAPE;
  if (!m.child_off || !m.backoff || !m.fail || !m.uni_logp || !m.uni_next) return AVSR_E_ARG;
  // tok / logp / next may be NULL for a model without entries below the unigram level: every span
  // is empty then and they are never read; all three or none
  if ((!m.tok || !m.logp || !m.next) && (m.tok || m.logp || m.next)) return AVSR_E_ARG;
  return 0;
}

}  // namespace

extern "C" int avsr_ngram_step(const avsr_ngram_params* p, void* stream) {
  if (!p || p->R <= 0) return p ? 0 : AVSR_E_ARG;
  if (p->P < 1 || p->P + 1 > 64) return AVSR_E_SHAPE;
  if (const int e = check_lm(p->lm)) return e;
  if (!p->state || !p->ids || !p->out || !p->out_next) return AVSR_E_ARG;
  hipLaunchKernelGGL(ngram_step_kernel, dim3(p->R), dim3(64), 0, (hipStream_t)stream, *p);
  AVSR_CHECK_LAUNCH();
  return 0;
}

extern "C" int avsr_ngram_score_seqs(const avsr_ngram_seq_params* p, void* stream) {
  if (!p || p->n <= 0) return p ? 0 : AVSR_E_ARG;
  if (p->L < 0) return AVSR_E_SHAPE;
  if (const int e = check_lm(p->lm)) return e;
  if ((p->L > 0 && !p->tokens) || !p->out) return AVSR_E_ARG;
  hipLaunchKernelGGL(ngram_score_seqs_kernel, dim3((p->n + 63) / 64), dim3(64), 0, (hipStream_t)stream, *p);
  AVSR_CHECK_LAUNCH();
  return 0;
}
