// Hot-word biasing of the device beam search (declaration and contract: include/avsr_hip.h
// avsr_hotword_step; host side and semantics: avsr_amd/hotwords.py).
// One wave per hypothesis row, once per search step between the pre-beam and the CTC prefix
// scores: lanes [P, P + C) write the row's continuation candidates (the children of its tree node
// that the pre-beam lacks), then lane c < P + C + 1 scores column c (the last one is eos). Integer
// logic and one fp32 product per column; latency-bound like the other bookkeeping kernels.
#include "common.h"

namespace {

// child(n, v) or -1: binary search of node n's span of the token-sorted CSR arrays
AVSR_DEV int hw_child(const avsr_hotword_params& p, int n, int v) {
  int lo = p.child_off[n];
  const int end = p.child_off[n + 1];
  int hi = end;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (p.child_tok[mid] < v) lo = mid + 1; else hi = mid;
  }
  return (lo < end && p.child_tok[lo] == v) ? p.child_node[lo] : -1;
}
// where a match on m leaves the hypothesis: a completed phrase with no longer one goes back to the root
AVSR_DEV int hw_land(const avsr_hotword_params& p, int m) {
  return (p.terminal[m] && p.child_off[m] == p.child_off[m + 1]) ? 0 : m;
}

__global__ __launch_bounds__(64) void hotword_step_kernel(avsr_hotword_params p) {
  const int r = blockIdx.x, c = threadIdx.x;
  const int Pw = p.P + p.C, W = Pw + 1;
  int n = p.node[r];
  if ((unsigned)n >= (unsigned)p.nodes) n = 0;            // (a row no search step has written yet)
  int id = p.blank;
  if (c < p.P) {
    id = p.ids_pre[r * p.P + c];
  } else if (c < Pw && n != 0) {
    // continuation j of a started phrase: child j of n in token order, unless the pre-beam has it
    const int j = c - p.P, e = p.child_off[n] + j;
    if (e < p.child_off[n + 1]) {
      id = p.child_tok[e];
      for (int q = 0; q < p.P; ++q)
        if (p.ids_pre[r * p.P + q] == id) { id = p.blank; break; }
    }
  } else if (c == Pw) {
    id = p.eos;
  }
  if (c >= W) return;
  if (c < Pw) p.ids[r * Pw + c] = id;
  int k, nx;
  const int m = (id == p.eos || id == p.blank) ? -1 : hw_child(p, n, id);
  if (m >= 0) {
    k = 1; nx = hw_land(p, m);
  } else {
    k = -p.pend[n]; nx = 0;
    if (id != p.eos && id != p.blank && n != 0) {          // restart on the mismatching token
      const int m0 = hw_child(p, 0, id);
      if (m0 >= 0) { k += 1; nx = hw_land(p, m0); }
    }
  }
  p.bonus[r * W + c] = p.beta * (float)k;
  p.next[r * W + c] = nx;
}

}  // namespace

extern "C" int avsr_hotword_step(const avsr_hotword_params* p, void* stream) {
  if (!p || p->R <= 0) return p ? 0 : AVSR_E_ARG;
  if (p->P < 1 || p->C < 0 || p->C > AVSR_HOTWORD_C || p->P + p->C + 1 > 64 || p->nodes < 1) return AVSR_E_SHAPE;
  if (!p->child_off || !p->child_tok || !p->child_node || !p->pend || !p->terminal || !p->node || !p->ids_pre ||
      !p->ids || !p->bonus || !p->next)
    return AVSR_E_ARG;
  hipLaunchKernelGGL(hotword_step_kernel, dim3(p->R), dim3(64), 0, (hipStream_t)stream, *p);
  AVSR_CHECK_LAUNCH();
  return 0;
}
