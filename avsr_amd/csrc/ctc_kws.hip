// avsr_ctc_kws (include/avsr_hip.h): keyword spotting on CTC posteriors, the CTC Viterbi of a
// keyword with a free start and a free end inside the utterance, for K keywords x U utterances in
// one launch (avsr_amd/kws.py).
//   One wavefront per (utterance, keyword), one state per lane: a keyword of L <= 32 pieces has
//   S = 2L - 1 <= 63 states (no outer blanks), so the whole DP row -- d and the start frame st it
//   carries -- lives in two registers per lane, and a frame is: the s-1 and s-2 neighbours by two
//   whole-wave DPP shifts each (v_mov_b32_dpp wave_shr:1; the lanes shifted in get -inf / -1, which
//   is the recursion's "no such state"), two compares, the free entry at state 0, one add. No LDS
//   and no barrier anywhere: a 256-thread block is four independent waves (four keywords of one
//   utterance), and avsr_ctc_align's per-frame LDS ping-pong + barrier (~0.27 us a frame) is gone.
//   The gathers logp[t][ext_s] and the filler logp[t][top[t]] do not depend on the DP: they are
//   issued KW_PF frames ahead into registers (the next block's loads are in flight while this
//   block's frames are computed; the filler's index, the first of two dependent loads, two blocks
//   ahead), so the loop's dependent chain is shift, max, max, add -- not a memory round trip. The
//   filler of a block is loaded one frame per lane and read back by v_readlane.
//   Lanes s >= S run the same code on the blank column with d that nothing reads (a state only
//   looks down); they keep the wave converged for the DPP moves.
#include "common.h"

namespace {

constexpr float NINF = -__builtin_inff();
constexpr int KW_PF = 8;          // frames of emissions in flight ahead of the DP

// lane l <- lane l - 1 over the whole wave; lane 0 keeps `fill`
AVSR_DEV float shr1f(float x, float fill) {
  return __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(fill), __float_as_int(x), 0x138, 0xf, 0xf, false));
}
AVSR_DEV int shr1i(int x, int fill) { return __builtin_amdgcn_update_dpp(fill, x, 0x138, 0xf, 0xf, false); }

template <bool FILL>
__global__ __launch_bounds__(256) void ctc_kws_kernel(avsr_ctc_kws_params p) {
  const int lane = threadIdx.x & 63;
  const int k = blockIdx.x * 4 + __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6), u = blockIdx.y;
  if (k >= p.K) return;                               // the tail block's spare waves; no barrier follows
  const int64_t pair = (int64_t)u * p.K + k;
  float* TR = p.trace ? p.trace + pair * p.Tm : nullptr;
  int* TS = p.trace ? p.tstart + pair * p.Tm : nullptr;
  const int L = p.label_len[k], n = min(p.tlen[u], p.Tm);
  const bool shape_ok = L >= 1 && L <= p.Lmax && n > 0;
  const int S = shape_ok ? 2 * L - 1 : 0;
  // ext_s: the keyword's pieces at even states, blanks between them
  int e = p.blank;
  bool bad = false, rep = false;
  if (lane < S && !(lane & 1)) {
    const int* lab = p.labels + (int64_t)k * p.Lmax;
    e = lab[lane >> 1];
    bad = e < 0 || e >= p.V || e == p.blank;
    rep = lane >= 2 && e == lab[(lane >> 1) - 1];
    if (bad) e = p.blank;
  }
  const bool any_bad = __ballot(bad) != 0;
  const int nrep = __popcll(__ballot(rep));
  if (!shape_ok || any_bad || n < L + nrep) {
    if (lane == 0) { p.score[pair] = NINF; p.start[pair] = -1; p.end[pair] = -1; }
    if (TR)
      for (int t = lane; t < p.Tm; t += 64) { TR[t] = NINF; TS[t] = -1; }
    return;
  }
  const bool last = lane == S - 1, first = lane == 0;
  // skip(s): a piece that differs from the piece before it (rep marks the equal ones)
  const bool skip = lane < S && lane >= 2 && !(lane & 1) && !rep;
  const float* LP = p.logp + (int64_t)u * p.Tm * p.ldp;
  const int* TOP = FILL ? p.top + (int64_t)u * p.Tm : nullptr;
  // Frames come in blocks of KW_PF, rows clamped to n - 1 (never a padding frame, and a load past
  // the last block is harmless): emis() gathers a block's emissions, every lane its own column;
  // the fillers of a block sit one per lane (lane j: frame t0 + j % KW_PF; read back by
  // v_readlane), and being two dependent loads they run two blocks deep: topi() of block i + 2
  // is issued with fill() of block i + 1, while block i is computed.
  const int j = lane & (KW_PF - 1);
  auto emis = [&](float* ev, int t0) {
#pragma unroll
    for (int q = 0; q < KW_PF; ++q) ev[q] = LP[(int64_t)min(t0 + q, n - 1) * p.ldp + e];
  };
  auto topi = [&](int t0) { return FILL ? TOP[min(t0 + j, n - 1)] : 0; };
  auto fill = [&](int tp, int t0) {
    return FILL ? LP[(int64_t)min(t0 + j, n - 1) * p.ldp + min(max(tp, 0), p.V - 1)] : 0.f;
  };
  float d = NINF, best = NINF;
  int st = -1, bt = -1, bs = -1;
  float ec[KW_PF], en[KW_PF];
  emis(ec, 0);
  float fc = fill(topi(0), 0);
  int tpn = topi(KW_PF);
  for (int t0 = 0; t0 < n; t0 += KW_PF) {
    emis(en, t0 + KW_PF);
    const float fn = fill(tpn, t0 + KW_PF);
    tpn = topi(t0 + 2 * KW_PF);
#pragma unroll
    for (int q = 0; q < KW_PF; ++q) {
      const int t = t0 + q;
      if (t < n) {                                    // wave-uniform
        const float d1 = shr1f(d, NINF), d2 = shr1f(d1, NINF);
        const int s1 = shr1i(st, -1), s2 = shr1i(s1, -1);
        float m = d;
        int b = st;
        if (d1 > m) { m = d1; b = s1; }
        if (skip && d2 > m) { m = d2; b = s2; }
        if (first && 0.f > m) { m = 0.f; b = t; }
        d = m + (ec[q] - lanef(fc, q));
        st = d == NINF ? -1 : b;
        if (d >= best) { best = d; bt = t; bs = st; }
        if (TR && last) { TR[t] = d; TS[t] = st; }
      }
    }
#pragma unroll
    for (int q = 0; q < KW_PF; ++q) ec[q] = en[q];
    fc = fn;
  }
  if (last) {
    const bool hit = best != NINF;
    p.score[pair] = best;
    p.start[pair] = hit ? bs : -1;
    p.end[pair] = hit ? bt + 1 : -1;
  }
  if (TR)
    for (int t = n + lane; t < p.Tm; t += 64) { TR[t] = NINF; TS[t] = -1; }
}

}  // namespace

extern "C" int avsr_ctc_kws(const avsr_ctc_kws_params* p, void* stream) {
  if (!p) return AVSR_E_ARG;
  if (p->U < 1 || p->K < 1 || p->Tm < 1 || p->Lmax < 1 || p->Lmax > 32 || p->U > 65535) return AVSR_E_SHAPE;
  if (p->V < 1 || p->ldp < p->V || p->blank < 0 || p->blank >= p->V) return AVSR_E_ARG;
  if (!p->logp || !p->tlen || !p->labels || !p->label_len || !p->score || !p->start || !p->end) return AVSR_E_ARG;
  if ((p->trace == nullptr) != (p->tstart == nullptr)) return AVSR_E_ARG;
  const dim3 grid((unsigned)((p->K + 3) / 4), p->U);
  if (p->top) hipLaunchKernelGGL(ctc_kws_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, *p);
  else hipLaunchKernelGGL(ctc_kws_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, *p);
  AVSR_CHECK_LAUNCH();
  return 0;
}
