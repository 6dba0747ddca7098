// What two or more of the beam-search translation units share (decode_softmax.hip, ctc_prefix.hip,
// beam.hip; dec_attn.hip needs none of it): the CTC log-zero, the width of the per-thread top-k
// lists, and the (value, index) arg-max over a wave and a 256-thread block.
#pragma once
#include "common.h"

namespace {

constexpr float LOGZERO = -10000000000.0f;   // CTCPrefixScoreTH.logzero (ctc_prefix_score.py:29)

// top-k width of row_topk / log_softmax_topk (K) and of beam_select (beam): per-thread sorted lists
constexpr int KMAX = 16;

// Cross-lane reductions on DPP row rotations (common.h): the __shfl_xor butterflies they replace
// are ds_bpermute round trips through the LDS unit (~2 us per block arg-max: the pre-beam's 7
// rounds took 12 us of an 18 us kernel).
// (value, index) arg-max over the wave, ties -> smaller index (a total order: exact, uniform)
AVSR_DEV void dwave_argmax(float& v, int& i) {
#define DA_STEP(R_) { const float ov = rorf<R_>(v); const int oi = rori<R_>(i); \
                      if (ov > v || (ov == v && oi < i)) { v = ov; i = oi; } }
  DA_STEP(8) DA_STEP(4) DA_STEP(2) DA_STEP(1)
#undef DA_STEP
  float bv = lanef(v, 0); int bi = __builtin_amdgcn_readlane(i, 0);
#pragma unroll
  for (int r = 1; r < 4; ++r) {
    const float ov = lanef(v, 16 * r); const int oi = __builtin_amdgcn_readlane(i, 16 * r);
    if (ov > bv || (ov == bv && oi < bi)) { bv = ov; bi = oi; }
  }
  v = bv; i = bi;
}

// (value, index) arg-max across the 256-thread block; ties -> smaller index
AVSR_DEV void block_argmax256(float& v, int& i, float* shv, int* shi) {
  dwave_argmax(v, i);
  if ((threadIdx.x & 63) == 0) { shv[threadIdx.x >> 6] = v; shi[threadIdx.x >> 6] = i; }
  __syncthreads();
  v = shv[0]; i = shi[0];
#pragma unroll
  for (int w = 1; w < 4; ++w)
    if (shv[w] > v || (shv[w] == v && shi[w] < i)) { v = shv[w]; i = shi[w]; }
  __syncthreads();
}

}  // namespace
