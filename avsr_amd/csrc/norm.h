// What the BatchNorm (batchnorm.hip) and pooling (pool.hip) kernels share: both walk NHWC
// tensors in 16-byte channel vectors with a grid stride that keeps a thread on one channel group.
#pragma once
#include "common.h"

// Per-channel parameters of the thread's fixed channel group (the grid stride is a multiple
// of C/VE, so every vector a thread visits has the same channels): loaded once.
template <int VE>
AVSR_DEV void chan_load(const float* p, int c0, float (&o)[VE]) {
#pragma unroll
  for (int j = 0; j < VE; ++j) o[j] = p ? p[c0 + j] : 0.f;
}

// grid of 256-thread blocks over nv channel vectors, at most 2048 blocks (the kernels grid-stride)
static inline int bn_grid(int64_t nv) { return avsr_grid(nv, 256, 2048); }
