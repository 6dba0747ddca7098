// What the translation units of avsr_gemm (gemm.hip, gemm_wgrad.hip, gemm_skinny.hip) share: the
// kernel argument block, the per-tile epilogue arguments, the host entry points that cross files.
#pragma once
#include "gemm_core.h"
#include "gemm_glds.h"

namespace gemmd {
using namespace gemmcore;

struct DenseArgs {
  int M, N, K, splits, kchunk;
  uint32_t a_bytes, b_bytes;   // buffer extents of one batch's A / B (buffer-DMA loaders); 0 = pointer loaders
  int64_t sSplit;      // slab mode: C offset between K splits (0: atomics / no split)
  const void* A; int64_t lda, sA;
  const void* B; int64_t ldb, sB;
  int64_t sC, sR;
  Epi e;
  unsigned long long* stamp;   // diagnostic {min start, max end} (avsr_gemm_params.stamp) or null
  unsigned* cnt;               // wgrad_dual_kernel slab mode: per-tile arrival counters (zeroed) or null
  float* fC; int64_t fldc;     // ... its final output C (the slabs' reduction target)
  float falpha, fbeta;
  const float* ln_c1; float ln_eps;   // skinny_mma_kernel LayerNorm prologue (avsr_gemm_params.ln_c1)
  float* lnst;                        // ... its per-chunk row statistics (split launches)
  float* kvk; float* kvv; const int* kvpos; int kvrows; int kvposs;   // KV-cache append (avsr_gemm_params.kv_k)
};

// the epilogue arguments of one output tile's batch / K split, pinned to the variant EV
// (T: storage of res / preact / gate)
template <typename T, typename OutT, int EV>
AVSR_DEV Epi tile_epi(const DenseArgs& a, int bz, int sp) {
  Epi e = a.e;
  epi_fold<EV>(e);
  e.C = (OutT*)e.C + (int64_t)bz * a.sC + sp * a.sSplit;
  if (e.res) e.res = (const T*)e.res + (int64_t)bz * a.sR;
  if (e.preact) e.preact = (T*)e.preact + (int64_t)bz * a.sC;
  if (e.gate) e.gate = (const T*)e.gate + (int64_t)bz * a.sC;
  e.drop_base = (uint64_t)bz * (uint64_t)a.M * (uint64_t)a.N;
  return e;
}

// gemm.hip: the LDS-DMA path takes this call (bf16, whole 16-byte vectors along every operand's
// contiguous dimension); the argument block of a checked call (slab: split partials go to p->ws)
bool glds_ok(const avsr_gemm_params* p);
DenseArgs dense_args(const avsr_gemm_params* p, int splits, bool slab);

// gemm_wgrad.hip: the weight-gradient shape; its launch (*reduced: the last split of every tile
// summed the slabs in the kernel, no reduction pass is due)
bool wgrad_dual_ok(const avsr_gemm_params* p, int splits, bool slab);
int wgrad_dual_launch(const avsr_gemm_params* p, const DenseArgs& a, hipStream_t st, bool* reduced);

// gemm_skinny.hip: forward linears with few rows
bool skinny_ok(const avsr_gemm_params* p, int splits);
int skinny_launch(const avsr_gemm_params* p, const DenseArgs& a, hipStream_t st);

}  // namespace gemmd
