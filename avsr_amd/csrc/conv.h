// What the translation units of the implicit-GEMM convolution (conv.hip and conv_*.hip) share: the kernel
// argument block, the plan conv.hip's conv_plan fills once per call, the constants and the one loader that
// more than one file uses (each naming its users), and the per-family launchers conv.hip dispatches to.
#pragma once
#include "gemm_core.h"
#include "gemm_glds.h"

namespace conv {
using namespace gemmcore;
using gemmg::GBK;
using gemmg::OOB;
using gemmg::bglds16;
using gemmg::make_rsrc;

struct ConvArgs {
  ConvGeom g;
  uint32_t a_bytes, b_bytes;      // per-group operand extents for the buffer-DMA loaders (0: pointer loaders)
  const void* a; const void* b;   // operand bases (group 0)
  int64_t a_gstride, b_gstride, c_gstride;
  int M, N, K, splits, kchunk;
  float* ws;                      // bwd_weight split-K slabs [groups][splits][M][N] (nullptr: direct / atomics)
  Epi e;
  gemmg::BnrArgs bnr;             // K_DGRAD_BNR: BatchNorm-backward reduction of the stored tile
};

// K_DGRAD_BNR + r: data-grad whose epilogue is gemmg::epilogue_bnr with residual mode r
// (0 none, 1 identity, 2 under its own BN); bf16 LDS-DMA and patch kernels only
enum { K_FWD = 0, K_DGRAD = 1, K_WGRAD = 2, K_DGRAD_BNR = 3 };

// weight-gradient split-K (conv.hip wgrad_plan): K = pixels in `splits` chunks of `kchunk`; slab:
// per-split fp32 slabs in the workspace and an ordered reduce, else direct (one split) / fp32 atomics
struct WgradPlan { int splits, kchunk; bool slab; };
// What conv.hip's conv_plan decides about a call; the launches and the size queries only read it.
struct ConvPlan {
  int path, bm, tiles;          // AVSR_CONV_PATH_*; row-tile height (256 / 192 / 128 / 64); fwd / dgrad: row tiles
  int cls_bm[4], cls_tiles[4];  // PATH_S2: per parity class (tiles = their sum; an empty class has 0)
  uint32_t a_bytes, b_bytes;    // ConvArgs' operand extents
  WgradPlan w;                  // weight-grad through the general kernels
  int64_t ws_floats;            // weight-grad: the workspace it uses when the caller passes one
};

// patch-resident 3x3 tile (conv.hip: the PATCH_ROWS span rule and the row tiles of the plan;
// conv_patch.hip: the kernel)
constexpr int PATCH_ROWS = 384;                        // padded pixels of 64 channels (128 B) per block
using PCfg = gemmg::GCfg<4, 1, 2, 2, 3>;               // 256 x 64, 4 waves of 64 x 64, 3-stage weight ring
// persistent blocks and slab columns of the patch-resident weight-grads (conv.hip: workspace sizes;
// conv_wpatch.hip: the kernels). Stages 1-4: 128 blocks, one on every other CU. These run on the
// side stream beside the ResNet backward's data-gradient chain, and a block holds up to 152 KB of
// LDS, so at one block per CU (256) every chain kernel needing LDS waited for free CUs; 128 blocks
// take longer on the side but the step is shorter (6 of 6 interleaved pairs, +0.3-0.5 %
// value_expected; 64: slower; profiles/r05_wpatch_blocks_ab.txt). Stem: one block per CU.
constexpr int WP_BLOCKS = 128, WP_COLS = 576, SWP_BLOCKS = 256, SWP_COLS = 392;

// data-grad B: weight [cout][kh][kw][cin] as (r = cin, k = (kh, kw, cout)), r-contiguous, by buffer
// DMA (conv_igemm.hip conv_glds_kernel, conv_patch.hip conv_patch_kernel)
template <int R, int NW> struct BWgtR {
  static constexpr bool KMAJ = false;
  static constexpr int CPR = R / 8, RPP = 64 / CPR, SLOTS = GBK / RPP / NW;
  __amdgpu_buffer_rsrc_t rs; ConvGeom g;
  uint32_t vo[SLOTS];
  AVSR_DEV void init(const bf16* base, uint32_t bytes, const ConvGeom& g_, int r0, int rext, int wave, int lane) {
    rs = make_rsrc(base, bytes); g = g_;
    const int ktot = g.ktot_w;
#pragma unroll
    for (int i = 0; i < SLOTS; ++i) {
      const int pc = i * NW + wave, pk = pc * RPP + lane / CPR;
      const int r = r0 + ((lane % CPR) ^ gemmg::rswz<CPR>(pk)) * 8;
      vo[i] = r < rext ? (uint32_t)(((int64_t)pk * ktot + r) * 2) : OOB;
    }
  }
  AVSR_DEV void issue(char* img, int k0, int wave) const {
    const int ktot = g.ktot_w;
    int tap = k0 >> g.cout_shift;
    if (g.tap_step != 1) {      // parity class of a stride-2 data-grad: class tap (u, v) -> kernel tap
      const int u = (int)fdiv(tap, g.f_kw), v = tap - u * (int)g.f_kw.d;
      tap = (g.tap_kh0 + g.tap_step * u) * g.tap_kfw + g.tap_kw0 + g.tap_step * v;
    }
    const uint32_t so = (uint32_t)((((int64_t)(k0 & ((1 << g.cout_shift) - 1))) * ktot + (int64_t)tap * g.cin) * 2);
#pragma unroll
    for (int i = 0; i < SLOTS; ++i) bglds16(rs, vo[i], so, img + (i * NW + wave) * 1024);
  }
};

// The launchers conv.hip dispatches to, each beside its kernels (kind: K_*; bm: the plan's row-tile
// height); they return 0, a HIP launch error or an AVSR_E_* code
int igemm_f32(int kind, int bm, const ConvArgs& a, int groups, hipStream_t st);    // conv_igemm.hip, register-staged
int igemm_glds(int kind, int bm, const ConvArgs& a, int groups, hipStream_t st);   // conv_igemm.hip, LDS-DMA (bf16)
int patch_launch(int kind, const ConvArgs& a, const avsr_conv_params* p, hipStream_t st);   // conv_patch.hip
int wpatch_launch(const avsr_conv_params* p, hipStream_t st);                      // conv_wpatch.hip, stages 1-4
int stem_wpatch_launch(const avsr_conv_params* p, hipStream_t st);                 // conv_wpatch.hip
// conv.hip: dw[g] += the slabs ws[g][s][mn] in split order, in `chunks` chunks first (users: the general
// weight-grad, conv_wpatch.hip's stem weight-grad)
int wgrad_reduce(float* ws, int splits, int chunks, int64_t mn, int groups, float* dw, int64_t dw_gstride, hipStream_t st);
}  // namespace conv
