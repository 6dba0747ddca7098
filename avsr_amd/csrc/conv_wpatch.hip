// Implicit-GEMM convolution, the patch-resident weight-gradients: ResNet stages 1-4
// (AVSR_CONV_PATH_WPATCH: conv_wgrad_patch_kernel + wpatch_reduce_kernel) and the stem
// (AVSR_CONV_PATH_STEM_WPATCH: stem_wgrad_patch_kernel, reduced by conv.hip's wgrad_reduce).
#include "conv.h"

namespace conv {
namespace {

// ---------------------------------------------------------------- patch-resident weight-grad
// dW[co][(kh, kw, ci)] = sum_p dy[p][co] * x[p + (kh-1, kw-1)][ci] for the 3x3 / stride 1 /
// pad 1 convolutions of ResNet stages 1 (22 x 22 x 64) and 2 (11 x 11 x 128). The general
// weight-grad re-gathers x for every tap (9 passes of the input through L2; at stage 1 its
// 64 x 256 tiles are 1/4 padding). Here persistent blocks (WP_BLOCKS, conv.h) walk tiles of TR whole
// image rows; a block owns a 64 x 64 (co, ci) block of every tap. Per tile the block's dy
// channels and the zero-padded (TR+2) x (W+2) patch of its x channels are DMA'd into LDS once,
// double buffered, and all 9 taps read the patch at row offsets. Every tile has the same
// geometry, so each LDS address of the main loop is a per-lane base fixed for the kernel plus a
// compile-time offset. The 64 x 576 gradient block stays in registers: wave w owns input
// channels [16w, 16w + 16) of all 9 taps (36 accumulators of 16 x 16). Both operands are
// pixel-major, so both fragments are transposed LDS reads (ds_read_b64_tr_b16); the MFMA k
// order within a fragment is permuted (k bits 2 and 3 swapped) so that each half-wave read
// covers 8 consecutive pixels: the dy image (128-byte rows) is conflict-free with a chunk XOR
// on pixel bits 1-2, the patch (padded rows, no XOR) is (nearly) conflict-free. The
// DMAs of the next tile are spread over the k-steps. With several (co, ci) blocks (stage 2:
// 2 x 2), the blocks that share an XCD (ids b, b+8, ...) take the blocks of the same tile range,
// so x and dy come from that XCD's L2 after the first read. Each block writes its fp32 partial
// once to a slab [block][64][576]; wpatch_reduce_kernel sums them in block order (deterministic).
//
// Stages 3 (6 x 6, 256 channels) and 4 (3 x 3, 512 channels): a tile is IPT whole images stacked
// vertically in the patch with ONE shared zero row between neighbours (a tap above an image's
// first row or below its last reads that row), so the 9 taps stay row offsets; IPT is chosen so
// that IPT x H x W pixels nearly fill whole 32-pixel k-steps (180 of 192, 126 of 128). NBLK
// persistent blocks; the next tile's DMAs are issued over the first SPREAD k-steps of the current
// one (with few k-steps per tile, DMAs issued at the last one would have no time to land).
template <int W_, int TR_, int TPI_, int NBUF_, int PST_, int IPT_ = 1, int NBLK_ = WP_BLOCKS, int SPREAD_ = 0>
struct WPGeo {
  static constexpr int W = W_, TR = TR_, TPI = TPI_, H = TR * TPI, NBUF = NBUF_, PST = PST_, IPT = IPT_, NBLK = NBLK_;
  static constexpr int IMGT = TR * W;                // pixels of one image in a tile
  static constexpr int PX = IPT * IMGT;              // pixels per tile
  static constexpr int KS = (PX + 31) / 32;          // k-steps of 32 pixels
  static constexpr int DYR = KS * 32;                // dy image rows (>= PX: zero)
  static constexpr int WP = W + 2, PROWS = (IPT * (TR + 1) + 1) * WP;
  static constexpr int SLOTS = PST / 16;             // 16-byte slots per patch row (8 data + pad)
  static constexpr int PPIECE = (PROWS * SLOTS + 255) / 256;   // patch DMA pieces per wave
  static constexpr int PBYTES = PPIECE * 4 * 1024;
  static constexpr int DYPIECE = DYR * 128 / 4096;   // dy DMA pieces per wave
  static constexpr int DYB = DYR * 128;
  static constexpr int BUF = DYB + PBYTES;
  static constexpr int LDS = NBUF * BUF;
  static constexpr int NP = DYPIECE + PPIECE;        // DMAs per wave per tile
  static constexpr int SPREAD = SPREAD_ > 0 ? SPREAD_ : KS;
  static_assert(LDS <= 160 * 1024, "the tile buffers must fit the CU's LDS");
  static_assert(IPT == 1 || TPI == 1, "a tile is part of one image or whole images");
  static_assert(NBUF >= 2 && (NBUF - 2) * NP <= 63 && SPREAD <= KS, "vmcnt range / DMA spread");
  static_assert(NBLK % 8 == 0, "blocks come in XCD groups of 8");
};
// patch row stride 144 B: one 2-way overlap among 8 consecutive rows' 32-byte windows; 160 B:
// none (what the LDS allows)
using WPStage1 = WPGeo<22, 11, 2, 2, 144>;   // half images: 242 pixels, 13 x 24 patch, double buffered
using WPStage2 = WPGeo<11, 11, 1, 3, 160>;   // whole images: 121 pixels, 13 x 13 patch, 3 buffers (short tiles)
using WPStage3 = WPGeo<6, 6, 1, 2, 144, 5, WP_BLOCKS, 3>;    // 5 images: 180 pixels, 36 x 8 patch
using WPStage4 = WPGeo<3, 3, 1, 2, 160, 14, WP_BLOCKS, 2>;   // 14 images: 126 pixels, 57 x 5 patch

AVSR_DEV int whswz(int row) { return ((row >> 1) & 3) << 1; }
AVSR_DEV bf16x8 trpair(const char* pa, const char* pb) {
  const v4i16 a = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_v4i16*)pa);
  const v4i16 b = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_v4i16*)pb);
  union { v4i16 s4[2]; bf16x8 h; } u;
  u.s4[0] = a; u.s4[1] = b;
  return u.h;
}

// (co, ci) block q and tile range r of block b among nblk: blocks b, b+8, ... share an XCD under
// round-robin placement (S = nblk / 8 per XCD). nq <= S (S % nq == 0): the nq blocks with the same
// range sit on one XCD; nq > S (nq % S == 0): a range's blocks fill nq / S XCDs. Ranges per
// block kind: bpq = nblk / nq either way.
AVSR_DEV void wp_block(int b, int nq, int nblk, int& q, int& r) {
  const int x = b & 7, s = b >> 3, S = nblk >> 3;
  if (nq <= S) {
    q = s % nq;
    r = (s / nq) * 8 + x;
  } else {
    const int k = nq / S;
    r = x / k;
    q = (x - r * k) * S + s;
  }
}

// wait until at most min(ahead, K) tiles of NP DMAs each are still in flight (vmcnt is an immediate)
template <int NP, int K>
AVSR_DEV void wp_wait_ahead(int ahead) {
  if constexpr (K == 0) {
    gemmg::wait_vmcnt<0>();
  } else {
    if (ahead >= K) gemmg::wait_vmcnt<NP * K>();
    else wp_wait_ahead<NP, K - 1>(ahead);
  }
}

template <class G>
__global__ __launch_bounds__(256, 1) void conv_wgrad_patch_kernel(const bf16* __restrict__ x, const bf16* __restrict__ dy,
                                                                  uint32_t x_bytes, uint32_t dy_bytes, int nimg,
                                                                  int cin, int cout, float* __restrict__ ws) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  constexpr int IMG = G::H * G::W;
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int ncih = cin / 64, nq = (cout / 64) * ncih, bpq = gridDim.x / nq;
  int q, rng;
  wp_block(blockIdx.x, nq, gridDim.x, q, rng);
  const int coh = q / ncih, cih = q - coh * ncih;
  const int ntiles = (nimg * G::TPI + G::IPT - 1) / G::IPT;   // a last part tile reads zeros past the end
  const int ta = (int)((int64_t)ntiles * rng / bpq), tb = (int)((int64_t)ntiles * (rng + 1) / bpq);
  const __amdgpu_buffer_rsrc_t rx = make_rsrc(x, x_bytes), rdy = make_rsrc(dy, dy_bytes);
  // DMA pieces of a tile (offsets recomputed per issue: compile-time divisors, no registers held)
  auto tile_px = [&](int t) { return (t / G::TPI) * IMG * G::IPT + (t % G::TPI) * G::PX; };
  auto issue_dy = [&](int i, int t, char* buf) {
    const int s = (wave + 4 * i) * 64 + lane, row = s >> 3;
    const int c = (s & 7) ^ whswz(row);
    const uint32_t vo = row < G::PX ? (uint32_t)(tile_px(t) + row) * (uint32_t)(cout * 2) + coh * 128 + c * 16 : gemmg::OOB;
    gemmg::bglds16(rdy, vo, 0u, buf + (wave + 4 * i) * 1024);
  };
  auto issue_patch = [&](int i, int t, char* buf) {
    const int s = (wave + 4 * i) * 64 + lane, row = s / G::SLOTS, ch = s - row * G::SLOTS;
    const int py = row / G::WP, pxp = row - py * G::WP;
    bool ok;
    int src;                                           // input pixel of this slot (relative to the tile's first)
    if constexpr (G::IPT == 1) {
      const int y = (t % G::TPI) * G::TR + py - 1;     // image row of this slot's patch row
      ok = y >= 0 && y < G::H;
      src = (py - 1) * G::W + pxp - 1;
    } else {                                           // image i's rows 1 + i (H + 1) ..., shared zero rows between
      const int i = (py - 1) / (G::TR + 1), yl = py - 1 - i * (G::TR + 1);
      ok = py >= 1 && yl < G::TR;
      src = i * G::IMGT + yl * G::W + pxp - 1;
    }
    ok = ok && ch < 8 && row < G::PROWS && pxp >= 1 && pxp <= G::W;
    const uint32_t vo = ok ? (uint32_t)(tile_px(t) + src) * (uint32_t)(cin * 2) + cih * 128 + ch * 16 : gemmg::OOB;
    gemmg::bglds16(rx, vo, 0u, buf + G::DYB + (wave + 4 * i) * 1024);
  };
  // fragment bases: lane group g holds k = 8g + j <-> pixel 32kb + 16(g >> 1) + 4(g & 1) + (j & 3) + 8(j >> 2)
  const int g = lane >> 4, qq = (lane & 15) >> 2, pp = lane & 3;
  const int pxa = 16 * (g >> 1) + 4 * (g & 1) + qq;
  const int sw = whswz(pxa);
  int dA[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) dA[i] = pxa * 128 + (((2 * i + (pp >> 1)) ^ sw) << 4) + 8 * (pp & 1);
  auto prow = [&](int px) {                        // tile pixel -> patch row
    px = min(px, G::PX - 1);
    const int i = px / G::IMGT, r = px - i * G::IMGT, yy = r / G::W, xx = r - yy * G::W;
    return (i * (G::TR + 1) + yy + 1) * G::WP + xx + 1;
  };
  int pA[G::KS], pB[G::KS];               // patch byte bases (tap (0, 0) = offset 0) per k-step
#pragma unroll
  for (int kb = 0; kb < G::KS; ++kb) {
    pA[kb] = (prow(32 * kb + pxa) - G::WP - 1) * G::PST + 32 * wave + 8 * pp;
    pB[kb] = (prow(32 * kb + pxa + 8) - G::WP - 1) * G::PST + 32 * wave + 8 * pp;
  }
  f32x4 acc[4][9];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int t = 0; t < 9; ++t) acc[i][t] = f32x4{0.f, 0.f, 0.f, 0.f};
  constexpr int PD = G::NBUF - 1;          // tiles in flight ahead of the one computed
#pragma unroll
  for (int d = 0; d < PD; ++d)
    if (ta + d < tb) {
#pragma unroll
      for (int i = 0; i < G::DYPIECE; ++i) issue_dy(i, ta + d, smem + d * G::BUF);
#pragma unroll
      for (int i = 0; i < G::PPIECE; ++i) issue_patch(i, ta + d, smem + d * G::BUF);
    }
  constexpr int PER = (G::NP + G::SPREAD - 1) / G::SPREAD;   // DMAs per k-step
  for (int t = ta; t < tb; ++t) {
    const char* buf = smem + ((t - ta) % G::NBUF) * G::BUF;
    char* nbuf = smem + ((t + PD - ta) % G::NBUF) * G::BUF;
    const bool more = t + PD < tb;
    // tile t has landed: the DMAs of the (up to PD - 1) later tiles already issued may still fly
    wp_wait_ahead<G::NP, PD - 1>(tb - 1 - t);
    __builtin_amdgcn_s_barrier();         // ... for every wave; every wave is done with tile t-1
    asm volatile("" ::: "memory");
    const char* patch = buf + G::DYB;
    // fragments of k-step kb: 4 dy (A) and 9 tap (B) transposed reads; the reads of step kb+1
    // are issued before the MFMAs of step kb (one wave per SIMD: nothing else hides their
    // latency), the next tile's DMAs after them (the asm DMA is a compiler memory barrier)
    struct Fr { bf16x8 a[4], b[9]; };
    auto load = [&](Fr& f, int kb) {
#pragma unroll
      for (int i = 0; i < 4; ++i) f.a[i] = trpair(buf + dA[i] + kb * 4096, buf + dA[i] + kb * 4096 + 1024);
#pragma unroll
      for (int tp = 0; tp < 9; ++tp) {
        const int off = ((tp / 3) * G::WP + tp % 3) * G::PST;
        f.b[tp] = trpair(patch + pA[kb] + off, patch + pB[kb] + off);
      }
    };
    Fr cur, nxt;
    load(cur, 0);
#pragma unroll
    for (int kb = 0; kb < G::KS; ++kb) {
      if (kb + 1 < G::KS) load(nxt, kb + 1);
      if (more && kb < G::SPREAD) {
#pragma unroll
        for (int d = 0; d < PER; ++d) {
          const int pc = kb * PER + d;
          if (pc < G::DYPIECE) issue_dy(pc, t + PD, nbuf);
          else if (pc < G::DYPIECE + G::PPIECE) issue_patch(pc - G::DYPIECE, t + PD, nbuf);
        }
      }
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int tp = 0; tp < 9; ++tp) acc[i][tp] = mfma16(cur.a[i], cur.b[tp], acc[i][tp]);
      if (kb + 1 < G::KS) cur = nxt;
    }
  }
  // partial -> ws[block][co 64][576]: accumulator (i, tap) register r = co 16i + 4g + r, column
  // tap * 64 + 16 * wave + (lane & 15)
  float* o = ws + (int64_t)blockIdx.x * 64 * WP_COLS;
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int tp = 0; tp < 9; ++tp)
#pragma unroll
      for (int r = 0; r < 4; ++r) o[(16 * i + 4 * g + r) * WP_COLS + tp * 64 + 16 * wave + (lane & 15)] = acc[i][tp][r];
}

AVSR_DEV int wp_bid(int q, int r, int nq, int nblk) {   // inverse of wp_block
  const int S = nblk >> 3;
  if (nq <= S) return ((((r >> 3) * nq) + q) << 3) + (r & 7);
  const int k = nq / S;
  return ((q % S) << 3) + r * k + q / S;
}

// dw[co][tap][ci] += sum over the tile ranges r of block kind q of ws[wp_bid(q, r)][co % 64][tap * 64 + ci % 64],
// in range order (deterministic), in two passes: chunk c of WPR_CHUNKS folds its ranges into the
// slab of its first range (in place); pass 2 (chunk < 0) adds the chunk heads in order to dw.
// 4 consecutive ci per thread.
constexpr int WPR_CHUNKS = 8;
__global__ __launch_bounds__(256) void wpatch_reduce_kernel(float* __restrict__ ws, int nblk, int cin, int cout,
                                                            float* dw, int pass2) {
  const int ncih = cin / 64, nq = (cout / 64) * ncih, bpq = nblk / nq;
  const int e = (blockIdx.x * 256 + threadIdx.x) * 4;      // element of the 64 x 576 block
  const int q = blockIdx.y, c = blockIdx.z;
  if (e >= 64 * WP_COLS) return;
  f32x4 s = {0.f, 0.f, 0.f, 0.f};
  if (!pass2) {
    const int r0 = bpq * c / WPR_CHUNKS, r1 = bpq * (c + 1) / WPR_CHUNKS;
    for (int r = r0; r < r1; ++r) s += *(const f32x4*)(ws + (int64_t)wp_bid(q, r, nq, nblk) * 64 * WP_COLS + e);
    if (r1 > r0) *(f32x4*)(ws + (int64_t)wp_bid(q, r0, nq, nblk) * 64 * WP_COLS + e) = s;
    return;
  }
  for (int k = 0; k < WPR_CHUNKS; ++k) {
    const int r0 = bpq * k / WPR_CHUNKS, r1 = bpq * (k + 1) / WPR_CHUNKS;
    if (r1 > r0) s += *(const f32x4*)(ws + (int64_t)wp_bid(q, r0, nq, nblk) * 64 * WP_COLS + e);
  }
  const int r = e / WP_COLS, col = e - r * WP_COLS, tap = col >> 6, ci = col & 63;
  const int coh = q / ncih, cih = q - coh * ncih;
  float* d = dw + ((int64_t)(coh * 64 + r) * 9 + tap) * cin + cih * 64 + ci;
#pragma unroll
  for (int k = 0; k < 4; ++k) d[k] += s[k];     // dw is a view into the parameter arena: 4-byte aligned only
}

template <class G>
int wpatch_launch_g(const avsr_conv_params* p, hipStream_t st) {
  static bool attr = false;
  if (!attr) {
    (void)hipFuncSetAttribute((const void*)conv_wgrad_patch_kernel<G>, hipFuncAttributeMaxDynamicSharedMemorySize, G::LDS);
    attr = true;
  }
  const uint32_t bytes = (uint32_t)((int64_t)p->nimg * p->hin * p->win * p->cin * 2);
  const int nq = (p->cout / 64) * (p->cin / 64), S = G::NBLK / 8;
  if (nq <= S ? S % nq != 0 : (nq % S != 0 || 8 % (nq / S) != 0)) return AVSR_E_SHAPE;   // wp_block's mapping
  hipLaunchKernelGGL((conv_wgrad_patch_kernel<G>), dim3(G::NBLK), dim3(256), G::LDS, st, (const bf16*)p->x,
                     (const bf16*)p->dy, bytes, bytes, p->nimg, p->cin, p->cout, p->ws);
  AVSR_CHECK_LAUNCH();
  const unsigned gx = (64 * WP_COLS / 4 + 255) / 256;
  hipLaunchKernelGGL(wpatch_reduce_kernel, dim3(gx, (unsigned)nq, (unsigned)WPR_CHUNKS), dim3(256), 0, st, p->ws,
                     G::NBLK, p->cin, p->cout, p->dw, 0);
  AVSR_CHECK_LAUNCH();
  hipLaunchKernelGGL(wpatch_reduce_kernel, dim3(gx, (unsigned)nq, 1u), dim3(256), 0, st, p->ws, G::NBLK, p->cin,
                     p->cout, p->dw, 1);
  AVSR_CHECK_LAUNCH();
  return 0;
}

// ---------------------------------------------------------------- patch-resident stem weight-grad
// The stem conv's weight-gradient (Conv3d 1 -> 64, 5 x 7 x 7, stride (1, 2, 2), pad (2, 3, 3)) on
// the packed input xp [N][88][88][8] (the 5 frames t-2 .. t+2 of each pixel in channels 0-4,
// zeros after; ops.stem_pack): gp[co][kh][kw][c] += sum_p dy[p][co] * xp[p's image][2oy+kh-3]
// [2ox+kw-3][c] over the N x 44 x 44 output pixels. The general implicit GEMM computes an im2col
// address per 16-byte DMA slot and amortises its 256-column tiles over only 64 output channels
// (VALU-bound, MFMA busy 0.28: profiles/r05_stem_wgrad_counters.txt). Here persistent blocks
// (one per CU) walk tiles of 4 output rows of one image, 48 columns wide (44 real; the other dy
// rows are DMA zeros). Per tile the dy rows and the zero-padded 13 x 103 input patch (16 bytes
// per pixel) are DMA'd into LDS once, three buffers deep, and every tap of every pixel is an
// offset into the patch. A k-step's 32 pixels are a 4-row x 8-column block (dy rows stored in
// that order), so every LDS address of the main loop is a per-lane base fixed for the kernel plus
// a compile-time offset (no address arithmetic per k-step), and the DMA offsets are per-lane
// constants plus a per-tile scalar. The 64 x 392 gradient block stays in registers: columns are
// pairs of taps (t, t+1) x 8 channels (16 per MFMA tile; 25 pairs, the 49th tap's partner a
// discarded duplicate), pair P belongs to wave P mod 4, and waves 1-3 run a discarded 7th pair
// so that every wave has the same branch-free loop. The fragment reads of k-step kb+1 are issued
// between the two halves of k-step kb's MFMAs (scheduling barriers keep them there): the LDS
// latency hides behind the second half instead of an lgkmcnt drain in front of every k-step
// (lgkmcnt counts to 15; a step has 22 reads). Both operands are pixel-major, read
// transposed (ds_read_b64_tr_b16) with wgrad_patch's pixel order; a 16-lane group's patch read
// covers 4 pixels x 2 taps x 8 channels in 128 contiguous bytes modulo the banks (row stride
// 103 x 16 B keeps the pairs that straddle two kernel rows conflict-free too). Each block writes
// its fp32 partial to a slab [block][64][392]; wgrad_reduce_kernel sums the slabs in block order
// (deterministic).
constexpr int SWP_TR = 4, SWP_TC = 48, SWP_KS = SWP_TC / 8, SWP_TPI = 44 / SWP_TR;
constexpr int SWP_DYB = SWP_KS * 32 * 128, SWP_DYPIECE = SWP_DYB / 4096;
constexpr int SWP_PR = 2 * SWP_TR + 5, SWP_PC = 103, SWP_SLOTS = SWP_PR * SWP_PC, SWP_RB = SWP_PC * 16;
constexpr int SWP_PPIECE = (SWP_SLOTS + 255) / 256, SWP_PBYTES = SWP_PPIECE * 4096;
constexpr int SWP_BUF = SWP_DYB + SWP_PBYTES, SWP_NBUF = 3, SWP_LDS = SWP_NBUF * SWP_BUF;
constexpr int SWP_NP = SWP_DYPIECE + SWP_PPIECE, SWP_PAIRS = 25;
constexpr int SWP_JW = (SWP_PAIRS + 3) / 4;     // pairs per wave (7; pairs >= 25 are discarded)
static_assert(SWP_LDS <= 160 * 1024 && SWP_DYB % 4096 == 0 && SWP_KS % 2 == 0, "stem weight-grad tile buffers");
static_assert(2 * (SWP_TC - 1) + 6 - 3 < SWP_PC - 3 + 1 && SWP_NP % SWP_KS == 0, "patch width / DMA spread");

AVSR_DEV int swp_toff(int t) {                 // patch byte offset of tap t = (kh, kw) (t > 48 -> 48)
  t = t > 48 ? 48 : t;
  const int kh = t / 7, kw = t - 7 * kh;
  return kh * SWP_RB + kw * 16;
}

__global__ __launch_bounds__(256, 1) void stem_wgrad_patch_kernel(const bf16* __restrict__ xp, const bf16* __restrict__ dy,
                                                                  uint32_t x_bytes, uint32_t dy_bytes, int nimg,
                                                                  float* __restrict__ ws) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int ntiles = nimg * SWP_TPI;
  const int ta = (int)((int64_t)ntiles * blockIdx.x / gridDim.x), tb = (int)((int64_t)ntiles * (blockIdx.x + 1) / gridDim.x);
  const __amdgpu_buffer_rsrc_t rx = make_rsrc(xp, x_bytes), rdy = make_rsrc(dy, dy_bytes);
  // per-lane DMA offsets relative to the tile's first dy pixel / input pixel (OOB: zeros)
  uint32_t vdy[SWP_DYPIECE];
  int vpt[SWP_PPIECE], ppr[SWP_PPIECE];
#pragma unroll
  for (int i = 0; i < SWP_DYPIECE; ++i) {
    const int sl = (wave + 4 * i) * 64 + lane, row = sl >> 3;          // dy LDS row = kb * 32 + r * 8 + c
    const int ch = (sl & 7) ^ whswz(row), k = row & 31, col = 8 * (row >> 5) + (k & 7);
    vdy[i] = col < 44 ? (uint32_t)(((k >> 3) * 44 + col) * 128 + ch * 16) : gemmg::OOB;
  }
#pragma unroll
  for (int i = 0; i < SWP_PPIECE; ++i) {
    const int sl = (wave + 4 * i) * 64 + lane, pr = sl / SWP_PC, pc = sl - pr * SWP_PC;
    const bool ok = sl < SWP_SLOTS && pc >= 3 && pc < 91;
    vpt[i] = ((pr - 3) * 88 + pc - 3) * 16;
    ppr[i] = ok ? pr - 3 : -1000;                   // input row offset of the slot (-1000: never valid)
  }
  auto issue = [&](int pc, int t, char* buf) {      // DMA piece pc of tile t (dy pieces, then patch)
    const int img = t / SWP_TPI, oy0 = (t - img * SWP_TPI) * SWP_TR;
    if (pc < SWP_DYPIECE) {
      gemmg::bglds16(rdy, vdy[pc], (uint32_t)(img * 1936 + oy0 * 44) * 128u, buf + (wave + 4 * pc) * 1024);
    } else {
      const int i = pc - SWP_DYPIECE, y = 2 * oy0 + ppr[i];
      const uint32_t vo = (uint32_t)y < 88u ? (uint32_t)(img * 123904 + oy0 * 2816 + vpt[i]) : gemmg::OOB;
      gemmg::bglds16(rx, vo, 0u, buf + SWP_DYB + (wave + 4 * i) * 1024);
    }
  };
  // fragment bases: lane group g holds k = 8g + j <-> pixel 16(g >> 1) + 4(g & 1) + (j & 3) + 8(j >> 2)
  // of the k-step = row k >> 3, column 8 kb + (k & 7) of the tile
  const int g = lane >> 4, qq = (lane & 15) >> 2, pp = lane & 3;
  const int pxa = 16 * (g >> 1) + 4 * (g & 1) + qq;
  const int sw = whswz(pxa);
  int dA[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) dA[i] = pxa * 128 + (((2 * i + (pp >> 1)) ^ sw) << 4) + 8 * (pp & 1);
  const int pbase = SWP_DYB + (2 * (pxa >> 3) * SWP_PC + 2 * (pxa & 7)) * 16;
  int oB[SWP_JW];                                   // patch byte base of this lane per pair
#pragma unroll
  for (int j = 0; j < SWP_JW; ++j) oB[j] = pbase + swp_toff(2 * (wave + 4 * j) + (pp >> 1)) + 8 * (pp & 1);
  f32x4 acc[4][SWP_JW];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < SWP_JW; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  constexpr int PD = SWP_NBUF - 1, PER = SWP_NP / SWP_KS;
#pragma unroll
  for (int d = 0; d < PD; ++d)
    if (ta + d < tb)
#pragma unroll
      for (int pc = 0; pc < SWP_NP; ++pc) issue(pc, ta + d, smem + d * SWP_BUF);
  struct Fr { bf16x8 a[4], b[SWP_JW]; };
  // k-step kb: dy rows kb * 32 (+ 8: the next tile row), patch columns + 16 kb pixels (+ 2 rows)
  auto load = [&](Fr& f, const char* buf, int kb) {
#pragma unroll
    for (int i = 0; i < 4; ++i) f.a[i] = trpair(buf + dA[i] + kb * 4096, buf + dA[i] + kb * 4096 + 1024);
#pragma unroll
    for (int j = 0; j < SWP_JW; ++j) f.b[j] = trpair(buf + oB[j] + kb * 256, buf + oB[j] + kb * 256 + 2 * SWP_RB);
  };
  auto mma = [&](const Fr& f, int h) {            // output-channel tiles 2h, 2h + 1
#pragma unroll
    for (int i = 2 * h; i < 2 * h + 2; ++i)
#pragma unroll
      for (int j = 0; j < SWP_JW; ++j) acc[i][j] = mfma16(f.a[i], f.b[j], acc[i][j]);
  };
  for (int t = ta; t < tb; ++t) {
    const char* buf = smem + ((t - ta) % SWP_NBUF) * SWP_BUF;
    char* nbuf = smem + ((t + PD - ta) % SWP_NBUF) * SWP_BUF;
    const bool more = t + PD < tb;
    if (t + 1 < tb) gemmg::wait_vmcnt<SWP_NP>();   // tile t landed; tile t+1's DMAs may fly
    else gemmg::wait_vmcnt<0>();
    __builtin_amdgcn_s_barrier();                  // ... for every wave; every wave is done with tile t-1
    asm volatile("" ::: "memory");
    // two fragment sets in fixed roles (even / odd k-steps): no register copies
    Fr f0, f1;
    load(f0, buf, 0);
#pragma unroll
    for (int kb = 0; kb < SWP_KS; kb += 2) {
      mma(f0, 0);
      __builtin_amdgcn_sched_barrier(0);
      load(f1, buf, kb + 1);
      __builtin_amdgcn_sched_barrier(0);
      mma(f0, 1);
      if (more)
#pragma unroll
        for (int d = 0; d < PER; ++d) issue(kb * PER + d, t + PD, nbuf);
      mma(f1, 0);
      __builtin_amdgcn_sched_barrier(0);
      if (kb + 2 < SWP_KS) load(f0, buf, kb + 2);
      __builtin_amdgcn_sched_barrier(0);
      mma(f1, 1);
      if (more)
#pragma unroll
        for (int d = 0; d < PER; ++d) issue((kb + 1) * PER + d, t + PD, nbuf);
    }
  }
  // partial -> ws[block][co 64][392]: accumulator (i, j) register r = co 16i + 4g + r, column
  // 16 * pair + (lane & 15) = (tap 2 * pair + ((lane >> 3) & 1)) * 8 + channel (lane & 7)
  float* o = ws + (int64_t)blockIdx.x * 64 * SWP_COLS;
#pragma unroll
  for (int j = 0; j < SWP_JW; ++j) {
    const int col = 16 * (wave + 4 * j) + (lane & 15);
    if (col < SWP_COLS)
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int r = 0; r < 4; ++r) o[(16 * i + 4 * g + r) * SWP_COLS + col] = acc[i][j][r];
  }
}

}  // namespace

int wpatch_launch(const avsr_conv_params* p, hipStream_t st) {
  if (p->cin == 64) return wpatch_launch_g<WPStage1>(p, st);
  if (p->cin == 128) return wpatch_launch_g<WPStage2>(p, st);
  if (p->cin == 256) return wpatch_launch_g<WPStage3>(p, st);
  return wpatch_launch_g<WPStage4>(p, st);
}

int stem_wpatch_launch(const avsr_conv_params* p, hipStream_t st) {
  static bool attr = false;
  if (!attr) {
    (void)hipFuncSetAttribute((const void*)stem_wgrad_patch_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, SWP_LDS);
    attr = true;
  }
  const uint32_t xb = (uint32_t)((int64_t)p->nimg * 88 * 88 * 16), dyb = (uint32_t)((int64_t)p->nimg * 1936 * 128);
  hipLaunchKernelGGL(stem_wgrad_patch_kernel, dim3(SWP_BLOCKS), dim3(256), SWP_LDS, st, (const bf16*)p->x,
                     (const bf16*)p->dy, xb, dyb, p->nimg, p->ws);
  AVSR_CHECK_LAUNCH();
  return wgrad_reduce(p->ws, SWP_BLOCKS, 8, 64 * SWP_COLS, 1, p->dw, 0, st);
}
}  // namespace conv
