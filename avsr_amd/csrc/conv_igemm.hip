// Implicit-GEMM convolution, the general kernels: the register-staged conv_kernel (AVSR_CONV_PATH_REG:
// fp32) and the LDS-DMA conv_glds_kernel (_GLDS: bf16; also the class GEMMs of _S2), loaders and tiles.
//  fwd         C[m = y pixel][co]        = sum_{k=(kh,kw,ci)} x[im2col(m, k)] * w[co][k]
//              (+ fused BatchNorm partial statistics of the stored tile)
//  bwd_data    C[m = x pixel][ci]        = sum_{k=(kh,kw,co)} dy[col2im(m, k)] * w[co][kh][kw][ci]
//  bwd_weight  dw[co][(kh,kw,ci)]       += sum_{m = y pixel} dy[m][co] * x[im2col(m, (kh,kw,ci))]
//              (K = pixels is split over blocks: fp32 slabs, or fp32 atomics into the gradient)
#include "conv.h"

namespace conv {
namespace {

// fp32 only: bf16 runs conv_glds_kernel (T stays a parameter of the gemm_core.h pieces it is built of)
template <typename T, typename OutT, int WM, int WN, int KIND>
__global__ __launch_bounds__(NT) void conv_kernel(ConvArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  using TL = Tile<T, WM, WN>;   // BM/BN only (LDS sizing: launch below)
  const int z = blockIdx.z, grp = z / a.splits, sp = z % a.splits;
  const int m0 = blockIdx.y * TL::BM, n0 = blockIdx.x * TL::BN;
  const T* pa = (const T*)a.a + (int64_t)grp * a.a_gstride;
  const T* pb = (const T*)a.b + (int64_t)grp * a.b_gstride;
  f32x16 acc[2][2];
  const int kbeg = sp * a.kchunk, kend = min(a.K, kbeg + a.kchunk);
  if constexpr (KIND == K_FWD) {
    LdConvK<T, TL::BM, false> la; la.p = pa; la.g = a.g; la.rext = a.M; la.K = a.K;
    LdDenseK<T, TL::BN> lb; lb.p = pb; lb.ld = a.K; lb.rext = a.N; lb.K = a.K;
    mainloop<T, WM, WN>(la, lb, m0, n0, kbeg, kend, acc, smem);
  } else if constexpr (KIND == K_DGRAD) {
    LdConvK<T, TL::BM, true> la; la.p = pa; la.g = a.g; la.rext = a.M; la.K = a.K;
    LdWgtR<T, TL::BN> lb; lb.p = pb; lb.g = a.g; lb.rext = a.N; lb.K = a.K;
    mainloop<T, WM, WN>(la, lb, m0, n0, kbeg, kend, acc, smem);
  } else {
    LdDenseR<T, TL::BM> la; la.p = pa; la.ld = a.g.ldy; la.rext = a.M; la.K = a.K;
    LdConvR<T, TL::BN> lb; lb.p = pb; lb.g = a.g; lb.rext = a.N; lb.K = a.K;
    mainloop<T, WM, WN>(la, lb, m0, n0, kbeg, kend, acc, smem);
  }
  Epi e = a.e;
  if (KIND == K_WGRAD && a.ws) e.C = a.ws + ((int64_t)grp * a.splits + sp) * a.M * a.N;
  else e.C = (OutT*)e.C + (int64_t)grp * a.c_gstride;
  if (e.res) e.res = (const T*)e.res + (int64_t)grp * a.c_gstride;
  if (e.preact) e.preact = (T*)e.preact + (int64_t)grp * a.c_gstride;
  if (e.bias) e.bias += (int64_t)grp * a.c_gstride;
  epilogue<T, OutT, WM, WN>(e, m0, n0, acc, smem);
}

// ---------------------------------------------------------------- LDS-DMA (bf16) loaders
// Same operand views as the register-staged loaders (gemm_core.h), but every 16-byte vector is
// DMA'd straight into the swizzled LDS image (gemm_glds.h); invalid taps -> zero line.
using gemmg::glds16;
using gemmg::g_zero_line;

// A of forward (TRANSP=false: r = output pixel, gather x) / data-grad (TRANSP=true: r = input
// pixel, gather dy): k-major image, k = (kh, kw, c) with c fastest.
template <int R, int NW, bool TRANSP> struct GConvK {
  static constexpr bool KMAJ = true;
  static constexpr int SLOTS = R / 8 / NW;
  const bf16* p; ConvGeom g; int kend;
  int pn[SLOTS], ph_[SLOTS], pw_[SLOTS], kc[SLOTS];
  AVSR_DEV void init(const bf16* base, const ConvGeom& g_, int r0, int rext, int kend_, int wave, int lane) {
    p = base; g = g_; kend = kend_;
#pragma unroll
    for (int i = 0; i < SLOTS; ++i) {
      const int pc = i * NW + wave, pr = pc * 8 + (lane >> 3);
      kc[i] = ((lane & 7) ^ ((pr >> 1) & 7)) * 8;
      const int r = r0 + pr;
      if (r >= rext) { pn[i] = 0; ph_[i] = -1000000; pw_[i] = 0; continue; }
      if (!TRANSP) {
        uint32_t n = fdiv(r, g.f_hw_out); uint32_t rem = r - n * g.f_hw_out.d;
        uint32_t oh = fdiv(rem, g.f_w_out); uint32_t ow = rem - oh * g.f_w_out.d;
        pn[i] = n * g.hin * g.win; ph_[i] = oh * g.sh - g.ph; pw_[i] = ow * g.sw - g.pw;
      } else {
        uint32_t n = fdiv(r, g.f_hw_in); uint32_t rem = r - n * g.f_hw_in.d;
        uint32_t h = fdiv(rem, g.f_w_in); uint32_t w = rem - h * g.f_w_in.d;
        pn[i] = n * g.hout * g.wout; ph_[i] = h + g.ph; pw_[i] = w + g.pw;
      }
    }
  }
  AVSR_DEV void issue(char* img, int k0, int wave) const {
    const int cs = TRANSP ? g.cout_shift : g.cin_shift;
#pragma unroll
    for (int i = 0; i < SLOTS; ++i) {
      const int k = k0 + kc[i];
      const int c = k & ((1 << cs) - 1), khw = k >> cs;
      const int kh = fdiv(khw, g.f_kw), kw = khw - kh * g.f_kw.d;
      bool ok = k < kend;
      int64_t off;
      if (!TRANSP) {
        const int ih = ph_[i] + kh, iw = pw_[i] + kw;
        ok = ok && ih >= 0 && ih < g.hin && iw >= 0 && iw < g.win;
        off = (int64_t)(pn[i] + ih * g.win + iw) * g.ldx + c;
      } else {
        const int th = ph_[i] - kh, tw = pw_[i] - kw;
        const int oh = th / g.sh, ow = tw / g.sw;
        ok = ok && th >= 0 && tw >= 0 && oh * g.sh == th && ow * g.sw == tw && oh < g.hout && ow < g.wout;
        off = (int64_t)(pn[i] + oh * g.wout + ow) * g.ldy + c;
      }
      glds16(ok ? (const void*)(p + off) : (const void*)g_zero_line, img + (i * NW + wave) * 1024);
    }
  }
};

// B of data-grad: weight [cout][kh][kw][cin] viewed as (r = cin, k = (kh, kw, cout)); r-contiguous.
template <int R, int NW> struct GWgtR {
  static constexpr bool KMAJ = false;
  static constexpr int CPR = R / 8, RPP = 64 / CPR, SLOTS = GBK / RPP / NW;
  const bf16* p; ConvGeom g; int kend;
  int kr[SLOTS], rr[SLOTS];
  AVSR_DEV void init(const bf16* base, const ConvGeom& g_, int r0, int rext, int kend_, int wave, int lane) {
    p = base; g = g_; kend = kend_;
#pragma unroll
    for (int i = 0; i < SLOTS; ++i) {
      const int pc = i * NW + wave, pk = pc * RPP + lane / CPR;
      const int c = (lane % CPR) ^ gemmg::rswz<CPR>(pk);
      kr[i] = pk;
      rr[i] = r0 + c * 8 < rext ? r0 + c * 8 : -1;
    }
  }
  AVSR_DEV void issue(char* img, int k0, int wave) const {
    const int ktot = g.kh * g.kw * g.cin;
#pragma unroll
    for (int i = 0; i < SLOTS; ++i) {
      const int k = k0 + kr[i];
      const int co = k & ((1 << g.cout_shift) - 1), khw = k >> g.cout_shift;
      const bool ok = k < kend && rr[i] >= 0;
      glds16(ok ? (const void*)(p + (int64_t)co * ktot + khw * g.cin + rr[i]) : (const void*)g_zero_line,
             img + (i * NW + wave) * 1024);
    }
  }
};

// B of weight-grad: r = (kh, kw, cin) (vectors along cin), k = output pixel; r-contiguous.
template <int R, int NW> struct GConvR {
  static constexpr bool KMAJ = false;
  static constexpr int CPR = R / 8, RPP = 64 / CPR, SLOTS = GBK / RPP / NW;
  const bf16* p; ConvGeom g; int kend;
  int kr[SLOTS], rk[SLOTS], rw[SLOTS], rc[SLOTS];
  AVSR_DEV void init(const bf16* base, const ConvGeom& g_, int r0, int rext, int kend_, int wave, int lane) {
    p = base; g = g_; kend = kend_;
#pragma unroll
    for (int i = 0; i < SLOTS; ++i) {
      const int pc = i * NW + wave, pk = pc * RPP + lane / CPR;
      const int r = r0 + ((lane % CPR) ^ gemmg::rswz<CPR>(pk)) * 8;
      kr[i] = pk;
      if (r >= rext) { rk[i] = -1000000; rw[i] = 0; rc[i] = 0; continue; }
      const int c = r & ((1 << g.cin_shift) - 1), khw = r >> g.cin_shift;
      const int kh = fdiv(khw, g.f_kw);
      rk[i] = kh; rw[i] = khw - kh * g.f_kw.d; rc[i] = c;
    }
  }
  AVSR_DEV void issue(char* img, int k0, int wave) const {
#pragma unroll
    for (int i = 0; i < SLOTS; ++i) {
      const int k = k0 + kr[i];
      bool ok = k < kend;
      const uint32_t kk = ok ? k : 0;
      const uint32_t n = fdiv(kk, g.f_hw_out), rem = kk - n * g.f_hw_out.d;
      const uint32_t oh = fdiv(rem, g.f_w_out), ow = rem - oh * g.f_w_out.d;
      const int ih = (int)oh * g.sh - g.ph + rk[i], iw = (int)ow * g.sw - g.pw + rw[i];
      ok = ok && ih >= 0 && ih < g.hin && iw >= 0 && iw < g.win;
      glds16(ok ? (const void*)(p + (int64_t)(n * g.hin * g.win + ih * g.win + iw) * g.ldx + rc[i])
                : (const void*)g_zero_line,
             img + (i * NW + wave) * 1024);
    }
  }
};

// ---------------------------------------------------------------- buffer-DMA conv loaders
// Tap-uniform K-tiles: with cin (forward) / cout (data-grad) a multiple of 64, one K-tile of
// 64 lies inside one (kh, kw) tap, so the tap decomposition is wave-uniform (scalar) and a
// lane's work per DMA piece is its bounds check and one add (see gemm_glds.h BDenseK). The
// data-grad's B (BWgtR) is in conv.h.

// forward A: r = output pixel, gather x
template <int R, int NW> struct BConvK {
  static constexpr bool KMAJ = true;
  static constexpr int SLOTS = R / 8 / NW;
  __amdgpu_buffer_rsrc_t rs; ConvGeom g;
  int ih0[SLOTS], iw0[SLOTS], ro[SLOTS];
  AVSR_DEV void init(const bf16* base, uint32_t bytes, const ConvGeom& g_, int r0, int rext, int wave, int lane) {
    rs = make_rsrc(base, bytes); g = g_;
#pragma unroll
    for (int i = 0; i < SLOTS; ++i) {
      const int pc = i * NW + wave, pr = pc * 8 + (lane >> 3);
      const int kc = ((lane & 7) ^ ((pr >> 1) & 7)) * 8;
      const int r = r0 + pr;
      if (r >= rext) { ih0[i] = -1000000; iw0[i] = 0; ro[i] = 0; continue; }
      const uint32_t n = fdiv(r, g.f_hw_out), rem = r - n * g.f_hw_out.d;
      const uint32_t oh = fdiv(rem, g.f_w_out), ow = rem - oh * g.f_w_out.d;
      ih0[i] = oh * g.sh - g.ph; iw0[i] = ow * g.sw - g.pw;
      ro[i] = (int)((((int64_t)n * g.hin * g.win + (int64_t)ih0[i] * g.win + iw0[i]) * g.ldx + kc) * 2);
    }
  }
  AVSR_DEV void issue(char* img, int k0, int wave) const {
    const int khw = k0 >> g.cin_shift, cb = k0 & ((1 << g.cin_shift) - 1);
    const int kh = (int)fdiv(khw, g.f_kw), kw = khw - kh * (int)g.f_kw.d;
    const int tap = (int)(((int64_t)(kh * g.win + kw) * g.ldx + cb) * 2);
#pragma unroll
    for (int i = 0; i < SLOTS; ++i) {
      const bool ok = (unsigned)(ih0[i] + kh) < (unsigned)g.hin && (unsigned)(iw0[i] + kw) < (unsigned)g.win;
      bglds16(rs, ok ? (uint32_t)(ro[i] + tap) : OOB, 0u, img + (i * NW + wave) * 1024);
    }
  }
};

// data-grad A: r = input pixel, gather dy at ((h+ph-kh)/sh, (w+pw-kw)/sw); strides 1 or 2
template <int R, int NW> struct BConvKT {
  static constexpr bool KMAJ = true;
  static constexpr int SLOTS = R / 8 / NW;
  __amdgpu_buffer_rsrc_t rs; ConvGeom g;
  int th0[SLOTS], tw0[SLOTS], ro[SLOTS];
  AVSR_DEV void init(const bf16* base, uint32_t bytes, const ConvGeom& g_, int r0, int rext, int wave, int lane) {
    rs = make_rsrc(base, bytes); g = g_;
#pragma unroll
    for (int i = 0; i < SLOTS; ++i) {
      const int pc = i * NW + wave, pr = pc * 8 + (lane >> 3);
      const int kc = ((lane & 7) ^ ((pr >> 1) & 7)) * 8;
      const int r = r0 + pr;
      if (r >= rext) { th0[i] = -1000000; tw0[i] = 0; ro[i] = 0; continue; }
      const uint32_t n = fdiv(r, g.f_hw_in), rem = r - n * g.f_hw_in.d;
      const uint32_t h = fdiv(rem, g.f_w_in), w = rem - h * g.f_w_in.d;
      th0[i] = h + g.ph; tw0[i] = w + g.pw;
      ro[i] = (int)(((int64_t)n * g.hout * g.wout * g.ldy + kc) * 2);
    }
  }
  AVSR_DEV void issue(char* img, int k0, int wave) const {
    const int khw = k0 >> g.cout_shift, cb = k0 & ((1 << g.cout_shift) - 1);
    const int kh = (int)fdiv(khw, g.f_kw), kw = khw - kh * (int)g.f_kw.d;
    const int ldy2 = (int)g.ldy * 2, cb2 = cb * 2;
#pragma unroll
    for (int i = 0; i < SLOTS; ++i) {
      const int th = th0[i] - kh, tw = tw0[i] - kw;
      bool ok;
      int pix;
      if (g.sh == 1) {
        ok = (unsigned)th < (unsigned)g.hout && (unsigned)tw < (unsigned)g.wout;
        pix = th * g.wout + tw;
      } else {
        ok = ((th | tw) & 1) == 0 && (unsigned)(th >> 1) < (unsigned)g.hout && (unsigned)(tw >> 1) < (unsigned)g.wout;
        pix = (th >> 1) * g.wout + (tw >> 1);
      }
      bglds16(rs, ok ? (uint32_t)(ro[i] + pix * ldy2 + cb2) : OOB, 0u, img + (i * NW + wave) * 1024);
    }
  }
};

// weight-grad B: r = (kh, kw, cin) (vectors along cin), k = output pixel; r-contiguous
template <int R, int NW> struct BConvR {
  static constexpr bool KMAJ = false;
  static constexpr int CPR = R / 8, RPP = 64 / CPR, SLOTS = GBK / RPP / NW;
  __amdgpu_buffer_rsrc_t rs; ConvGeom g; int kend;
  int kr[SLOTS], rk[SLOTS], rw[SLOTS], rc[SLOTS];
  AVSR_DEV void init(const bf16* base, uint32_t bytes, const ConvGeom& g_, int r0, int rext, int kend_, int wave, int lane) {
    rs = make_rsrc(base, bytes); g = g_; kend = kend_;
#pragma unroll
    for (int i = 0; i < SLOTS; ++i) {
      const int pc = i * NW + wave, pk = pc * RPP + lane / CPR;
      const int r = r0 + ((lane % CPR) ^ gemmg::rswz<CPR>(pk)) * 8;
      kr[i] = pk;
      if (r >= rext) { rk[i] = -1000000; rw[i] = 0; rc[i] = 0; continue; }
      const int c = r & ((1 << g.cin_shift) - 1), khw = r >> g.cin_shift;
      const int kh = fdiv(khw, g.f_kw);
      rk[i] = kh - g.ph; rw[i] = khw - kh * g.f_kw.d - g.pw; rc[i] = c * 2;
    }
  }
  AVSR_DEV void issue(char* img, int k0, int wave) const {
    const int ldx2 = (int)g.ldx * 2;
#pragma unroll
    for (int i = 0; i < SLOTS; ++i) {
      const int k = k0 + kr[i];
      const uint32_t kk = k < kend ? k : 0;
      const uint32_t n = fdiv(kk, g.f_hw_out), rem = kk - n * g.f_hw_out.d;
      const uint32_t oh = fdiv(rem, g.f_w_out), ow = rem - oh * g.f_w_out.d;
      const int ih = (int)oh * g.sh + rk[i], iw = (int)ow * g.sw + rw[i];
      const bool ok = k < kend && (unsigned)ih < (unsigned)g.hin && (unsigned)iw < (unsigned)g.win;
      const uint32_t v = (uint32_t)(((int)n * g.hin * g.win + ih * g.win + iw) * ldx2 + rc[i]);
      bglds16(rs, ok ? v : OOB, 0u, img + (i * NW + wave) * 1024);
    }
  }
};

template <typename OutT, int KIND, class CF>
__global__ __launch_bounds__(CF::NTH, CF::MINB) void conv_glds_kernel(ConvArgs a, int tiles_m, int tiles_n) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int id = gemmg::xcd_remap(blockIdx.x, gridDim.x);
  int tm, tn, z;
  gemmg::tile_of(id, tiles_m, tiles_n, tm, tn, z);
  const int grp = z / a.splits, sp = z % a.splits;
  const int m0 = tm * CF::BM, n0 = tn * CF::BN;
  const bf16* pa = (const bf16*)a.a + (int64_t)grp * a.a_gstride;
  const bf16* pb = (const bf16*)a.b + (int64_t)grp * a.b_gstride;
  const int kbeg = sp * a.kchunk, kend = min(a.K, kbeg + a.kchunk);
  const int nk = (kend - kbeg + GBK - 1) / GBK;
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  f32x4 acc[CF::TM][CF::TN];
  if (a.a_bytes) {                // buffer-DMA loaders (tap-uniform K-tiles, extents < 2 GiB)
    if constexpr (KIND == K_FWD) {
      BConvK<CF::BM, CF::NW> la; la.init(pa, a.a_bytes, a.g, m0, a.M, wave, lane);
      gemmg::BDenseK<CF::BN, CF::NW> lb; lb.init(pb, a.b_bytes, a.K, n0, a.N, kend, wave, lane);
      gemmg::mainloop_glds<CF>(la, lb, kbeg, nk, acc, smem);
    } else if constexpr (KIND == K_DGRAD || KIND >= K_DGRAD_BNR) {
      BConvKT<CF::BM, CF::NW> la; la.init(pa, a.a_bytes, a.g, m0, a.M, wave, lane);
      BWgtR<CF::BN, CF::NW> lb; lb.init(pb, a.b_bytes, a.g, n0, a.N, wave, lane);
      gemmg::mainloop_glds<CF>(la, lb, kbeg, nk, acc, smem);
    } else {
      gemmg::BDenseR<CF::BM, CF::NW> la; la.init(pa, a.a_bytes, a.g.ldy, m0, a.M, kend, wave, lane);
      BConvR<CF::BN, CF::NW> lb; lb.init(pb, a.b_bytes, a.g, n0, a.N, kend, wave, lane);
      gemmg::mainloop_glds<CF>(la, lb, kbeg, nk, acc, smem);
    }
  } else if constexpr (KIND == K_FWD) {
    GConvK<CF::BM, CF::NW, false> la; la.init(pa, a.g, m0, a.M, kend, wave, lane);
    gemmg::GDenseK<CF::BN, CF::NW> lb; lb.init(pb, a.K, n0, a.N, kend, wave, lane);
    gemmg::mainloop_glds<CF>(la, lb, kbeg, nk, acc, smem);
  } else if constexpr (KIND == K_DGRAD || KIND >= K_DGRAD_BNR) {
    GConvK<CF::BM, CF::NW, true> la; la.init(pa, a.g, m0, a.M, kend, wave, lane);
    GWgtR<CF::BN, CF::NW> lb; lb.init(pb, a.g, n0, a.N, kend, wave, lane);
    gemmg::mainloop_glds<CF>(la, lb, kbeg, nk, acc, smem);
  } else {
    gemmg::GDenseR<CF::BM, CF::NW> la; la.init(pa, a.g.ldy, m0, a.M, kend, wave, lane);
    GConvR<CF::BN, CF::NW> lb; lb.init(pb, a.g, n0, a.N, kend, wave, lane);
    gemmg::mainloop_glds<CF>(la, lb, kbeg, nk, acc, smem);
  }
  if constexpr (KIND >= K_DGRAD_BNR) {
    gemmg::epilogue_bnr<CF, KIND - K_DGRAD_BNR>(a.e, a.bnr, m0, n0, acc, smem);
    return;
  }
  Epi e = a.e;
  if (KIND == K_WGRAD && a.ws) e.C = a.ws + ((int64_t)grp * a.splits + sp) * a.M * a.N;
  else e.C = (OutT*)e.C + (int64_t)grp * a.c_gstride;
  if (e.res) e.res = (const bf16*)e.res + (int64_t)grp * a.c_gstride;
  if (e.preact) e.preact = (bf16*)e.preact + (int64_t)grp * a.c_gstride;
  if (e.bias) e.bias += (int64_t)grp * a.c_gstride;
  gemmg::epilogue_g<bf16, OutT, CF>(e, m0, n0, acc, smem);
}

// the tiles, by the plan's row-tile height (conv.hip row_tile: 192 where conv192 says it pays)
using CCfg128 = gemmg::GCfg<2, 2, 2, 2, 2>;    // 128x128
using CCfg256x64 = gemmg::GCfg<4, 1, 2, 2, 2>; // 256x64  (N <= 64: cout / cin = 64)
using CCfg64x256 = gemmg::GCfg<1, 4, 2, 2, 2>; // 64x256  (M <= 64: weight-grad with cout = 64)
using CCfg192 = gemmg::GCfg<2, 2, 3, 2, 2>;    // 192x128 (96x64 per wave), k-major A (fwd / data-grad)

template <typename OutT, int KIND, class CF>
int launch_glds(const ConvArgs& a, int groups, hipStream_t st) {
  const int tm = (a.M + CF::BM - 1) / CF::BM, tn = (a.N + CF::BN - 1) / CF::BN;
  if (a.e.stats && a.e.stats_tiles != tm) return AVSR_E_SHAPE;   // partials sized for another tile height
  const long nwg = (long)tm * tn * groups * a.splits;
  if (nwg > 0x7fffffffL) return AVSR_E_SHAPE;
  hipLaunchKernelGGL((conv_glds_kernel<OutT, KIND, CF>), dim3((unsigned)nwg), dim3(CF::NTH), CF::LDS_BYTES, st, a,
                     tm, tn);
  AVSR_CHECK_LAUNCH();
  return 0;
}

template <typename OutT, int KIND>
int glds_by_tile(int bm, const ConvArgs& a, int groups, hipStream_t st) {
  if constexpr (KIND != K_WGRAD) {
    if (bm == 192) return launch_glds<OutT, KIND, CCfg192>(a, groups, st);
  }
  if (bm == 256) return launch_glds<OutT, KIND, CCfg256x64>(a, groups, st);
  if (bm == 64) return launch_glds<OutT, KIND, CCfg64x256>(a, groups, st);
  return bm == 128 ? launch_glds<OutT, KIND, CCfg128>(a, groups, st) : AVSR_E_ARG;
}

template <typename T, typename OutT, int WM, int WN, int KIND>
int launch(const ConvArgs& a, int groups, hipStream_t st) {
  // operand kinds per convolution direction (fwd: K/K, dgrad: K/R, wgrad: R/R)
  using TL = Tile<T, WM, WN, KIND != K_WGRAD, KIND == K_FWD>;
  dim3 grid((a.N + TL::BN - 1) / TL::BN, (a.M + TL::BM - 1) / TL::BM, groups * a.splits);
  if (a.e.stats && a.e.stats_tiles != (int)grid.y) return AVSR_E_SHAPE;   // partials sized for another tile height
  if (grid.y > 65535) return AVSR_E_SHAPE;
  hipLaunchKernelGGL((conv_kernel<T, OutT, WM, WN, KIND>), grid, dim3(NT), TL::LDS_BYTES, st, a);
  AVSR_CHECK_LAUNCH();
  return 0;
}

template <int KIND>
int f32_by_tile(int bm, const ConvArgs& a, int groups, hipStream_t st) {
  if (bm == 256) return launch<float, float, 4, 1, KIND>(a, groups, st);
  if (bm == 64) return launch<float, float, 1, 4, KIND>(a, groups, st);
  return bm == 128 ? launch<float, float, 2, 2, KIND>(a, groups, st) : AVSR_E_ARG;
}

}  // namespace

int igemm_f32(int kind, int bm, const ConvArgs& a, int groups, hipStream_t st) {
  if (kind == K_FWD) return f32_by_tile<K_FWD>(bm, a, groups, st);
  if (kind == K_DGRAD) return f32_by_tile<K_DGRAD>(bm, a, groups, st);
  return kind == K_WGRAD ? f32_by_tile<K_WGRAD>(bm, a, groups, st) : AVSR_E_ARG;
}

int igemm_glds(int kind, int bm, const ConvArgs& a, int groups, hipStream_t st) {
  switch (kind) {
    case K_FWD: return glds_by_tile<bf16, K_FWD>(bm, a, groups, st);
    case K_DGRAD: return glds_by_tile<bf16, K_DGRAD>(bm, a, groups, st);
    case K_WGRAD: return glds_by_tile<float, K_WGRAD>(bm, a, groups, st);
    case K_DGRAD_BNR: return glds_by_tile<bf16, K_DGRAD_BNR>(bm, a, groups, st);
    case K_DGRAD_BNR + 1: return glds_by_tile<bf16, K_DGRAD_BNR + 1>(bm, a, groups, st);
    case K_DGRAD_BNR + 2: return glds_by_tile<bf16, K_DGRAD_BNR + 2>(bm, a, groups, st);
    default: return AVSR_E_ARG;
  }
}
}  // namespace conv
