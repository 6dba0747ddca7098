// Implicit-GEMM convolution (NHWC, grouped) forward / data-grad / weight-grad: the C ABI (avsr_conv_*,
// include/avsr_hip.h), the choice of kernel family (conv_plan; the families: AVSR_CONV_PATH_* there),
// the stride-2 parity classes and the ordered slab reduce. The kernels: conv_igemm.hip (REG, GLDS and
// the class GEMMs of S2), conv_patch.hip (PATCH), conv_wpatch.hip (WPATCH, STEM_WPATCH); shared: conv.h.
#include "conv.h"

namespace conv {
namespace {

int ilog2(int v) { int s = 0; while ((1 << s) < v) ++s; return (1 << s) == v ? s : -1; }

int make_geom(const avsr_conv_params* p, ConvGeom& g) {
  g.nimg = p->nimg; g.hin = p->hin; g.win = p->win; g.hout = p->hout; g.wout = p->wout;
  g.kh = p->kh; g.kw = p->kw; g.sh = p->sh; g.sw = p->sw; g.ph = p->ph; g.pw = p->pw;
  g.cin = p->cin; g.cout = p->cout; g.ldx = p->ldx; g.ldy = p->ldy;
  g.f_hw_out = make_fastdiv((uint32_t)(p->hout * p->wout));
  g.f_w_out = make_fastdiv((uint32_t)p->wout);
  g.f_hw_in = make_fastdiv((uint32_t)(p->hin * p->win));
  g.f_w_in = make_fastdiv((uint32_t)p->win);
  g.f_kw = make_fastdiv((uint32_t)p->kw);
  g.cin_shift = ilog2(p->cin); g.cout_shift = ilog2(p->cout);
  g.ktot_w = p->kh * p->kw * p->cin; g.tap_kfw = p->kw; g.tap_kh0 = 0; g.tap_kw0 = 0; g.tap_step = 1;
  const int ve = p->dtype == AVSR_BF16 ? 8 : 4;
  if (g.cin_shift < 0 || g.cout_shift < 0 || p->cin < ve || p->cout < ve) return AVSR_E_SHAPE;
  if (p->ldx % ve || p->ldy % ve) return AVSR_E_ALIGN;
  if (p->groups < 1 || p->ldx < (int64_t)p->groups * p->cin || p->ldy < (int64_t)p->groups * p->cout) return AVSR_E_SHAPE;
  return 0;
}

// ---------------------------------------------------------------- the plan and its predicates
// 192x128 for the k-major-A directions (forward, data-grad) where it still runs >= 2 blocks per
// CU and its rounds carry no more work than 128x128's (the dense rule, gemm.hip tile_cfg):
// ResNet stages 2-3 at C2 (video fwd 9.09 -> 8.83 ms, bwd 17.13 -> 16.84, profiles/r02_resnet_c192_ab.txt)
bool conv192(int M, int N, int groups) {
  if (N <= 64 || M <= 64 || !avsr_opt(AVSR_OPT_CONV_192)) return false;
  const long tn = (long)((N + 127) / 128) * groups;
  const long n128 = ((long)((M + 127) / 128) * tn + 255) / 256, n192 = ((long)((M + 191) / 192) * tn + 255) / 256;
  return n192 >= 2 && 3 * n192 * 50 <= 2 * n128 * 51;
}

// row-tile height of the general kernels: N <= 64 -> 256x64; M <= 64 -> 64x256; else 128x128, or
// 192x128 (c192: a bf16 forward / data-grad) where conv192 says it pays
int row_tile(int M, int N, int groups, bool c192) {
  if (c192 && conv192(M, N, groups)) return 192;
  return N <= 64 ? 256 : (M <= 64 ? 64 : 128);
}

// extents (elements, one group) of the A / B operands -> buffer-DMA loaders when allowed
void set_extents(ConvPlan& pl, bool allowed, int64_t ea, int64_t eb) {
  const int64_t lim = ((int64_t)OOB - (1 << 20)) / 2;
  const bool ok = allowed && ea > 0 && eb > 0 && ea < lim && eb < lim;
  pl.a_bytes = ok ? (uint32_t)(ea * 2) : 0u;
  pl.b_bytes = ok ? (uint32_t)(eb * 2) : 0u;
}

// weight-gradient split-K plan. The LDS-DMA path writes per-split fp32 slabs (plain stores)
// and reduces them afterwards: device-scope fp32 atomics on the 8-XCD part are resolved beyond
// the per-XCD L2 and sustain only ~50 G adds/s (measured: splits x M x N atomics dominated the
// ResNet wgrad at 683 splits), while a slab costs 8 bytes/float of HBM traffic.
WgradPlan wgrad_plan(const avsr_conv_params* p, int bm, bool glds, bool with_ws) {
  const int M = p->cout, N = p->kh * p->kw * p->cin, K = p->nimg * p->hout * p->wout;
  const int bn = N <= 64 ? 64 : (M <= 64 ? 256 : 128);
  const long tiles = (long)((M + bm - 1) / bm) * ((N + bn - 1) / bn) * p->groups;
  WgradPlan w;
  const int kq = glds ? GBK : BKE;
  long splits = p->splitk;
  w.slab = with_ws;   // deterministic: per-split slabs + an ordered reduce (no fp32 atomics)
  if (splits <= 0) {
    // slab: ~2 full rounds of 512 block slots (2 per CU), rounded DOWN so the last round is
    // not a 1-block tail (513 blocks cost 2 rounds: measured 812 -> ~550 us on stage 1)
    const long target = w.slab ? 1024 : 2048;   // 512-2048 measured within noise (r02_conv_wgrad_target_ab)
    const long want = w.slab ? (target / tiles > 0 ? target / tiles : 1) : (target + tiles - 1) / tiles;
    const long maxs = w.slab ? (K + 1023) / 1024 : (K + 2047) / 2048;
    splits = want < maxs ? want : maxs;
    if (splits < 1) splits = 1;
  }
  w.kchunk = (int)(((K + splits - 1) / splits + kq - 1) / kq * kq);
  w.splits = (K + w.kchunk - 1) / w.kchunk;
  if (w.splits <= 1) { w.splits = 1; w.slab = false; }
  return w;
}

// Stride-2 data-grad by parity class of the input pixel. Class (a, b) = pixels (2i+a, 2j+b)
// receives contributions only from the taps kh = kh0 + 2u, kh0 = (a + ph) mod 2 (kw likewise),
// through dy at (i + ci - u, j + cj - v), ci = (a + ph - kh0) / 2: a stride-1 data-grad over
// the class grid. The four class GEMMs do 1/4 of the multiply-adds of the full one, whose
// other taps land on the zeros between the strided output pixels. A class with no taps (1x1
// kernels) still runs its epilogue (zeros, or the fused BatchNorm reduction of beta * dx).
struct S2Class { int a, b, hc, wc, nkh, nkw, kh0, kw0, ci, cj; };

void s2_classes(const avsr_conv_params* p, S2Class (&c)[4]) {
  for (int q = 0; q < 4; ++q) {
    S2Class& k = c[q];
    k.a = q >> 1; k.b = q & 1;
    k.hc = (p->hin - k.a + 1) / 2; k.wc = (p->win - k.b + 1) / 2;
    k.kh0 = (k.a + p->ph) & 1; k.kw0 = (k.b + p->pw) & 1;
    k.nkh = k.kh0 < p->kh ? (p->kh - k.kh0 + 1) / 2 : 0;
    k.nkw = k.kw0 < p->kw ? (p->kw - k.kw0 + 1) / 2 : 0;
    k.ci = (k.a + p->ph - k.kh0) / 2; k.cj = (k.b + p->pw - k.kw0) / 2;
  }
}

// the parity-class path: bf16 buffer-DMA loaders (pl: the data-grad's extents), one group, stride 2
bool s2_phase(const avsr_conv_params* p, const ConvPlan& pl) {
  if (!avsr_opt(AVSR_OPT_CONV_S2PHASE)) return false;
  return p->sh == 2 && p->sw == 2 && p->groups == 1 && p->cout % 64 == 0 && pl.a_bytes != 0;
}

// the patch-resident 3x3 kernel applies (buffer-DMA extents, 3x3 / stride 1 / pad 1, 64 -> 64 channels)
bool patch_ok(const avsr_conv_params* p, const ConvPlan& pl) {
  if (!avsr_opt(AVSR_OPT_CONV_PATCH) || !pl.a_bytes || p->groups != 1) return false;
  if (p->kh != 3 || p->kw != 3 || p->sh != 1 || p->sw != 1 || p->ph != 1 || p->pw != 1) return false;
  if (p->cin != 64 || p->cout != 64 || p->ldx != 64 || p->ldy != 64) return false;
  if (p->hin != p->hout || p->win != p->wout) return false;
  // worst-case padded span of 256 consecutive output pixels, plus the tap halo on both sides
  const int64_t W = p->win, HW = (int64_t)p->hin * p->win, Wp = W + 2;
  const int64_t span = (PCfg::BM - 1) + 2 * ((PCfg::BM - 1) / W + 1) + 2 * Wp * ((PCfg::BM - 1) / HW + 1) + 2 * (Wp + 1) + 1;
  return span <= PATCH_ROWS;
}

// the patch-resident weight-grad applies: automatic split, 3x3 / stride 1 / pad 1, one group, the
// stage-1 (22 x 22, 64 -> 64), stage-2 (11 x 11, 128 -> 128), stage-3 (6 x 6, 256 -> 256) or
// stage-4 (3 x 3, 512 -> 512) geometry
bool wpatch_ok(const avsr_conv_params* p) {
  if (!avsr_opt(AVSR_OPT_CONV_WPATCH) || p->groups != 1 || p->splitk > 0) return false;
  if (p->kh != 3 || p->kw != 3 || p->sh != 1 || p->sw != 1 || p->ph != 1 || p->pw != 1) return false;
  if (p->cin != p->cout || p->ldx != p->cin || p->ldy != p->cout || p->hin != p->hout || p->win != p->wout) return false;
  if (p->hin != p->win) return false;
  const int64_t bytes = (int64_t)p->nimg * p->hin * p->win * p->cin * 2;
  if (bytes <= 0 || bytes >= (int64_t)OOB - (1 << 20)) return false;
  return (p->cin == 64 && p->hin == 22) || (p->cin == 128 && p->hin == 11) || (p->cin == 256 && p->hin == 6) ||
         (p->cin == 512 && p->hin == 3);
}

// the stem geometry on the packed input, automatic split, both tensors below the 2 GiB buffer extent
bool stem_wpatch_ok(const avsr_conv_params* p) {
  if (!avsr_opt(AVSR_OPT_STEM_WPATCH) || p->groups != 1 || p->splitk > 0) return false;
  if (p->cin != 8 || p->ldx != 8 || p->cout != 64 || p->ldy != 64 || p->kh != 7 || p->kw != 7) return false;
  if (p->sh != 2 || p->sw != 2 || p->ph != 3 || p->pw != 3 || p->hin != 88 || p->win != 88) return false;
  if (p->hout != 44 || p->wout != 44) return false;
  const int64_t dyb = (int64_t)p->nimg * 1936 * 128;
  return dyb > 0 && dyb < (int64_t)OOB - (1 << 20);
}

// The kernel family of a call whose geometry make_geom accepted, and what follows from it: the one
// place that decides them. pass: AVSR_CONV_FWD / _DGRAD / _WGRAD.
int conv_plan(const avsr_conv_params* p, int pass, ConvPlan& pl) {
  if (p->dtype != AVSR_BF16 && p->dtype != AVSR_F32) return AVSR_E_DTYPE;
  const bool bf = p->dtype == AVSR_BF16;
  pl = ConvPlan{};
  pl.path = bf ? AVSR_CONV_PATH_GLDS : AVSR_CONV_PATH_REG;
  // extents (elements, one group) of x, of y / dy and of w
  const int64_t ktot = (int64_t)p->kh * p->kw * p->cin, ew = p->cout * ktot;
  const int64_t ex = ((int64_t)p->nimg * p->hin * p->win - 1) * p->ldx + p->cin;
  const int64_t ey = ((int64_t)p->nimg * p->hout * p->wout - 1) * p->ldy + p->cout;
  if (pass == AVSR_CONV_WGRAD) {
    set_extents(pl, bf, ey, ex);
    pl.bm = row_tile(p->cout, (int)ktot, p->groups, false);
    if (p->nimg * p->hout * p->wout == 0) return 0;
    // the workspace is sized before the caller has one: as the call with a workspace will run
    const WgradPlan sized = wgrad_plan(p, pl.bm, bf, true);
    const int patch = !bf ? 0 : wpatch_ok(p) ? AVSR_CONV_PATH_WPATCH : stem_wpatch_ok(p) ? AVSR_CONV_PATH_STEM_WPATCH : 0;
    pl.ws_floats = patch == AVSR_CONV_PATH_WPATCH        ? (int64_t)WP_BLOCKS * 64 * WP_COLS
                   : patch == AVSR_CONV_PATH_STEM_WPATCH ? (int64_t)SWP_BLOCKS * 64 * SWP_COLS
                   : sized.slab                          ? (int64_t)p->groups * sized.splits * p->cout * ktot
                                                         : 0;
    if (p->ws && patch) pl.path = patch;     // patch-resident, ordered slab reduce
    pl.w = p->ws ? sized : wgrad_plan(p, pl.bm, bf, false);
    return 0;
  }
  const bool fwd = pass == AVSR_CONV_FWD;
  const int M = p->nimg * (fwd ? p->hout * p->wout : p->hin * p->win), N = fwd ? p->cout : p->cin;
  if (fwd) set_extents(pl, bf && (p->cin % 64) == 0, ex, ew);
  else set_extents(pl, bf && (p->cout % 64) == 0 && (p->sh == 1 || p->sh == 2) && p->sw == p->sh, ey, ew);
  if (!fwd && s2_phase(p, pl)) {
    pl.path = AVSR_CONV_PATH_S2;
    S2Class cl[4];
    s2_classes(p, cl);
    for (int q = 0; q < 4; ++q) {
      const int Mc = p->nimg * cl[q].hc * cl[q].wc;
      pl.cls_bm[q] = row_tile(Mc, N, 1, true);
      pl.cls_tiles[q] = (Mc + pl.cls_bm[q] - 1) / pl.cls_bm[q];
      pl.tiles += pl.cls_tiles[q];
    }
    return 0;
  }
  // a forward epilogue beyond the BN statistics keeps the call on the general kernel
  if (patch_ok(p, pl) && !(fwd && (p->bias || p->act || p->res || p->preact))) {
    pl.path = AVSR_CONV_PATH_PATCH;
    pl.bm = PCfg::BM;
  } else {
    pl.bm = row_tile(M, N, p->groups, bf);
  }
  pl.tiles = (M + pl.bm - 1) / pl.bm;
  return 0;
}

// ---------------------------------------------------------------- ordered slab reduce
// dw[g] += sum over the splits of ws[g][s], in split order (deterministic). With chunks > 1
// (few output elements, many splits) a first pass folds each chunk of splits into its first
// slab (in place), and a second pass (chunks == -nchunks) sums those chunk heads in order.
__global__ __launch_bounds__(256) void wgrad_reduce_kernel(float* ws, int splits, int chunks, int64_t mn,
                                                           float* dw, int64_t dw_gstride) {
  const int g = blockIdx.y, c = blockIdx.z;
  float* w = ws + (int64_t)g * splits * mn;
  float* d = dw + (int64_t)g * dw_gstride;
  const int nch = chunks < 0 ? -chunks : chunks;
  for (int64_t i = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 4; i < mn; i += (int64_t)gridDim.x * 1024) {
    f32x4 s = {0.f, 0.f, 0.f, 0.f};
    if (chunks < 0) {            // pass 2: the chunk heads
      for (int q = 0; q < nch; ++q) s += *(const f32x4*)(w + (int64_t)((int64_t)splits * q / nch) * mn + i);
    } else {
      const int s0 = (int)((int64_t)splits * c / chunks), s1 = (int)((int64_t)splits * (c + 1) / chunks);
      for (int q = s0; q < s1; ++q) s += *(const f32x4*)(w + (int64_t)q * mn + i);
      if (chunks > 1) {          // pass 1: fold into the chunk's first slab
        *(f32x4*)(w + (int64_t)s0 * mn + i) = s;
        continue;
      }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) d[i + r] += s[r];   // dw is a view into the parameter arena: 4-byte aligned only
  }
}

int s2_launch(int kind, const ConvArgs& a0, const avsr_conv_params* p, const ConvPlan& pl, hipStream_t st) {
  S2Class cl[4];
  s2_classes(p, cl);
  int64_t tile_off = 0;
  for (int q = 0; q < 4; ++q) {
    const S2Class& k = cl[q];
    const int Mc = p->nimg * k.hc * k.wc;
    if (Mc == 0) continue;
    ConvArgs a = a0;
    a.g.hin = k.hc; a.g.win = k.wc; a.g.kh = k.nkh; a.g.kw = k.nkw; a.g.sh = 1; a.g.sw = 1;
    a.g.ph = k.ci; a.g.pw = k.cj;
    a.g.f_hw_in = make_fastdiv((uint32_t)(k.hc * k.wc));
    a.g.f_w_in = make_fastdiv((uint32_t)k.wc);
    a.g.f_kw = make_fastdiv((uint32_t)(k.nkw > 0 ? k.nkw : 1));
    a.g.tap_kh0 = k.kh0; a.g.tap_kw0 = k.kw0; a.g.tap_step = 2;
    a.M = Mc; a.K = k.nkh * k.nkw * p->cout; a.kchunk = a.K;
    a.e.M = Mc;
    a.e.rm_wc = k.wc; a.e.rm_hc = k.hc; a.e.rm_hin = p->hin; a.e.rm_win = p->win; a.e.rm_a = k.a; a.e.rm_b = k.b;
    if (kind >= K_DGRAD_BNR) a.bnr.ws = a0.bnr.ws + tile_off * 4 * a.N;
    tile_off += pl.cls_tiles[q];
    if (kind == K_DGRAD && a.K == 0 && a.e.beta == 1.f) continue;   // dx += 0
    const int rc = igemm_glds(kind, pl.cls_bm[q], a, 1, st);
    if (rc) return rc;
  }
  return 0;
}

// the plan of a size query: no validation beyond the plan's own (0 tiles / floats for a bad dtype)
bool query_plan(const avsr_conv_params* p, int pass, ConvPlan& pl) { return p && conv_plan(p, pass, pl) == 0; }

}  // namespace

int wgrad_reduce(float* ws, int splits, int chunks, int64_t mn, int groups, float* dw, int64_t dw_gstride, hipStream_t st) {
  const int xb = avsr_grid(mn / 4, 256, 1024);
  hipLaunchKernelGGL(wgrad_reduce_kernel, dim3((unsigned)xb, (unsigned)groups, (unsigned)chunks), dim3(256), 0, st, ws,
                     splits, chunks, mn, dw, dw_gstride);
  AVSR_CHECK_LAUNCH();
  if (chunks > 1) {
    hipLaunchKernelGGL(wgrad_reduce_kernel, dim3((unsigned)xb, (unsigned)groups, 1u), dim3(256), 0, st, ws, splits,
                       -chunks, mn, dw, dw_gstride);
    AVSR_CHECK_LAUNCH();
  }
  return 0;
}
}  // namespace conv
using namespace conv;

extern "C" int avsr_conv_path(const avsr_conv_params* p, int pass) {
  if (!p || pass < AVSR_CONV_FWD || pass > AVSR_CONV_WGRAD) return AVSR_E_ARG;
  ConvGeom g;
  ConvPlan pl;
  int rc = make_geom(p, g);
  if (!rc) rc = conv_plan(p, pass, pl);
  return rc ? rc : pl.path;
}

extern "C" int avsr_conv_stat_tiles(const avsr_conv_params* p) {
  ConvPlan pl;
  return query_plan(p, AVSR_CONV_FWD, pl) ? pl.tiles : 0;
}

extern "C" int avsr_conv_bnr_tiles(const avsr_conv_params* p) {
  ConvPlan pl;
  return query_plan(p, AVSR_CONV_DGRAD, pl) ? pl.tiles : 0;
}

extern "C" int64_t avsr_conv_wgrad_ws(const avsr_conv_params* p) {
  ConvPlan pl;
  return query_plan(p, AVSR_CONV_WGRAD, pl) ? pl.ws_floats : 0;
}

extern "C" int avsr_conv_fwd(const avsr_conv_params* p, void* stream) {
  if (!p) return AVSR_E_ARG;
  ConvArgs a{};   // every field the call does not set: 0 / null
  int rc = make_geom(p, a.g);
  if (rc) return rc;
  if (!avsr_aligned16(p->x) || !avsr_aligned16(p->w) || !avsr_aligned16(p->y)) return AVSR_E_ALIGN;
  if (p->stats && p->groups != 1) return AVSR_E_ARG;
  a.a = p->x; a.b = p->w;
  a.a_gstride = p->cin; a.b_gstride = (int64_t)p->cout * p->kh * p->kw * p->cin; a.c_gstride = p->cout;
  a.M = p->nimg * p->hout * p->wout; a.N = p->cout; a.K = p->kh * p->kw * p->cin;
  a.splits = 1; a.kchunk = a.K;
  a.e.M = a.M; a.e.N = a.N; a.e.C = p->y; a.e.ldc = p->ldy; a.e.alpha = 1.f; a.e.stats = p->stats;
  a.e.bias = p->bias; a.e.act = p->act; a.e.preact = p->preact; a.e.res = p->res; a.e.ldr = p->ldy;
  if (p->stats && (p->bias || p->act || p->res)) return AVSR_E_ARG;
  if (a.M == 0) return 0;
  ConvPlan pl;
  if ((rc = conv_plan(p, AVSR_CONV_FWD, pl))) return rc;
  a.a_bytes = pl.a_bytes; a.b_bytes = pl.b_bytes; a.e.stats_tiles = pl.tiles;
  hipStream_t st = (hipStream_t)stream;
  switch (pl.path) {
    case AVSR_CONV_PATH_REG: return igemm_f32(K_FWD, pl.bm, a, p->groups, st);
    case AVSR_CONV_PATH_PATCH: return patch_launch(K_FWD, a, p, st);
    default: return igemm_glds(K_FWD, pl.bm, a, p->groups, st);
  }
}

extern "C" int avsr_conv_bwd_data(const avsr_conv_params* p, void* stream) {
  if (!p) return AVSR_E_ARG;
  ConvArgs a{};   // every field the call does not set: 0 / null
  int rc = make_geom(p, a.g);
  if (rc) return rc;
  if (!avsr_aligned16(p->dx) || !avsr_aligned16(p->w) || !avsr_aligned16(p->dy)) return AVSR_E_ALIGN;
  a.a = p->dy; a.b = p->w;
  a.a_gstride = p->cout; a.b_gstride = (int64_t)p->cout * p->kh * p->kw * p->cin; a.c_gstride = p->cin;
  a.M = p->nimg * p->hin * p->win; a.N = p->cin; a.K = p->kh * p->kw * p->cout;
  a.splits = 1; a.kchunk = a.K;
  a.e.M = a.M; a.e.N = a.N; a.e.C = p->dx; a.e.ldc = p->ldx; a.e.alpha = p->alpha; a.e.beta = p->beta;
  int kind = K_DGRAD;
  if (p->bnr_h) {
    // BN-backward reduction in the epilogue: bf16 (LDS-DMA / patch kernels), one group, every
    // operand of the epilogue 16-byte aligned with the row stride of dx
    if (p->dtype != AVSR_BF16 || p->groups != 1 || !p->bnr_ws || !p->bnr_scale ||
        !p->bnr_shift || !p->bnr_prelu || !p->bnr_mean || !p->bnr_invstd || (p->bnr_scale2 && !p->bnr_res) ||
        (p->bnr_scale2 && (!p->bnr_shift2 || !p->bnr_mean2 || !p->bnr_invstd2)))
      return AVSR_E_ARG;
    if (!avsr_aligned16(p->bnr_h) || (p->bnr_res && !avsr_aligned16(p->bnr_res))) return AVSR_E_ALIGN;
    a.bnr.h = (const bf16*)p->bnr_h; a.bnr.res = (const bf16*)p->bnr_res;
    a.bnr.scale = p->bnr_scale; a.bnr.shift = p->bnr_shift; a.bnr.prelu = p->bnr_prelu;
    a.bnr.mean = p->bnr_mean; a.bnr.invstd = p->bnr_invstd; a.bnr.scale2 = p->bnr_scale2;
    a.bnr.shift2 = p->bnr_shift2; a.bnr.mean2 = p->bnr_mean2; a.bnr.invstd2 = p->bnr_invstd2; a.bnr.ws = p->bnr_ws;
    kind = K_DGRAD_BNR + (p->bnr_scale2 ? 2 : p->bnr_res ? 1 : 0);
  }
  if (a.M == 0) return 0;
  ConvPlan pl;
  if ((rc = conv_plan(p, AVSR_CONV_DGRAD, pl))) return rc;
  a.a_bytes = pl.a_bytes; a.b_bytes = pl.b_bytes;
  hipStream_t st = (hipStream_t)stream;
  switch (pl.path) {
    case AVSR_CONV_PATH_REG: return igemm_f32(kind, pl.bm, a, p->groups, st);
    case AVSR_CONV_PATH_S2: return s2_launch(kind, a, p, pl, st);
    case AVSR_CONV_PATH_PATCH: return patch_launch(kind, a, p, st);
    default: return igemm_glds(kind, pl.bm, a, p->groups, st);
  }
}

extern "C" int avsr_conv_bwd_weight(const avsr_conv_params* p, void* stream) {
  if (!p) return AVSR_E_ARG;
  ConvArgs a{};   // every field the call does not set: 0 / null
  int rc = make_geom(p, a.g);
  if (rc) return rc;
  if (!avsr_aligned16(p->x) || !avsr_aligned16(p->dy) || !p->dw) return AVSR_E_ALIGN;
  a.a = p->dy; a.b = p->x;
  const int64_t ktot = (int64_t)p->kh * p->kw * p->cin;
  a.a_gstride = p->cout; a.b_gstride = p->cin; a.c_gstride = p->cout * ktot;
  a.M = p->cout; a.N = (int)ktot; a.K = p->nimg * p->hout * p->wout;
  if (a.K == 0) return 0;
  ConvPlan pl;
  if ((rc = conv_plan(p, AVSR_CONV_WGRAD, pl))) return rc;
  hipStream_t st = (hipStream_t)stream;
  if (pl.path == AVSR_CONV_PATH_WPATCH) return wpatch_launch(p, st);
  if (pl.path == AVSR_CONV_PATH_STEM_WPATCH) return stem_wpatch_launch(p, st);
  const WgradPlan& w = pl.w;
  a.a_bytes = pl.a_bytes; a.b_bytes = pl.b_bytes;
  a.splits = w.splits; a.kchunk = w.kchunk;
  a.ws = w.slab ? p->ws : nullptr;
  a.e.M = a.M; a.e.N = a.N; a.e.C = p->dw; a.e.ldc = ktot; a.e.alpha = 1.f;
  if (w.slab) { a.e.ldc = a.N; }                       // plain stores into the slabs
  else if (w.splits == 1) { a.e.beta = 1.f; }          // dw += wgrad, one writer per element
  else { a.e.atomic = 1; }
  rc = pl.path == AVSR_CONV_PATH_REG ? igemm_f32(K_WGRAD, pl.bm, a, p->groups, st) : igemm_glds(K_WGRAD, pl.bm, a, p->groups, st);
  if (rc || !w.slab) return rc;
  const int64_t mn = (int64_t)a.M * a.N;
  const int64_t xb = (int64_t)avsr_grid(mn / 4, 256, 1024) * p->groups;
  int chunks = (int)((65536 / 256 + xb - 1) / xb);
  if (chunks > w.splits) chunks = w.splits;
  if (chunks < 1) chunks = 1;
  return wgrad_reduce(p->ws, w.splits, chunks, mn, p->groups, p->dw, a.c_gstride, st);
}
