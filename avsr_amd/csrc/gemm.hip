// Dense GEMM with fused epilogue (C-ABI avsr_gemm): parameter checks, argument block, path choice,
// and the tiled cores' kernels and launchers (register-staged: gemm_core.h; LDS-DMA tile table:
// gemm_glds.h; ping-pong: gemm_pp.h). The weight-gradient and few-row kernels: gemm_dense.h.
// Replaces every torch.nn.Linear on the AVSR hot path (forward, data-grad, weight-grad);
// see include/avsr_hip.h for the reference call sites.
#include "gemm_dense.h"
#include "gemm_pp.h"
#include <type_traits>
#include <utility>

using namespace gemmd;

namespace {

template <typename T, typename OutT, int WM, int WN, bool AK, bool BK>
__global__ __launch_bounds__(NT) void dense_kernel(DenseArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  using TL = Tile<T, WM, WN, AK, BK>;
  const int z = blockIdx.z, bz = z / a.splits, sp = z % a.splits;
  const int m0 = blockIdx.y * TL::BM, n0 = blockIdx.x * TL::BN;
  using LA = typename std::conditional<AK, LdDenseK<T, TL::BM>, LdDenseR<T, TL::BM>>::type;
  using LB = typename std::conditional<BK, LdDenseK<T, TL::BN>, LdDenseR<T, TL::BN>>::type;
  LA la; la.p = (const T*)a.A + (int64_t)bz * a.sA; la.ld = a.lda; la.rext = a.M; la.K = a.K;
  LB lb; lb.p = (const T*)a.B + (int64_t)bz * a.sB; lb.ld = a.ldb; lb.rext = a.N; lb.K = a.K;
  const int kbeg = sp * a.kchunk, kend = min(a.K, kbeg + a.kchunk);
  f32x16 acc[2][2];
  mainloop<T, WM, WN>(la, lb, m0, n0, kbeg, kend, acc, smem);
  const Epi e = tile_epi<T, OutT, EV_GENERIC>(a, bz, sp);
  epilogue<T, OutT, WM, WN>(e, m0, n0, acc, smem);
}

// bf16 LDS-DMA path (gemm_glds.h): GCfg tiles, 1-D XCD-remapped grid
template <typename OutT, bool AK, bool BK, class CF, int EV = EV_GENERIC>
__global__ __launch_bounds__(CF::NTH, CF::MINB) void dense_glds_kernel(DenseArgs a, int tiles_m, int tiles_n) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  if (a.stamp != nullptr && threadIdx.x == 0) atomicMin(a.stamp, (unsigned long long)__builtin_amdgcn_s_memrealtime());
  const int id = gemmg::xcd_remap(blockIdx.x, gridDim.x);
  int tm, tn, z;
  gemmg::tile_of(id, tiles_m, tiles_n, tm, tn, z);
  const int bz = z / a.splits, sp = z % a.splits;
  const int m0 = tm * CF::BM, n0 = tn * CF::BN;
  const int kbeg = sp * a.kchunk, kend = min(a.K, kbeg + a.kchunk);
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  f32x4 acc[CF::TM][CF::TN];
  const int nk = (kend - kbeg + gemmg::GBK - 1) / gemmg::GBK;
  if (a.a_bytes) {   // buffer-DMA loaders (operands < 2 GiB)
    using LA = typename std::conditional<AK, gemmg::BDenseK<CF::BM, CF::NW>, gemmg::BDenseR<CF::BM, CF::NW>>::type;
    using LB = typename std::conditional<BK, gemmg::BDenseK<CF::BN, CF::NW>, gemmg::BDenseR<CF::BN, CF::NW>>::type;
    LA la; la.init((const bf16*)a.A + (int64_t)bz * a.sA, a.a_bytes, a.lda, m0, a.M, kend, wave, lane);
    LB lb; lb.init((const bf16*)a.B + (int64_t)bz * a.sB, a.b_bytes, a.ldb, n0, a.N, kend, wave, lane);
    gemmg::mainloop_glds<CF>(la, lb, kbeg, nk, acc, smem);
  } else {
    using LA = typename std::conditional<AK, gemmg::GDenseK<CF::BM, CF::NW>, gemmg::GDenseR<CF::BM, CF::NW>>::type;
    using LB = typename std::conditional<BK, gemmg::GDenseK<CF::BN, CF::NW>, gemmg::GDenseR<CF::BN, CF::NW>>::type;
    LA la; la.init((const bf16*)a.A + (int64_t)bz * a.sA, a.lda, m0, a.M, kend, wave, lane);
    LB lb; lb.init((const bf16*)a.B + (int64_t)bz * a.sB, a.ldb, n0, a.N, kend, wave, lane);
    gemmg::mainloop_glds<CF>(la, lb, kbeg, nk, acc, smem);
  }
  const Epi e = tile_epi<bf16, OutT, EV>(a, bz, sp);
  gemmg::epilogue_g<bf16, OutT, CF, EV>(e, m0, n0, acc, smem);
  if (a.stamp != nullptr) {   // uniform: every wave's stores issued before the end stamp
    __syncthreads();
    if (threadIdx.x == 0) atomicMax(a.stamp + 1, (unsigned long long)__builtin_amdgcn_s_memrealtime());
  }
}

// 256x256 ping-pong core (gemm_pp.h)
template <typename OutT, bool AK, bool BK>
__global__ __launch_bounds__(gemmpp::NTH, 1) void dense_pp_kernel(DenseArgs a, int tiles_m, int tiles_n) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int id = gemmg::xcd_remap(blockIdx.x, gridDim.x);
  int tm, tn, z;
  gemmg::tile_of(id, tiles_m, tiles_n, tm, tn, z);
  const int bz = z / a.splits, sp = z % a.splits;
  const int m0 = tm * gemmpp::BM, n0 = tn * gemmpp::BN;
  const int kbeg = sp * a.kchunk, kend = min(a.K, kbeg + a.kchunk);
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  using LA = typename std::conditional<AK, gemmpp::HalfK<64>, gemmpp::HalfR<64>>::type;
  using LB = typename std::conditional<BK, gemmpp::HalfK<32>, gemmpp::HalfR<32>>::type;
  LA la; la.init((const bf16*)a.A + (int64_t)bz * a.sA, a.lda, m0, a.M, kend, wave, lane);
  LB lb; lb.init((const bf16*)a.B + (int64_t)bz * a.sB, a.ldb, n0, a.N, kend, wave, lane);
  f32x4 acc[8][4];
  gemmpp::mainloop_pp(la, lb, kbeg, (kend - kbeg + gemmg::GBK - 1) / gemmg::GBK, acc, smem);
  const Epi e = tile_epi<bf16, OutT, EV_GENERIC>(a, bz, sp);
  gemmg::epilogue_g<bf16, OutT, gemmpp::CF>(e, m0, n0, acc, smem);
}

template <typename OutT, bool AK, bool BK>
int launch_pp(const DenseArgs& a, int batch, hipStream_t st) {
  const int tm = (a.M + 255) / 256, tn = (a.N + 255) / 256;
  const long nwg = (long)tm * tn * batch * a.splits;
  if (nwg > 0x7fffffffL) return AVSR_E_SHAPE;
  hipLaunchKernelGGL((dense_pp_kernel<OutT, AK, BK>), dim3((unsigned)nwg), dim3(gemmpp::NTH), gemmpp::LDS_BYTES, st, a,
                     tm, tn);
  AVSR_CHECK_LAUNCH();
  return 0;
}

// The compile-time epilogue variant a launch qualifies for (gemm_core.h EV_*), or EV_GENERIC.
// A variant puts every vector of every tile on the 8-column path, so the host check covers what
// epi_vec_ok tests in the kernel with the batch / split offsets applied.
template <typename OutT>
int epi_variant(const DenseArgs& a, int batch) {
  const Epi& e = a.e;
  if (e.atomic || e.stats || e.rm_wc || e.alpha != 1.f || e.beta != 0.f || (e.N % 8)) return EV_GENERIC;
  const uintptr_t ptrs = (uintptr_t)e.C | (uintptr_t)e.preact | (uintptr_t)e.res | (uintptr_t)e.gate | (uintptr_t)e.bias;
  if (ptrs & 15u) return EV_GENERIC;
  const int64_t so = (int64_t)sizeof(OutT);
  if (((e.ldc * so) | (e.ldc * 2) | (e.ldr * 2)) & 15) return EV_GENERIC;
  if (batch > 1 && (((a.sC * so) | (a.sC * 2) | (a.sR * 2)) & 15)) return EV_GENERIC;
  if (a.splits > 1 && ((a.sSplit * so) & 15)) return EV_GENERIC;
  const bool drop = e.drop_p > 0.f;
  if (!e.bwd) {
    if (e.gate || e.colsum) return EV_GENERIC;
    if (!e.bias) return (!e.preact && !e.act && !e.res && !drop) ? EV_PLAIN : EV_GENERIC;
    if (!e.preact && !e.act && !e.res && !drop) return EV_BIAS;
    if (!e.preact && !e.act && e.res) return EV_BIAS_RES;
    if (e.preact && e.act == AVSR_ACT_GELU && !e.res) return EV_BIAS_ACT_PRE;
    return EV_GENERIC;
  }
  if (e.bias || e.preact || e.res) return EV_GENERIC;
  if (e.gate && e.act == AVSR_ACT_GELU) return EV_GATE;
  if (!e.gate && !e.act && !drop && !e.colsum) return EV_PLAIN;
  return EV_GENERIC;
}

// Variants are instantiated where the encoder's GEMMs run them: bf16 output, the forward ones
// on the forward layout (B k-major), the backward ones on the data-grad layout (B r-contiguous);
// every other combination runs the generic epilogue.
template <typename OutT, bool BK, int EV>
constexpr bool ev_built() {
  if (EV == EV_GENERIC) return true;
  if (sizeof(OutT) != 2) return false;
  return BK ? (EV == EV_BIAS || EV == EV_BIAS_RES || EV == EV_BIAS_ACT_PRE) : (EV == EV_PLAIN || EV == EV_GATE);
}

template <typename OutT, bool AK, bool BK, class CF, int EV>
int launch_glds_ev(const DenseArgs& a, int tm, int tn, long nwg, hipStream_t st) {
  if constexpr (!ev_built<OutT, BK, EV>()) {
    return launch_glds_ev<OutT, AK, BK, CF, EV_GENERIC>(a, tm, tn, nwg, st);
  } else {
    hipLaunchKernelGGL((dense_glds_kernel<OutT, AK, BK, CF, EV>), dim3((unsigned)nwg), dim3(CF::NTH), CF::LDS_BYTES,
                       st, a, tm, tn);
    AVSR_CHECK_LAUNCH();
    return 0;
  }
}

// VARIANTS: the configuration carries the compile-time epilogue variants (each costs build time)
template <typename OutT, bool AK, bool BK, class CF, bool VARIANTS = false>
int launch_glds(const DenseArgs& a, int batch, hipStream_t st) {
  const int tm = (a.M + CF::BM - 1) / CF::BM, tn = (a.N + CF::BN - 1) / CF::BN;
  const long nwg = (long)tm * tn * batch * a.splits;
  if (nwg > 0x7fffffffL) return AVSR_E_SHAPE;
  if constexpr (VARIANTS) {
    switch (epi_variant<OutT>(a, batch)) {
      case EV_PLAIN: return launch_glds_ev<OutT, AK, BK, CF, EV_PLAIN>(a, tm, tn, nwg, st);
      case EV_BIAS: return launch_glds_ev<OutT, AK, BK, CF, EV_BIAS>(a, tm, tn, nwg, st);
      case EV_BIAS_RES: return launch_glds_ev<OutT, AK, BK, CF, EV_BIAS_RES>(a, tm, tn, nwg, st);
      case EV_BIAS_ACT_PRE: return launch_glds_ev<OutT, AK, BK, CF, EV_BIAS_ACT_PRE>(a, tm, tn, nwg, st);
      case EV_GATE: return launch_glds_ev<OutT, AK, BK, CF, EV_GATE>(a, tm, tn, nwg, st);
      default: break;
    }
  }
  return launch_glds_ev<OutT, AK, BK, CF, EV_GENERIC>(a, tm, tn, nwg, st);
}

using Cfg128 = gemmg::GCfg<2, 2, 2, 2, 2>;       // 128x128, 4 waves, 2 stages, 2 blocks/CU
using Cfg256 = gemmg::GCfg<2, 4, 4, 2, 2>;       // 256x256, 8 waves, 2 stages (128 KiB)
using Cfg256x128 = gemmg::GCfg<4, 2, 2, 2, 3>;   // 256x128, 8 waves, 3 stages (144 KiB)
using Cfg128x256 = gemmg::GCfg<2, 4, 2, 2, 3>;   // 128x256, 8 waves, 3 stages
using Cfg128s3 = gemmg::GCfg<2, 2, 2, 2, 3>;     // 128x128, 4 waves, 3 stages (96 KiB)
using Cfg128w8s3 = gemmg::GCfg<2, 4, 2, 1, 3>;   // 128x128, 8 waves (64x32 each), 3 stages
using Cfg192 = gemmg::GCfg<2, 2, 3, 2, 2>;       // 192x128, 4 waves (96x64 each), 2 stages (80 KiB), 2 blocks/CU
using Cfg192x256 = gemmg::GCfg<2, 4, 3, 2, 2>;   // 192x256, 8 waves (96x64 each), 2 stages (112 KiB)
using Cfg192w8s3 = gemmg::GCfg<2, 4, 3, 1, 3>;   // 192x128, 8 waves (96x32 each), 3 stages (120 KiB)
using Cfg64 = gemmg::GCfg<2, 2, 1, 1, 2>;        // 64x64, 4 waves (32x32 each), 2 stages (32 KiB)
using Cfg64s4 = gemmg::GCfg<2, 2, 1, 1, 4>;      // 64x64, 4 stages (64 KiB: 3 K-tiles in flight)
struct CorePP { static constexpr int BM = gemmpp::BM; };   // the 256x256 ping-pong core (launch_pp)

// One row of the tile table: the AVSR_TILE_* id, the configuration when A is k-major, and whether
// it carries the compile-time epilogue variants. With A r-contiguous the row runs it only if
// GDenseR can build its A image (a 64-lane DMA piece = whole k rows of BM / 8 vectors: BM = 64,
// 128, 256), else plain Cfg128 (weight-grads under a forced 192-row tile stay on 128x128).
template <int ID_, class CF_, bool VARIANTS_ = false>
struct TileRow {
  static constexpr int ID = ID_;
  static constexpr bool R_OK = 512 % CF_::BM == 0;
  template <bool AK> using CF = std::conditional_t<AK || R_OK, CF_, Cfg128>;
  static constexpr int bm(bool ak) { return ak ? CF<true>::BM : CF<false>::BM; }   // row-tile height
  template <typename OutT, bool AK, bool BK>
  static int launch(const DenseArgs& a, int batch, hipStream_t st) {
    if constexpr (std::is_same_v<CF<AK>, CorePP>) return launch_pp<OutT, AK, BK>(a, batch, st);
    else return launch_glds<OutT, AK, BK, CF<AK>, VARIANTS_ && (AK || R_OK)>(a, batch, st);
  }
};
template <class... R> struct TileTable { static constexpr int COUNT = sizeof...(R); };

// The tile configurations, in id order (include/avsr_hip.h AVSR_TILE_*, avsr_amd/_lib.py TILES).
// tile_cfg chooses 128, 192, 192w8s3, 64 and 64s4; the others run only when forced (the tests'
// coverage of GCfg's generality). Variants on the encoder's two 192-row tiles, where its GEMM time is.
using Tiles = TileTable<
    TileRow<AVSR_TILE_128, Cfg128>,
    TileRow<AVSR_TILE_256, Cfg256>,
    TileRow<AVSR_TILE_256x128, Cfg256x128>,
    TileRow<AVSR_TILE_128x256, Cfg128x256>,
    TileRow<AVSR_TILE_128s3, Cfg128s3>,
    TileRow<AVSR_TILE_128w8s3, Cfg128w8s3>,
    TileRow<AVSR_TILE_PP, CorePP>,
    TileRow<AVSR_TILE_192, Cfg192, true>,
    TileRow<AVSR_TILE_192x256, Cfg192x256>,
    TileRow<AVSR_TILE_192w8s3, Cfg192w8s3, true>,
    TileRow<AVSR_TILE_64, Cfg64>,
    TileRow<AVSR_TILE_64s4, Cfg64s4>>;

template <class... R, int... I>
constexpr bool rows_in_id_order(TileTable<R...>, std::integer_sequence<int, I...>) {
  return ((R::ID == I) && ...);
}
static_assert(Tiles::COUNT == AVSR_TILE_COUNT, "one table row per AVSR_TILE_* id");
static_assert(rows_in_id_order(Tiles{}, std::make_integer_sequence<int, Tiles::COUNT>{}), "row k is AVSR_TILE_* id k");

// cfg is an id of the table (avsr_set_option range-checks a forced one)
template <class... R>
int cfg_bm(TileTable<R...>, int cfg, bool ak) {
  int bm = 0;
  (void)((cfg == R::ID && ((bm = R::bm(ak)), true)) || ...);
  return bm;
}

template <typename OutT, bool AK, bool BK, class... R>
int launch_cfg(TileTable<R...>, int cfg, const DenseArgs& a, int batch, hipStream_t st) {
  int rc = AVSR_E_ARG;
  (void)((cfg == R::ID && ((rc = R::template launch<OutT, AK, BK>(a, batch, st)), true)) || ...);
  return rc;
}

// tile choice: AVSR_OPT_GEMM_TILE = k + 1 forces configuration k (AVSR_TILE_*, benchmarks);
// otherwise the configuration with the fewest block rounds x per-tile work (wave quantisation
// over 256 CUs)
#ifndef AVSR_AB_FWD2      // A/B builds only (tools/build_variant.py): tile of the multi-round shapes
#define AVSR_AB_FWD2 AVSR_TILE_192
#endif
#ifndef AVSR_AB_ROUND1    // ... and of the one-round (N = 1024) shapes
#define AVSR_AB_ROUND1 AVSR_TILE_192w8s3
#endif
int tile_cfg(const avsr_gemm_params* p, int splits) {
  const int forced = (int)avsr_opt(AVSR_OPT_GEMM_TILE) - 1;
  if (forced >= 0) return forced;
  const long tiles_z = (long)p->batch * splits;
  const long t128 = (long)((p->M + 127) / 128) * ((p->N + 127) / 128) * tiles_z;
  // 128x128 at two blocks per CU is the default (tools/gemm_table.py, profiles/r02_gemm_table.*:
  // the 256x256 ping-pong core loses 8-36 % at M = 6000, the 3-stage / 8-wave variants are
  // slower). The 192x128 tile (96x64 per wave: 48 MFMAs per 20 fragment reads and 10 DMAs
  // instead of 32 per 16 and 8) wins where it still runs >= 2 blocks per CU and its rounds
  // carry no more work than 128x128's: the M = 6000 encoder GEMMs with N >= 3072 (QKV / FFN1
  // fwd, FFN2 dgrad: -7..-15 %, profiles/r02_gemm_table192.txt). With one block per CU
  // (N = 1024) it loses 4-18 %. k-major A only (TileRow: r-contiguous A runs Cfg128 there).
  if (p->a_kmajor) {
    const long t192 = (long)((p->M + 191) / 192) * ((p->N + 127) / 128) * tiles_z;
    const long n128 = (t128 + 255) / 256, n192 = (t192 + 255) / 256;   // blocks on the busiest CU
    if (n192 >= 2 && 3 * n192 * 50 <= 2 * n128 * 51) return AVSR_AB_FWD2;      // 1.5 n192 <= 1.02 n128
    // one round of 192-row tiles that fills at least half the chip (the M = 6000, N = 1024
    // encoder GEMMs: 256 tiles): one block per CU, so 8 waves (two per SIMD, one's MFMAs cover
    // the other's LDS-DMA issue) and 3 stages: -10..-15 % vs 128x128 (profiles/r03_gemm_table_192w8.txt)
    if (t192 > 128 && t192 <= 256) return AVSR_AB_ROUND1;
  }
  // grids of fewer 128x128 tiles than CUs (the teacher-forced decoder: M = 16 x 41 rows, N = 1024:
  // 48 tiles) leave most of the chip idle: 64x64 tiles (4x the workgroups, several per CU).
  // With at most one 64x64 block per CU and a long K (>= 32 K-tiles) the K loop is DMA-latency
  // bound: 4 stages keep 3 K-tiles in flight (decoder K = 3072 / 5056 GEMMs 26 -> 20 us,
  // 41 -> 30 us; with 2+ blocks per CU or K = 1024 the 2-stage tile stays ahead,
  // profiles/r05_dec_gemm_stages.txt)
  const long t64 = (long)((p->M + 63) / 64) * ((p->N + 63) / 64) * tiles_z;
  if (t128 < 256 && t64 >= 2 * t128) return (t64 <= 256 && p->K >= 2048) ? AVSR_TILE_64s4 : AVSR_TILE_64;
  return AVSR_TILE_128;
}

template <typename OutT>
int glds_by_layout(const avsr_gemm_params* p, int cfg, const DenseArgs& a, hipStream_t st) {
  if (p->a_kmajor && p->b_kmajor) return launch_cfg<OutT, true, true>(Tiles{}, cfg, a, p->batch, st);
  if (p->a_kmajor) return launch_cfg<OutT, true, false>(Tiles{}, cfg, a, p->batch, st);
  if (p->b_kmajor) return launch_cfg<OutT, false, true>(Tiles{}, cfg, a, p->batch, st);
  return launch_cfg<OutT, false, false>(Tiles{}, cfg, a, p->batch, st);
}

template <typename T, typename OutT, int WM, int WN, bool AK, bool BK>
int launch(const DenseArgs& a, int batch, hipStream_t st) {
  using TL = Tile<T, WM, WN, AK, BK>;
  dim3 grid((a.N + TL::BN - 1) / TL::BN, (a.M + TL::BM - 1) / TL::BM, batch * a.splits);
  hipLaunchKernelGGL((dense_kernel<T, OutT, WM, WN, AK, BK>), grid, dim3(NT), TL::LDS_BYTES, st, a);
  AVSR_CHECK_LAUNCH();
  return 0;
}

template <typename T, typename OutT, int WM, int WN>
int by_layout(const avsr_gemm_params* p, const DenseArgs& a, hipStream_t st) {
  if (p->a_kmajor && p->b_kmajor) return launch<T, OutT, WM, WN, true, true>(a, p->batch, st);
  if (p->a_kmajor) return launch<T, OutT, WM, WN, true, false>(a, p->batch, st);
  if (p->b_kmajor) return launch<T, OutT, WM, WN, false, true>(a, p->batch, st);
  return launch<T, OutT, WM, WN, false, false>(a, p->batch, st);
}

template <typename T, typename OutT>
int by_tile(const avsr_gemm_params* p, const DenseArgs& a, hipStream_t st) {
  if (p->N <= 64) return by_layout<T, OutT, 4, 1>(p, a, st);
  if (p->M <= 64) return by_layout<T, OutT, 1, 4>(p, a, st);
  return by_layout<T, OutT, 2, 2>(p, a, st);
}

// Everything avsr_gemm rejects, in a fixed order (0: the call runs). glds: glds_ok(p); slab: the
// split partials go to p->ws.
int check_params(const avsr_gemm_params* p, int splits, bool slab, bool glds) {
  if (p->M < 0 || p->N < 0 || p->K < 0 || p->batch <= 0) return AVSR_E_SHAPE;
  if (p->dtype != AVSR_F32 && p->dtype != AVSR_BF16) return AVSR_E_DTYPE;
  const int ve = p->dtype == AVSR_BF16 ? 8 : 4;
  if (!avsr_aligned16(p->A) || !avsr_aligned16(p->B)) return AVSR_E_ALIGN;
  if (p->lda % ve || p->ldb % ve || p->strideA % ve || p->strideB % ve) return AVSR_E_ALIGN;
  if ((p->a_kmajor || p->b_kmajor) && (p->K % ve)) return AVSR_E_ALIGN;
  if (splits > 1 && !(p->c_f32 || p->dtype == AVSR_F32)) return AVSR_E_ARG;
  if (slab && (p->bias || p->act || p->preact || p->res || p->gate || p->drop_p > 0.f || p->epi_bwd || (p->N % 4) ||
               (p->ldc % 4) || (p->strideC % 4) || !avsr_aligned16(p->C)))
    return AVSR_E_ARG;
  const bool skinny = !glds && !slab && skinny_ok(p, splits);
  if (p->kv_k && (p->dtype != AVSR_F32 || p->M > 64 || splits > 1 || (p->N % 3) || !p->kv_v || !p->kv_pos ||
                  p->kv_rows < p->M || p->kv_pos_stride < 0))
    return AVSR_E_ARG;
  if (p->kv_k && !skinny) return AVSR_E_ARG;
  if (p->ln_c1 && (p->dtype != AVSR_F32 || p->M > 64 || splits > 1)) return AVSR_E_ARG;
  // fused bias gradient: the LDS-DMA bf16 path's vector epilogue, one K pass
  if (p->db && (!glds || p->dtype != AVSR_BF16 || p->c_f32 || splits > 1 || p->batch != 1 || !p->db_ws || (p->N % 8) ||
                (p->ldc % 8) || (p->ldr % 8) || !avsr_aligned16(p->C) || (p->gate && !avsr_aligned16(p->gate)) ||
                (p->preact && !avsr_aligned16(p->preact)) || (p->res && (!avsr_aligned16(p->res) || (p->ldr % 8))) ||
                (p->bias && !avsr_aligned16(p->bias))))
    return AVSR_E_ARG;
  if (p->K == 0) return AVSR_E_SHAPE;
  if (p->ln_c1 && !skinny) return AVSR_E_ARG;   // the prologue is the few-row kernel's
  return 0;
}

}  // namespace

// the LDS-DMA path needs whole 16-byte vectors along every operand's contiguous dimension
bool gemmd::glds_ok(const avsr_gemm_params* p) {
  return p->dtype == AVSR_BF16 && p->M >= 128 && p->N >= 128 && (p->a_kmajor || p->M % 8 == 0) &&
         (p->b_kmajor || p->N % 8 == 0);
}

DenseArgs gemmd::dense_args(const avsr_gemm_params* p, int splits, bool slab) {
  DenseArgs a{};
  a.M = p->M; a.N = p->N; a.K = p->K;
  a.splits = splits;
  const int kq = glds_ok(p) ? gemmg::GBK : BKE;
  a.kchunk = ((p->K + splits - 1) / splits + kq - 1) / kq * kq;
  a.A = p->A; a.lda = p->lda; a.sA = p->strideA;
  a.B = p->B; a.ldb = p->ldb; a.sB = p->strideB;
  {   // operand extents in bytes (last element touched + 1) for the buffer-DMA loaders
    const int esz = p->dtype == AVSR_BF16 ? 2 : 4;
    const int64_t ea = (p->a_kmajor ? ((int64_t)(p->M - 1) * p->lda + p->K) : ((int64_t)(p->K - 1) * p->lda + p->M)) * esz;
    const int64_t eb = (p->b_kmajor ? ((int64_t)(p->N - 1) * p->ldb + p->K) : ((int64_t)(p->K - 1) * p->ldb + p->N)) * esz;
    const int64_t lim = (int64_t)gemmg::OOB - (1 << 20);
    const bool ok = ea > 0 && eb > 0 && ea < lim && eb < lim;
    a.a_bytes = ok ? (uint32_t)ea : 0u;
    a.b_bytes = ok ? (uint32_t)eb : 0u;
  }
  a.sC = p->strideC; a.sR = p->strideR;
  a.stamp = p->stamp;
  a.falpha = 1.f;
  a.ln_c1 = p->ln_c1; a.ln_eps = p->ln_eps;
  a.kvk = (float*)p->kv_k; a.kvv = (float*)p->kv_v; a.kvpos = p->kv_pos; a.kvrows = p->kv_rows; a.kvposs = p->kv_pos_stride;
  Epi& e = a.e;   // (the fields the conv epilogues use stay zero)
  e.M = p->M; e.N = p->N; e.C = p->C; e.ldc = p->ldc;
  e.alpha = p->alpha; e.beta = p->beta; e.bias = p->bias;
  e.act = p->act; e.bwd = p->epi_bwd; e.atomic = splits > 1 && !slab;
  if (slab) {   // partial tiles -> ws[b][split][M][N], reduced by the caller's tail
    e.C = p->ws; e.ldc = p->N; e.alpha = 1.f; e.beta = 0.f;
    a.sSplit = (int64_t)p->M * p->N + AVSR_GEMM_SLAB_PAD; a.sC = (int64_t)splits * a.sSplit;
  }
  e.preact = p->preact; e.res = p->res; e.ldr = p->ldr; e.gate = p->gate;
  e.drop_p = p->drop_p; e.seed = p->seed;
  e.colsum = p->db ? p->db_ws : nullptr;
  return a;
}

extern "C" int avsr_gemm(const avsr_gemm_params* p, void* stream) {
  if (!p) return AVSR_E_ARG;
  if (p->M == 0 || p->N == 0) return 0;
  const int splits = p->splitk > 1 ? p->splitk : 1;
  const bool slab = splits > 1 && p->ws != nullptr;
  const bool glds = glds_ok(p);
  int rc = check_params(p, splits, slab, glds);
  if (rc) return rc;
  const DenseArgs a = dense_args(p, splits, slab);
  hipStream_t st = (hipStream_t)stream;
  int colsum_bm = 0;
  if (!glds && !slab && skinny_ok(p, splits)) return skinny_launch(p, a, st);
  if (glds && wgrad_dual_ok(p, splits, slab)) {
    bool reduced;
    rc = wgrad_dual_launch(p, a, st, &reduced);
    if (reduced) return rc;
  } else if (glds) {
    const int cfg = tile_cfg(p, splits);
    rc = p->c_f32 ? glds_by_layout<float>(p, cfg, a, st) : glds_by_layout<bf16>(p, cfg, a, st);
    if (p->db) colsum_bm = cfg_bm(Tiles{}, cfg, p->a_kmajor != 0);
  } else if (p->dtype == AVSR_F32) rc = by_tile<float, float>(p, a, st);
  else if (p->c_f32) rc = by_tile<bf16, float>(p, a, st);
  else rc = by_tile<bf16, bf16>(p, a, st);
  if (rc) return rc;
  if (colsum_bm) {
    const int tiles = (p->M + colsum_bm - 1) / colsum_bm;
    rc = colsum_launch((const float*)p->db_ws, tiles, (int64_t)p->N, p->N, p->db, 0, nullptr, st);
    if (rc) return rc;
  }
  if (!slab) return 0;
  const int64_t per = (int64_t)p->M * (p->N / 4);
  if (per >= (1ll << 31)) return AVSR_E_SHAPE;
  const dim3 g((unsigned)avsr_grid(per, 256, 4096), p->batch);
  hipLaunchKernelGGL(slab_reduce_kernel, g, dim3(256), 0, st, (const float*)p->ws, splits, p->M, p->N,
                     (int64_t)p->M * p->N + AVSR_GEMM_SLAB_PAD, (float*)p->C, p->ldc, p->strideC, p->alpha, p->beta);
  AVSR_CHECK_LAUNCH();
  return 0;
}

