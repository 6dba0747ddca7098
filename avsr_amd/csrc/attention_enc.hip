// Fused attention, the encoder's self-attention: the query-tiled forward sq:: (AVSR_ATTN_PATH_SQ)
// and the backward rb:: (AVSR_ATTN_PATH_ENC, further down), which share the DMA and swizzle helpers.
// sq:: forward with K / V going through an LDS-DMA ring (bf16, non-causal, Lq >= 128, any Lk;
// option attn_sq_fwd). One workgroup = 4 waves x 32 rows of its own
// dimension of one (batch, head); grid = B*H x ceil(rows / 128) in XCD-remapped order (the
// blocks of one head adjacent: they share its streamed operands in one L2). 64-row tiles of the
// other dimension go HBM/L2 -> LDS by buffer_load ... lds (no staging registers, no VALU) into
// a 3-stage ring (two tiles in flight), ~48 KiB per workgroup, so three workgroups share a CU
// (12 waves) and one's load / store phases run beside the others' compute (the resident
// kernels hold a whole head, 110 KiB, per CU and serialise load -> compute -> store).
// LDS images are unpadded [64][64] bf16 (128-B rows) whose 16-byte chunk c of row r sits at
// c ^ swz(r), swz(r) = g ^ ((g & 1) << 2), g = (r >> 1) & 7 (applied on the DMA's global side):
// conflict-free for both fragment forms — ds_read_b128 rows on the lanes (every 16-lane bank
// group meets each (row parity, swz) once) and ds_read_b64_tr_b16 transposed reads (rows
// 4m, 4m + 2 land in opposite 64-B halves) — and every lane's fragment offsets are
// loop-invariant (tile base + compile-time row-block offsets).
#include "attention.h"

namespace attn {
namespace sq {
constexpr int KT = 64;                   // rows per streamed tile
constexpr int NS = 3;                    // ring stages
constexpr int IMGB = KT * 128;           // bytes of one [64][64] bf16 image
constexpr int STAGEB = 2 * IMGB;         // two images (K | V)
static_assert(4 * 32 * 65 * 4 <= NS * STAGEB, "store slabs exceed the ring");

typedef __attribute__((address_space(3))) void lds_void_t;

AVSR_DEV int swz(int row) { const int g = (row >> 1) & 7; return g ^ ((g & 1) << 2); }
// base and extent are wave-uniform at every call; readfirstlane states it, so the descriptor
// always lands in SGPRs (the DMA asm requires them)
AVSR_DEV __amdgpu_buffer_rsrc_t rsrc(const void* base, uint32_t bytes) {
  const uint64_t b = (uint64_t)(uintptr_t)base;
  const uint64_t ub = ((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((uint32_t)(b >> 32)) << 32) |
                      (uint32_t)__builtin_amdgcn_readfirstlane((uint32_t)b);
  return __builtin_amdgcn_make_buffer_rsrc((void*)(uintptr_t)ub, (short)0, (int)__builtin_amdgcn_readfirstlane(bytes),
                                           0x00020000);
}
// one wave-instruction: 64 lanes x 16 B (x4: 4 B) -> 1 KiB (256 B) of LDS at lds_wave_base.
// Inline asm as gemm_glds.h bglds16: the compiler's waitcnt pass would otherwise drain the
// ring before each transposed LDS read; the ring is ordered by explicit vmcnt waits + barriers.
AVSR_DEV void dma16(__amdgpu_buffer_rsrc_t r, uint32_t voff, char* lds_wave_base) {
  const uint32_t m = __builtin_amdgcn_readfirstlane((uint32_t)(uintptr_t)(lds_void_t*)lds_wave_base);
  asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tbuffer_load_dwordx4 %1, %2, 0 offen lds" ::"s"(m), "v"(voff), "s"(r)
               : "memory", "m0");
}
AVSR_DEV void dma4(__amdgpu_buffer_rsrc_t r, uint32_t voff, char* lds_wave_base) {
  const uint32_t m = __builtin_amdgcn_readfirstlane((uint32_t)(uintptr_t)(lds_void_t*)lds_wave_base);
  asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tbuffer_load_dword %1, %2, 0 offen lds" ::"s"(m), "v"(voff), "s"(r)
               : "memory", "m0");
}
template <int N> AVSR_DEV void vmwait() { asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory"); }

// per-lane byte offsets of the two fragment forms inside an image
struct FragOff {
  uint32_t row[4];       // b128 fragment, row on the lane: row c (+4096: rows 32..63), d-chunk 2s + hh
  uint32_t tr[2][2];     // transposed fragment of a 16-row block (+ r0 * 128): [d half][second 8 rows]
  AVSR_DEV void init(int l) {
    const int c = l & 31, hh = l >> 5, i = l & 15, gl = (l >> 4) & 1;
#pragma unroll
    for (int s = 0; s < 4; ++s) row[s] = c * 128 + (((2 * s + hh) ^ swz(c)) << 4);
#pragma unroll
    for (int cb = 0; cb < 2; ++cb)
#pragma unroll
      for (int e = 0; e < 2; ++e) {
        const int R = 4 * hh + (i >> 2) + 8 * e, ch = 4 * cb + 2 * gl + ((i & 3) >> 1);
        tr[cb][e] = R * 128 + ((ch ^ swz(R)) << 4) + (i & 1) * 8;
      }
  }
};
AVSR_DEV bf16x8 ldA(const char* img, uint32_t off) { return *(const bf16x8*)(img + off); }
// lane l: X^T[d = 32 cb + (l & 31)][rows r0 + 4hh + {0..3, 8..11}] (see rdT, attention.h)
AVSR_DEV bf16x8 ldT(const char* img, int r0, const FragOff& f, int cb) {
  union { s4v s[2]; bf16x8 x; } u;
  u.s[0] = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s4v*)(img + r0 * 128 + f.tr[cb][0]));
  u.s[1] = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s4v*)(img + r0 * 128 + f.tr[cb][1]));
  return u.x;
}

// the DMA pieces of one tile: wave w moves 8-row pieces 2w, 2w+1 of both images
struct Ring {
  const bf16* s0; const bf16* s1; int64_t ld0, ld1; int n;
  uint32_t o0[2], o1[2];
  static constexpr int DMAS = 4;         // per wave per tile
  AVSR_DEV void init(const bf16* a, int64_t la, const bf16* b, int64_t lb, int n_, int w, int l) {
    s0 = a; s1 = b; ld0 = la; ld1 = lb; n = n_;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int row = 8 * (2 * w + i) + (l >> 3), ch = (l & 7) ^ swz(row);
      o0[i] = (uint32_t)((row * ld0 + ch * 8) * 2);
      o1[i] = (uint32_t)((row * ld1 + ch * 8) * 2);
    }
  }
  // rows of tile t past n lie outside the buffer extent: the DMA writes zeros for them
  AVSR_DEV void issue(char* stage, int t, int w, int l) const {
    const int r0 = t * KT, nr = min(KT, n - r0);
    const __amdgpu_buffer_rsrc_t ra = rsrc(s0 + (int64_t)r0 * ld0, (uint32_t)(((nr - 1) * ld0 + DH) * 2));
    const __amdgpu_buffer_rsrc_t rb = rsrc(s1 + (int64_t)r0 * ld1, (uint32_t)(((nr - 1) * ld1 + DH) * 2));
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      dma16(ra, o0[i], stage + (2 * w + i) * 1024);
      dma16(rb, o1[i], stage + IMGB + (2 * w + i) * 1024);
    }
  }
  // wait until tile t has landed (tile t+1 may still be in flight), then the workgroup barrier
  AVSR_DEV void arrive(int t, int nt, int w) const {
    if (t + 1 < nt) vmwait<DMAS>(); else vmwait<0>();
    __builtin_amdgcn_s_barrier();          // tile t visible; every wave is done with tile t-1
    asm volatile("" ::: "memory");
  }
};

AVSR_DEV int next_stage(int s) { return s + 1 == NS ? 0 : s + 1; }
AVSR_DEV int prev_stage(int s) { return s == 0 ? NS - 1 : s - 1; }

template <bool MASK>
__global__ __launch_bounds__(256, 3) void attn_fwd_kernel(AttnArgs a, int nqb) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int id = xcd_id(blockIdx.x, gridDim.x);
  const int bh = id / nqb, qb = id - bh * nqb, b = bh / a.H, h = bh % a.H;
  const int tid = threadIdx.x, w = __builtin_amdgcn_readfirstlane(tid >> 6), l = tid & 63, c = l & 31, hh = l >> 5;
  const int q0 = qb * 128 + w * 32, qi = q0 + c;
  Ring ring;
  ring.init((const bf16*)a.k + (int64_t)b * a.Lk * a.ldk + h * DH, a.ldk,
            (const bf16*)a.v + (int64_t)b * a.Lk * a.ldv + h * DH, a.ldv, a.Lk, w, l);
  const int klen = a.klen ? min(a.klen[b], a.Lk) : a.Lk;
  const int nt = (klen + KT - 1) / KT;
  // tile 0's DMA, then the Q fragments; the empty asm reading them makes the compiler's own wait
  // for these loads (vmcnt(0), covering tile 0 too) happen here once instead of at their first
  // use inside the tile loop, where it would drain the ring's prefetch every tile
  if (nt > 0) ring.issue(smem, 0, w, l);
  const bf16* Q = (const bf16*)a.q + (int64_t)b * a.Lq * a.ldq + h * DH;
  bf16x8 qf[4];
#pragma unroll
  for (int s = 0; s < 4; ++s) qf[s] = ldrow_sel(Q, a.ldq, qi, a.Lq, s * 16 + 8 * hh);
#pragma unroll
  for (int s = 0; s < 4; ++s) asm volatile("" ::"v"(qf[s]));
  if (nt > 1) ring.issue(smem + STAGEB, 1, w, l);
  FragOff fo;
  fo.init(l);
  const float sl2 = a.scale * LOG2E;
  const AttnDrop drop(a.drop_p, a.seed, a.B, a.H, a.Lq, a.Lk);
  const uint32_t rowG = MASK ? 0u : ((uint32_t)bh * (uint32_t)a.Lq + (uint32_t)min(qi, a.Lq - 1)) * drop.npair * GOLD;
  const int64_t mrow = MASK ? ((int64_t)bh * a.mnqb + (q0 >> 5)) * a.mnkb : 0;
  f32x16 o0, o1;
  zacc(o0); zacc(o1);
  float lsum = 0.f, mb = -INFINITY;          // lazy reference max, as res::attn_fwd_kernel
  int cs = 0;                                // stage of tile t
  for (int t = 0; t < nt; ++t) {
    ring.arrive(t, nt, w);
    if (t + 2 < nt) ring.issue(smem + prev_stage(cs) * STAGEB, t + 2, w, l);
    const char* Ks = smem + cs * STAGEB;
    const char* Vs = Ks + IMGB;
    uint64_t mw[32];
    if (MASK && a.drop_p > 0.f) {
      const smask_t mt = mask_tile(a.mq, mrow + 2 * t);
#pragma unroll
      for (int r = 0; r < 32; ++r) mw[r] = mt[r];
    }
    f32x16 s0, s1;
    zacc(s0); zacc(s1);
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      s0 = mfma32(ldA(Ks, fo.row[s]), qf[s], s0);
      s1 = mfma32(ldA(Ks + 4096, fo.row[s]), qf[s], s1);
    }
    const int k0 = t * KT;
    if (k0 + KT > klen) {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        s0[r] = k0 + qrow(r, hh) < klen ? s0[r] : -INFINITY;
        s1[r] = k0 + 32 + qrow(r, hh) < klen ? s1[r] : -INFINITY;
      }
    }
    // balanced trees (the 16-deep max / add chains were on the tile's dependent path)
    float mx[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) mx[r] = fmaxf(s0[r], s1[r]);
#pragma unroll
    for (int w2 = 8; w2 > 0; w2 >>= 1)
#pragma unroll
      for (int r = 0; r < w2; ++r) mx[r] = fmaxf(mx[r], mx[r + w2]);
    float mt = xor32_max(mx[0]) * sl2;
    const bool grow = mt > mb + 8.f;
    if (__any(grow)) {
      const float alpha = grow ? (mb == -INFINITY ? 0.f : fexp2(mb - mt)) : 1.f;
      mb = grow ? mt : mb;
      lsum *= alpha;
#pragma unroll
      for (int r = 0; r < 16; ++r) { o0[r] *= alpha; o1[r] *= alpha; }
    }
    const float mbu = mb == -INFINITY ? 0.f : mb;
    float ts[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      s0[r] = fexp2(fmaf(s0[r], sl2, -mbu));
      s1[r] = fexp2(fmaf(s1[r], sl2, -mbu));
      ts[r] = s0[r] + s1[r];
    }
#pragma unroll
    for (int w2 = 8; w2 > 0; w2 >>= 1)
#pragma unroll
      for (int r = 0; r < w2; ++r) ts[r] += ts[r + w2];
    lsum += ts[0];
    if (a.drop_p > 0.f) {
      if (MASK) {                            // the stored keep masks of key blocks 2t, 2t + 1
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          s0[r] = msel(s0[r], mw[r]);
          s1[r] = msel(s1[r], mw[16 + r]);
        }
      } else {
        drop_tile_sel(s0, rowG + (uint32_t)(k0 >> 1) * GOLD, drop, hh);
        drop_tile_sel(s1, rowG + (uint32_t)((k0 + 32) >> 1) * GOLD, drop, hh);
      }
    }
    const bf16x8 p0a = accb(s0, 0), p0b = accb(s0, 1), p1a = accb(s1, 0), p1b = accb(s1, 1);
    o0 = mfma32(ldT(Vs, 0, fo, 0), p0a, o0);
    o1 = mfma32(ldT(Vs, 0, fo, 1), p0a, o1);
    o0 = mfma32(ldT(Vs, 16, fo, 0), p0b, o0);
    o1 = mfma32(ldT(Vs, 16, fo, 1), p0b, o1);
    o0 = mfma32(ldT(Vs, 32, fo, 0), p1a, o0);
    o1 = mfma32(ldT(Vs, 32, fo, 1), p1a, o1);
    o0 = mfma32(ldT(Vs, 48, fo, 0), p1b, o0);
    o1 = mfma32(ldT(Vs, 48, fo, 1), p1b, o1);
    cs = next_stage(cs);
  }
  lsum = xor32_sum(lsum);
  if (hh == 0 && qi < a.Lq) a.lse[(int64_t)bh * a.Lq + qi] = lsum > 0.f ? (mb + log2f(lsum)) * LN2 : -INFINITY;
  __syncthreads();                           // the ring is free: reuse it as the store slabs
  const float inv = lsum > 0.f ? (a.drop_p > 0.f ? drop.scale : 1.f) / lsum : 0.f;
  bf16* O = (bf16*)a.o + ((int64_t)b * a.Lq + q0) * a.ldo + h * DH;
  store_t<bf16>(o0, o1, inv, (float*)smem + w * 32 * 65, O, a.ldo, a.Lq - q0);
}

}  // namespace sq

// Encoder backward (bf16, non-causal, 128 <= Lq, Lk <= 384): one 12-wave workgroup per (b, h),
// the streamed operands of the head DMA'd (buffer_load ... lds, no staging registers) into
// unpadded XOR-swizzled [384][64] LDS images in four rounds of 96 rows that are all issued up
// front; the waves start on the first 32-row tiles while the later rounds are in flight. Every
// fragment address is a per-lane FragOff offset plus a tile base (swz(32t + x) = swz(x)).
//   dQ kernel (runs first): K, V images; per wave 32 queries (Q, dO rows in registers), delta =
//     rowsum(dO * O) from this lane's dO / O half-rows, published for the dK / dV kernel.
//   dK / dV kernel: Q, dO images, lse and delta rows, and each wave's own 32-row K image
//     (K fragments re-read per tile instead of held: the register file then holds dK, dV,
//     V and the tile without spilling at 3 waves per SIMD).
// DM: 0 no dropout, 1 hashed per element (AttnDrop), 2 stored keep masks (a.mq).
// These two kernels are the path of option attn_enc_fused = 0; the default is the one fused
// kernel further down (attn_bwd_kernel), which is tested against them.
namespace rb {
using sq::swz; using sq::rsrc; using sq::dma16; using sq::dma4; using sq::vmwait;   // the DMA pieces
using sq::FragOff; using sq::ldA; using sq::ldT;                                    // the swizzled fragments
constexpr int NTH = 768;                 // 12 waves
constexpr int IMG384 = MAXR * 128;       // one swizzled [384][64] bf16 image

// wave w's 8-row piece `piece` of a [n][64] operand (row stride ld) into a swizzled image; rows
// past n lie outside the buffer extent and land as zeros
AVSR_DEV void dma_piece(const bf16* base, int64_t ld, int n, char* img, int piece, int l) {
  const int row = 8 * piece + (l >> 3), ch = (l & 7) ^ swz(row);
  dma16(rsrc(base, (uint32_t)(((n - 1) * ld + DH) * 2)), (uint32_t)((row * ld + ch * 8) * 2), img + piece * 1024);
}
AVSR_DEV void round_barrier() {                    // LDS writes done, no vmcnt drain
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();
  asm volatile("" ::: "memory");
}

template <typename OutT, int DM>
__global__ __launch_bounds__(NTH) void attn_bwd_dq_kernel(AttnArgs a, OutT* dq, int64_t lddq) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* Ks = smem;
  char* Vs = smem + IMG384;
  stamp_part(0, 0);
  const int bh = xcd_id(blockIdx.x, gridDim.x), b = bh / a.H, h = bh % a.H;
  const int tid = threadIdx.x, l = tid & 63, c = l & 31, hh = l >> 5;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int q0 = w * 32, qi = q0 + c;
  const bool qok = qi < a.Lq;
  const bf16* Kg = (const bf16*)a.k + (int64_t)b * a.Lk * a.ldk + h * DH;
  const bf16* Vg = (const bf16*)a.v + (int64_t)b * a.Lk * a.ldv + h * DH;
  dma_piece(Kg, a.ldk, a.Lk, Ks, w, l);                    // round 0
  dma_piece(Vg, a.ldv, a.Lk, Vs, w, l);
  const bf16* Q = (const bf16*)a.q + (int64_t)b * a.Lq * a.ldq + h * DH;
  const bf16* dO = (const bf16*)a.dout + (int64_t)b * a.Lq * a.lddo + h * DH;
  const bf16* Og = (const bf16*)a.o + (int64_t)b * a.Lq * a.ldo + h * DH;
  bf16x8 qf[4], of[4], ov[4];
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    qf[s] = ldrow_sel(Q, a.ldq, qi, a.Lq, s * 16 + 8 * hh);
    of[s] = ldrow_sel(dO, a.lddo, qi, a.Lq, s * 16 + 8 * hh);
    ov[s] = ldrow_sel(Og, a.ldo, qi, a.Lq, s * 16 + 8 * hh);
  }
  const int64_t bhq = (int64_t)bh * a.Lq + min(qi, a.Lq - 1);
  const float lq0 = a.lse[bhq];
  // the compiler's wait for these loads (vmcnt(0), covering round 0) happens here, once
#pragma unroll
  for (int s = 0; s < 4; ++s) asm volatile("" ::"v"(qf[s]), "v"(of[s]), "v"(ov[s]));
  asm volatile("" ::"v"(lq0));
  float dsum = 0.f;
#pragma unroll
  for (int s = 0; s < 4; ++s)
#pragma unroll
    for (int j = 0; j < 8; ++j) dsum = fmaf((float)of[s][j], (float)ov[s][j], dsum);
  dsum = xor32_sum(dsum);
  if (hh == 0 && qok) a.delta[bhq] = dsum;
#pragma unroll
  for (int r = 1; r < 4; ++r) {                           // rounds 1..3 in flight from here on
    dma_piece(Kg, a.ldk, a.Lk, Ks, 12 * r + w, l);
    dma_piece(Vg, a.ldv, a.Lk, Vs, 12 * r + w, l);
  }
  const float lq = qok ? lq0 * LOG2E : 0.f;
  const float dl = qok ? dsum : 0.f;
  const int klen = a.klen ? min(a.klen[b], a.Lk) : a.Lk;
  const int nt = (klen + 31) >> 5;
  const float sl2 = a.scale * LOG2E;
  const AttnDrop drop(a.drop_p, a.seed, a.B, a.H, a.Lq, a.Lk);
  const float dscale = DM ? drop.scale : 1.f;
  const uint32_t rowG = DM == 1 ? ((uint32_t)bh * (uint32_t)a.Lq + (uint32_t)min(qi, a.Lq - 1)) * drop.npair * GOLD : 0u;
  const int64_t mrow = DM == 2 ? ((int64_t)bh * a.mnqb + w) * a.mnkb : 0;
  FragOff fo;
  fo.init(l);
  f32x16 dq0, dq1;
  zacc(dq0); zacc(dq1);
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    if (r == 1) vmwait<4>();
    if (r == 2) vmwait<2>();
    if (r == 3) vmwait<0>();
    round_barrier();                                       // round r of every wave has landed
    if (r == 0) stamp_part(1, 0);
    if (q0 < a.Lq) {
#pragma unroll
      for (int u = 0; u < 3; ++u) {                        // unrolled: tile offsets become immediates
        const int t = 3 * r + u;
        if (t >= nt) break;
        uint64_t mw[16];
        if (DM == 2) {
          const smask_t mt = mask_tile(a.mq, mrow + t);
#pragma unroll
          for (int e = 0; e < 16; ++e) mw[e] = mt[e];
        }
        const char* Kt = Ks + t * 4096;
        const char* Vt = Vs + t * 4096;
        f32x16 st, dpt;
        zacc(st); zacc(dpt);
#pragma unroll
        for (int s = 0; s < 4; ++s) {
          st = mfma32(ldA(Kt, fo.row[s]), qf[s], st);
          dpt = mfma32(ldA(Vt, fo.row[s]), of[s], dpt);
        }
        if (t * 32 + 32 > klen) {                          // wave-uniform: keys past klen
#pragma unroll
          for (int e = 0; e < 16; ++e) st[e] = t * 32 + qrow(e, hh) < klen ? st[e] : -INFINITY;
        }
        // dP' = dropout(dP) (kept x 1/(1-p), dropped 0); the softmax scale of dS goes on dQ at the store
        if (DM == 1) {
#pragma unroll
          for (int e = 0; e < 16; ++e) dpt[e] *= dscale;
          drop_tile_sel(dpt, rowG + (uint32_t)(t * 16) * GOLD, drop, hh);
        }
#pragma unroll
        for (int e = 0; e < 16; ++e) {
          const float p = fexp2(fmaf(st[e], sl2, -lq));
          const float d = DM == 2 ? msel(dpt[e] * dscale, mw[e]) : dpt[e];   // rounding as DM 1
          dpt[e] = p * (d - dl);
        }
        const bf16x8 sa = accb(dpt, 0), sb = accb(dpt, 1);
        dq0 = mfma32(ldT(Ks, 32 * t, fo, 0), sa, dq0);
        dq0 = mfma32(ldT(Ks, 32 * t + 16, fo, 0), sb, dq0);
        dq1 = mfma32(ldT(Ks, 32 * t, fo, 1), sa, dq1);
        dq1 = mfma32(ldT(Ks, 32 * t + 16, fo, 1), sb, dq1);
      }
    }
  }
  stamp_part(2, 0);
  __syncthreads();                                         // images no longer read: store slabs
  if (q0 < a.Lq) {
    OutT* DQ = dq + ((int64_t)b * a.Lq + q0) * lddq + h * DH;
    store_t<OutT>(dq0, dq1, a.scale, (float*)smem + w * 32 * 65, DQ, lddq, a.Lq - q0);
  }
  if (g_stamps != nullptr) {
    __syncthreads();
    stamp_part(3, 0);
  }
}

template <int DM>
__global__ __launch_bounds__(NTH) void attn_bwd_dkdv_kernel(AttnArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* Qs = smem;
  char* dOs = smem + IMG384;
  float* lss = (float*)(smem + 2 * IMG384);                // lse, then lse * log2(e) (0 past Lq)
  float* dls = lss + MAXR;                                 // delta (0 past Lq)
  char* Kw = smem + 2 * IMG384 + 2 * MAXR * 4;             // this wave's [32][64] K image
  stamp_part(0, 1);
  const int bh = xcd_id(blockIdx.x, gridDim.x), b = bh / a.H, h = bh % a.H;
  const int tid = threadIdx.x, l = tid & 63, c = l & 31, hh = l >> 5;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  Kw += w * 4096;
  const int kb0 = w * 32, key = kb0 + c;
  const bf16* Qg = (const bf16*)a.q + (int64_t)b * a.Lq * a.ldq + h * DH;
  const bf16* dOg = (const bf16*)a.dout + (int64_t)b * a.Lq * a.lddo + h * DH;
  const bf16* Kg = (const bf16*)a.k + ((int64_t)b * a.Lk + kb0) * a.ldk + h * DH;
  const bf16* V = (const bf16*)a.v + (int64_t)b * a.Lk * a.ldv + h * DH;
  // this wave's K rows (4 pieces; rows past Lk zero), round 0 of Q / dO, the lse / delta rows
  if (kb0 < a.Lk) {
#pragma unroll
    for (int i = 0; i < 4; ++i) dma_piece(Kg, a.ldk, min(32, a.Lk - kb0), Kw, i, l);
  }
  dma_piece(Qg, a.ldq, a.Lq, Qs, w, l);
  dma_piece(dOg, a.lddo, a.Lq, dOs, w, l);
  {                                                        // 6 x 64 floats of each array
    const float* f = (w < 6 ? a.lse : a.delta) + (int64_t)bh * a.Lq;
    dma4(rsrc(f, (uint32_t)(a.Lq * 4)), (uint32_t)((64 * (w % 6) + l) * 4), (char*)((w < 6 ? lss : dls) + 64 * (w % 6)));
  }
  bf16x8 vf[4];
#pragma unroll
  for (int s = 0; s < 4; ++s) vf[s] = ldrow_sel(V, a.ldv, key, a.Lk, s * 16 + 8 * hh);
#pragma unroll
  for (int s = 0; s < 4; ++s) asm volatile("" ::"v"(vf[s]));    // vmcnt(0) here, covering round 0
#pragma unroll
  for (int r = 1; r < 4; ++r) {
    dma_piece(Qg, a.ldq, a.Lq, Qs, 12 * r + w, l);
    dma_piece(dOg, a.lddo, a.Lq, dOs, 12 * r + w, l);
  }
  round_barrier();
  if (tid < MAXR) lss[tid] *= LOG2E;
  const int klen = a.klen ? min(a.klen[b], a.Lk) : a.Lk;
  const bool active = kb0 < klen, kok = key < klen;
  const float sl2 = a.scale * LOG2E;
  const AttnDrop drop(a.drop_p, a.seed, a.B, a.H, a.Lq, a.Lk);
  const float dscale = DM ? drop.scale : 1.f;
  const uint32_t nG = DM == 1 ? drop.npair * GOLD : 0u;
  const uint32_t keyG = DM == 1 ? ((uint32_t)bh * (uint32_t)a.Lq * drop.npair + (uint32_t)(min(key, a.Lk - 1) >> 1)) * GOLD : 0u;
  const bool odd = c & 1;
  // DM 2: key c of this wave is bit (q & 31) + 32 hh' of lane mask r' of each (query block t, key
  // block w) tile of the query-on-the-lane masks, r' = (c & 3) + 4 (c >> 3), hh' = (c >> 2) & 1:
  // one 8-byte load per lane per tile, the half for this key, shifted to this lane's 4 hh rows
  const uint64_t* mp = DM == 2 ? a.mq + ((int64_t)bh * a.mnqb * a.mnkb + w) * 16 + ((c & 3) + 4 * (c >> 3)) : nullptr;
  const int mstride = a.mnkb * 16;
  const bool mhi = (c >> 2) & 1;
  const int nt = (a.Lq + 31) >> 5;
  FragOff fo;
  fo.init(l);
  f32x16 dv0, dv1, dk0, dk1;
  zacc(dv0); zacc(dv1); zacc(dk0); zacc(dk1);
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    if (r == 1) vmwait<4>();
    if (r == 2) vmwait<2>();
    if (r == 3) vmwait<0>();
    round_barrier();                       // round r landed (r = 0: the lse scaling is visible)
    if (r == 0) stamp_part(1, 1);
    if (active) {
      // the round's 3 query tiles unrolled: tile offsets into the Q / dO images and the lse /
      // delta rows become instruction offsets (no per-fragment address add)
#pragma unroll
      for (int u = 0; u < 3; ++u) {
        const int t = 3 * r + u;
        if (t >= nt) break;
        const int qt0 = t * 32;
        uint32_t mbits = 0;
        if (DM == 2) {
          const uint64_t m64 = mp[(int64_t)t * mstride];
          mbits = (mhi ? (uint32_t)(m64 >> 32) : (uint32_t)m64) >> (4 * hh);
        }
        const char* Qt = Qs + t * 4096;
        const char* dOt = dOs + t * 4096;
        f32x16 sc, dp;
        zacc(sc); zacc(dp);
        // K fragments re-read every tile: an opaque offset keeps the compiler from hoisting them
        // out of the loop into 16 more live registers (an integer, so the pointer stays LDS)
        uint32_t kz = 0;
        asm volatile("" : "+v"(kz));
        const char* Kt = Kw + kz;
#pragma unroll
        for (int s = 0; s < 4; ++s) {
          sc = mfma32(ldA(Qt, fo.row[s]), ldA(Kt, fo.row[s]), sc);
          dp = mfma32(ldA(dOt, fo.row[s]), vf[s], dp);
        }
        if (!(kb0 + 32 <= klen && qt0 + 32 <= a.Lq)) {     // wave-uniform: invalid keys / queries
#pragma unroll
          for (int e = 0; e < 16; ++e) sc[e] = kok & (qt0 + qrow(e, hh) < a.Lq) ? sc[e] : -INFINITY;
        }
        const uint32_t tG = keyG + (uint32_t)(qt0 + 4 * hh) * nG;
#pragma unroll
        for (int i = 0; i < 4; ++i) {                      // registers 4i..4i+3 = queries qt0 + 8i + 4hh + 0..3
          const f32x4 ls = *(const f32x4*)&lss[qt0 + 8 * i + 4 * hh];
          const f32x4 ds = *(const f32x4*)&dls[qt0 + 8 * i + 4 * hh];
          bool kb[4] = {true, true, true, true};
          if (DM == 1) {     // the key pair (2j, 2j+1) on lanes c, c^1 splits the 4 queries' hashes
#pragma unroll
            for (int u = 0; u < 2; ++u) {
              const uint32_t mine = hashG(tG + (uint32_t)(8 * i + (odd ? 2 : 0) + u) * nG, drop.pre);
              const uint32_t other = __shfl_xor(mine, 1, 64);
              const uint32_t h0 = odd ? other : mine, h1 = odd ? mine : other;
              kb[u] = (odd ? (h0 >> 16) : (h0 & 0xFFFFu)) >= drop.thr;
              kb[u + 2] = (odd ? (h1 >> 16) : (h1 & 0xFFFFu)) >= drop.thr;
            }
          }
          // P' = dropout(P) unscaled (1/(1-p) goes on dV at the store), dS = P (dP' - delta)
          // with dP' = dropout(dP) / (1-p); the softmax scale goes on dK at the store
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const int r4 = 4 * i + e;
            const float p = fexp2(fmaf(sc[r4], sl2, -ls[e]));
            if (DM == 2) {
              const bool kp = (mbits >> ((r4 & 3) + 8 * (r4 >> 2))) & 1u;
              sc[r4] = kp ? p : 0.f;
              dp[r4] = p * fmaf(kp ? dp[r4] : 0.f, dscale, -ds[e]);
            } else {
              sc[r4] = kb[e] ? p : 0.f;
              dp[r4] = p * fmaf(kb[e] ? dp[r4] : 0.f, dscale, -ds[e]);
            }
          }
        }
        const bf16x8 pa = accb(sc, 0), pb = accb(sc, 1), sa = accb(dp, 0), sb = accb(dp, 1);
        dv0 = mfma32(ldT(dOs, qt0, fo, 0), pa, dv0);
        dv0 = mfma32(ldT(dOs, qt0 + 16, fo, 0), pb, dv0);
        dv1 = mfma32(ldT(dOs, qt0, fo, 1), pa, dv1);
        dv1 = mfma32(ldT(dOs, qt0 + 16, fo, 1), pb, dv1);
        dk0 = mfma32(ldT(Qs, qt0, fo, 0), sa, dk0);
        dk0 = mfma32(ldT(Qs, qt0 + 16, fo, 0), sb, dk0);
        dk1 = mfma32(ldT(Qs, qt0, fo, 1), sa, dk1);
        dk1 = mfma32(ldT(Qs, qt0 + 16, fo, 1), sb, dk1);
      }
    }
  }
  stamp_part(2, 1);
  __syncthreads();
  if (kb0 < a.Lk) {
    float* scr = (float*)smem + w * 32 * 65;
    bf16* DK = (bf16*)a.dk + ((int64_t)b * a.Lk + kb0) * a.lddk + h * DH;
    store_t<bf16>(dk0, dk1, a.scale, scr, DK, a.lddk, a.Lk - kb0);
    bf16* DV = (bf16*)a.dv + ((int64_t)b * a.Lk + kb0) * a.lddv + h * DH;
    store_t<bf16>(dv0, dv1, dscale, scr, DV, a.lddv, a.Lk - kb0);
  }
  if (g_stamps != nullptr) {
    __syncthreads();
    stamp_part(3, 1);
  }
}

// ---- the fused backward: dQ from the dK / dV pass (option attn_enc_fused) -----------------
// The dK / dV kernel's walk (wave w owns key block w; dK, dV and the V fragments in registers;
// query tiles in order) with three additions. (1) The prologue computes delta for queries
// 32w.. as the dQ kernel does and publishes it in LDS (and in a.delta). (2) Q / dO go through a
// two-slot ring of the 96-row DMA rounds instead of resident images: round r + 2 is issued after
// the barrier that ends round r, round r + 1 lands while r computes. (3) Every active wave
// leaves its bf16 dS tile [key][query] in a double-buffered exchange; after the tile's one
// barrier two rotating waves (one per 32-column half of dh) form dQ_t = sum_w dS[t, w] K_w from
// the exchange and the K image, keys ascending in one accumulator chain, and store it.
// Every wave executes every barrier and every counted wait: those sit outside all conditions on
// w, klen, Lq and `active` (the tile loop always runs its 12 steps).
// LDS (bytes): ring 2 x (Q 12 K | dO 12 K) | K image 48 K | lse, delta 3 K | exchange 2 x 24 K |
// two dQ store slabs [32][33] floats = 155.25 KiB; the dK / dV store slabs reuse it from 0.
constexpr int RROWS = NTH / 64 * 8;                 // rows of one DMA round: an 8-row piece per wave
constexpr int RIMG = RROWS * 128;                   // one operand's image of a round
constexpr int SLOTB = 2 * RIMG;                     // ring slot: Q | dO
constexpr int XTILE = 32 * 64;                      // one wave's dS tile: [32 keys][32 queries] bf16
constexpr int XBUF = NTH / 64 * XTILE;
constexpr int DQSLAB = 32 * 33 * 4;
constexpr int F_K = 2 * SLOTB, F_LSE = F_K + IMG384, F_X = F_LSE + 2 * MAXR * 4, F_ST = F_X + 2 * XBUF;
constexpr size_t FUSED_LDS = F_ST + 2 * DQSLAB;
static_assert(MAXR == 4 * RROWS && RROWS % 32 == 0 && RROWS % 16 == 0, "four rounds of whole tiles, swizzle period 16");
static_assert(FUSED_LDS <= 160 * 1024 && NTH / 64 * 32 * 65 * 4 <= FUSED_LDS, "fused backward LDS");
static_assert(F_X % 16 == 0 && F_ST % 16 == 0, "exchange / slab alignment");

// The ring's DMA: wave w moves the 8-row piece w of each round. The round's rows 96 r .. go into
// the descriptor (base and extent, scalar), so the per-lane offset is the same every round;
// rows past n lie outside the extent and land as zeros (swz(96 r + x) = swz(x))
AVSR_DEV uint32_t round_voff(int64_t ld, int w, int l) {
  const int row = 8 * w + (l >> 3), ch = (l & 7) ^ swz(row);
  return (uint32_t)((row * ld + ch * 8) * 2);
}
AVSR_DEV void dma_round(const bf16* base, int64_t ld, int n, char* img, int r, uint32_t voff, int w) {
  const int nr = n - RROWS * r;
  dma16(rsrc(base + (int64_t)RROWS * r * ld, nr > 0 ? (uint32_t)(((nr - 1) * ld + DH) * 2) : 0u), voff, img + w * 1024);
}

// The exchange tile of a wave: row = key (64 B), 8-byte chunk j = queries 4j..4j+3 at position
// j ^ (key >> 2): the writers (key on the lane, one chunk j each: without the xor keys 4 apart
// would share a bank) spread evenly over the banks, and the transposed readers
// (ds_read_b64_tr_b16) read whole rows, 256 contiguous bytes per half-wave.
AVSR_DEV uint32_t xoff(int key, int j) { return (uint32_t)(key * 64 + ((j ^ ((key >> 2) & 7)) << 3)); }

// dQ_t columns 32 cb .. 32 cb + 31 by one wave: acc[r] = dQ^T[d = 32 cb + qrow(r, hh)][query c]
// (the dQ kernel's form: A = K^T fragments of the image, B = dS with the query on the lane),
// then through the wave's slab to whole 64-byte (bf16) / 128-byte (fp32) row halves of `out`
template <typename OutT>
AVSR_DEV void dq_tile(const char* X, const char* Ks, int nkb, int cb, const FragOff& fo, int l, float scale,
                      float* slab, OutT* out, int64_t ld, int nvalid) {
  // opaque per call: the per-lane offsets below are recomputed for every tile instead of staying
  // live (shared by the 12 unrolled tiles) across the dK / dV register peak
  asm volatile("" : "+v"(l));
  const int c = l & 31, hh = l >> 5, g = (l >> 4) & 1, i = l & 15;
  const uint32_t kt0 = cb ? fo.tr[1][0] : fo.tr[0][0], kt1 = cb ? fo.tr[1][1] : fo.tr[0][1];
  uint32_t xo[2][2];                                   // keys 16 S + 8 e + 4 hh + 0..3, query c
#pragma unroll
  for (int S = 0; S < 2; ++S)
#pragma unroll
    for (int e = 0; e < 2; ++e) xo[S][e] = xoff(16 * S + 8 * e + 4 * hh + (i >> 2), 4 * g + (i & 3));
  f32x16 acc;
  zacc(acc);
  // the fragments of key block kb + 1 are read while block kb multiplies (the last step re-reads
  // its own block: no branch); one chain, so the sum runs over the keys in ascending order
  union Frag { s4v s[2]; bf16x8 x; } ka[2], ds[2];
  auto read = [&](int kb) {
    const char* Kb = Ks + kb * 4096;
    const char* Xb = X + kb * XTILE;
#pragma unroll
    for (int S = 0; S < 2; ++S) {
      ka[S].s[0] = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s4v*)(Kb + S * 2048 + kt0));
      ka[S].s[1] = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s4v*)(Kb + S * 2048 + kt1));
      ds[S].s[0] = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s4v*)(Xb + xo[S][0]));
      ds[S].s[1] = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s4v*)(Xb + xo[S][1]));
    }
  };
  read(0);
  for (int kb = 0; kb < nkb; ++kb) {
    const bf16x8 a0 = ka[0].x, b0 = ds[0].x, a1 = ka[1].x, b1 = ds[1].x;
    read(min(kb + 1, nkb - 1));
    acc = mfma32(a0, b0, acc);
    acc = mfma32(a1, b1, acc);
  }
#pragma unroll
  for (int r = 0; r < 16; ++r) slab[c * 33 + qrow(r, hh)] = acc[r] * scale;
  __builtin_amdgcn_wave_barrier();       // the slab is this wave's own: LDS serves a wave in order
  constexpr int VE = 16 / (int)sizeof(OutT), LPR = 32 / VE, RPI = 64 / LPR;
  const int rr = l / LPR, ch = (l % LPR) * VE;
#pragma unroll
  for (int i0 = 0; i0 < 32; i0 += RPI) {
    const int q = i0 + rr;
    if (q < nvalid) {
      float v[VE];
#pragma unroll
      for (int j = 0; j < VE; ++j) v[j] = slab[q * 33 + ch + j];
      stv(out + (int64_t)q * ld + ch, v);
    }
  }
}

template <typename OutT, int DM>
__global__ __launch_bounds__(NTH) void attn_bwd_kernel(AttnArgs a, OutT* dq, int64_t lddq) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* Ks = smem + F_K;
  float* lss = (float*)(smem + F_LSE);                     // lse, then lse * log2(e) (0 past Lq)
  float* dls = lss + MAXR;                                 // delta (0 past Lq)
  stamp_part(0, 0);
  const int bh = xcd_id(blockIdx.x, gridDim.x), b = bh / a.H, h = bh % a.H;
  const int tid = threadIdx.x, l = tid & 63, c = l & 31, hh = l >> 5;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const char* Kw = Ks + w * 4096;                          // this wave's 32 rows of the K image
  const int kb0 = w * 32, key = kb0 + c;
  const bf16* Qg = (const bf16*)a.q + (int64_t)b * a.Lq * a.ldq + h * DH;
  const bf16* dOg = (const bf16*)a.dout + (int64_t)b * a.Lq * a.lddo + h * DH;
  const bf16* Og = (const bf16*)a.o + (int64_t)b * a.Lq * a.ldo + h * DH;
  const bf16* Kg = (const bf16*)a.k + ((int64_t)b * a.Lk + kb0) * a.ldk + h * DH;
  const bf16* V = (const bf16*)a.v + (int64_t)b * a.Lk * a.ldv + h * DH;
  // this wave's K rows (4 pieces; rows past Lk zero), round 0 of Q / dO, the lse rows
  if (kb0 < a.Lk) {
#pragma unroll
    for (int i = 0; i < 4; ++i) dma_piece(Kg, a.ldk, min(32, a.Lk - kb0), Ks + w * 4096, i, l);
  }
  const uint32_t vq = round_voff(a.ldq, w, l), vdo = round_voff(a.lddo, w, l);
  dma_round(Qg, a.ldq, a.Lq, smem, 0, vq, w);
  dma_round(dOg, a.lddo, a.Lq, smem + RIMG, 0, vdo, w);
  if (w < 6) dma4(rsrc(a.lse + (int64_t)bh * a.Lq, (uint32_t)(a.Lq * 4)), (uint32_t)((64 * w + l) * 4), (char*)(lss + 64 * w));
  // V fragments of this wave's keys; delta of queries 32 w .. from this lane's dO / O half-rows,
  // the dQ kernel's arithmetic (the two paths publish the same bits)
  const int qi = kb0 + c;
  const bool qok = qi < a.Lq;
  bf16x8 vf[4];
  float dsum = 0.f;
  {
    bf16x8 of[4], ov[4];
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      vf[s] = ldrow_sel(V, a.ldv, key, a.Lk, s * 16 + 8 * hh);
      of[s] = ldrow_sel(dOg, a.lddo, qi, a.Lq, s * 16 + 8 * hh);
      ov[s] = ldrow_sel(Og, a.ldo, qi, a.Lq, s * 16 + 8 * hh);
    }
#pragma unroll
    for (int s = 0; s < 4; ++s) asm volatile("" ::"v"(vf[s]), "v"(of[s]), "v"(ov[s]));
    vmwait<0>();                                           // these loads, the K rows, round 0, lse
#pragma unroll
    for (int s = 0; s < 4; ++s)
#pragma unroll
      for (int j = 0; j < 8; ++j) dsum = fmaf((float)of[s][j], (float)ov[s][j], dsum);
  }
  dsum = xor32_sum(dsum);
  if (hh == 0) {
    if (qok) a.delta[(int64_t)bh * a.Lq + qi] = dsum;
    dls[qi] = qok ? dsum : 0.f;
  }
  dma_round(Qg, a.ldq, a.Lq, smem + SLOTB, 1, vq, w);      // round 1 in flight from here on
  dma_round(dOg, a.lddo, a.Lq, smem + SLOTB + RIMG, 1, vdo, w);
  round_barrier();
  if (tid < MAXR) lss[tid] *= LOG2E;
  const int klen = a.klen ? min(a.klen[b], a.Lk) : a.Lk;
  const bool active = kb0 < klen, kok = key < klen;
  const int nkb = (klen + 31) >> 5;                        // key blocks that take part in dQ
  const float sl2 = a.scale * LOG2E;
  const AttnDrop drop(a.drop_p, a.seed, a.B, a.H, a.Lq, a.Lk);
  const float dscale = DM ? drop.scale : 1.f;
  const uint32_t nG = DM == 1 ? drop.npair * GOLD : 0u;
  const uint32_t keyG = DM == 1 ? ((uint32_t)bh * (uint32_t)a.Lq * drop.npair + (uint32_t)(min(key, a.Lk - 1) >> 1)) * GOLD : 0u;
  const bool odd = c & 1;
  // DM 2: as the dK / dV kernel (one 8-byte load per lane per tile, the half for this key)
  const uint64_t* mp = DM == 2 ? a.mq + ((int64_t)bh * a.mnqb * a.mnkb + w) * 16 + ((c & 3) + 4 * (c >> 3)) : nullptr;
  const int mstride = a.mnkb * 16;
  const bool mhi = (c >> 2) & 1;
  const int nt = (a.Lq + 31) >> 5;
  FragOff fo;
  fo.init(l);
  // this lane's chunk 0 (hh: 1) of its key's row in the wave's tile of exchange buffer 0; chunk
  // 2i + hh of the row is this address with bits 4..5 xor i (xoff)
  char* Xw = smem + F_X + w * XTILE;
  const uint32_t xw = xoff(c, hh);
  OutT* DQ = dq + (int64_t)b * a.Lq * lddq + h * DH;
  f32x16 dv0, dv1, dk0, dk1;
  zacc(dv0); zacc(dv1); zacc(dk0); zacc(dk1);
  round_barrier();                                         // the lse scaling is visible
  stamp_part(1, 0);
#pragma unroll
  for (int t = 0; t < MAXR / 32; ++t) {                    // unrolled: slot and tile offsets become immediates
    const int r = t / 3, u = t % 3, qt0 = t * 32;
    const char* Qs = smem + (r & 1) * SLOTB;
    const char* dOs = Qs + RIMG;
    if (active && t < nt) {
      uint32_t mbits = 0;
      if (DM == 2) {
        const uint64_t m64 = mp[(int64_t)t * mstride];
        mbits = (mhi ? (uint32_t)(m64 >> 32) : (uint32_t)m64) >> (4 * hh);
      }
      const char* Qt = Qs + u * 4096;
      const char* dOt = dOs + u * 4096;
      f32x16 sc, dp;
      zacc(sc); zacc(dp);
      // K fragments re-read every tile (see the dK / dV kernel)
      uint32_t kz = 0;
      asm volatile("" : "+v"(kz));
      const char* Kt = Kw + kz;
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        sc = mfma32(ldA(Qt, fo.row[s]), ldA(Kt, fo.row[s]), sc);
        dp = mfma32(ldA(dOt, fo.row[s]), vf[s], dp);
      }
      if (!(kb0 + 32 <= klen && qt0 + 32 <= a.Lq)) {       // wave-uniform: invalid keys / queries
#pragma unroll
        for (int e = 0; e < 16; ++e) sc[e] = kok & (qt0 + qrow(e, hh) < a.Lq) ? sc[e] : -INFINITY;
      }
      const uint32_t tG = keyG + (uint32_t)(qt0 + 4 * hh) * nG;
#pragma unroll
      for (int i = 0; i < 4; ++i) {                        // registers 4i..4i+3 = queries qt0 + 8i + 4hh + 0..3
        const f32x4 ls = *(const f32x4*)&lss[qt0 + 8 * i + 4 * hh];
        const f32x4 ds = *(const f32x4*)&dls[qt0 + 8 * i + 4 * hh];
        bool kb[4] = {true, true, true, true};
        if (DM == 1) {
#pragma unroll
          for (int u2 = 0; u2 < 2; ++u2) {
            const uint32_t mine = hashG(tG + (uint32_t)(8 * i + (odd ? 2 : 0) + u2) * nG, drop.pre);
            const uint32_t other = __shfl_xor(mine, 1, 64);
            const uint32_t h0 = odd ? other : mine, h1 = odd ? mine : other;
            kb[u2] = (odd ? (h0 >> 16) : (h0 & 0xFFFFu)) >= drop.thr;
            kb[u2 + 2] = (odd ? (h1 >> 16) : (h1 & 0xFFFFu)) >= drop.thr;
          }
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int r4 = 4 * i + e;
          const float p = fexp2(fmaf(sc[r4], sl2, -ls[e]));
          if (DM == 2) {
            const bool kp = (mbits >> ((r4 & 3) + 8 * (r4 >> 2))) & 1u;
            sc[r4] = kp ? p : 0.f;
            dp[r4] = p * fmaf(kp ? dp[r4] : 0.f, dscale, -ds[e]);
          } else {
            sc[r4] = kb[e] ? p : 0.f;
            dp[r4] = p * fmaf(kb[e] ? dp[r4] : 0.f, dscale, -ds[e]);
          }
        }
      }
      const bf16x8 pa = accb(sc, 0), pb = accb(sc, 1), sa = accb(dp, 0), sb = accb(dp, 1);
      // dS[queries 4j..4j+3][key c], j = 2i + hh, for the dQ waves
      char* Xt = Xw + (t & 1) * XBUF;
      *(bf16x4*)(Xt + xw) = __builtin_shufflevector(sa, sa, 0, 1, 2, 3);
      *(bf16x4*)(Xt + (xw ^ 16u)) = __builtin_shufflevector(sa, sa, 4, 5, 6, 7);
      *(bf16x4*)(Xt + (xw ^ 32u)) = __builtin_shufflevector(sb, sb, 0, 1, 2, 3);
      *(bf16x4*)(Xt + (xw ^ 48u)) = __builtin_shufflevector(sb, sb, 4, 5, 6, 7);
      dv0 = mfma32(ldT(dOs, 32 * u, fo, 0), pa, dv0);
      dv0 = mfma32(ldT(dOs, 32 * u + 16, fo, 0), pb, dv0);
      dv1 = mfma32(ldT(dOs, 32 * u, fo, 1), pa, dv1);
      dv1 = mfma32(ldT(dOs, 32 * u + 16, fo, 1), pb, dv1);
      dk0 = mfma32(ldT(Qs, 32 * u, fo, 0), sa, dk0);
      dk0 = mfma32(ldT(Qs, 32 * u + 16, fo, 0), sb, dk0);
      dk1 = mfma32(ldT(Qs, 32 * u, fo, 1), sa, dk1);
      dk1 = mfma32(ldT(Qs, 32 * u + 16, fo, 1), sb, dk1);
    }
    if (u == 2) vmwait<0>();               // this wave's pieces of round r + 1 have landed
    round_barrier();                       // tile t's dS is complete; every wave is done with Q / dO tile t
    if (u == 2 && r + 2 < 4) {             // the slot of round r is free
      dma_round(Qg, a.ldq, a.Lq, smem + (r & 1) * SLOTB, r + 2, vq, w);
      dma_round(dOg, a.lddo, a.Lq, smem + (r & 1) * SLOTB + RIMG, r + 2, vdo, w);
    }
    const int cb = w - (2 * t) % (NTH / 64);               // the tile's two dQ waves rotate
    if (t < nt && (cb == 0 || cb == 1))
      dq_tile<OutT>(smem + F_X + (t & 1) * XBUF, Ks, nkb, cb, fo, l, a.scale, (float*)(smem + F_ST + cb * DQSLAB),
                    DQ + (int64_t)qt0 * lddq + 32 * cb, lddq, a.Lq - qt0);
  }
  stamp_part(2, 0);
  __syncthreads();                         // the last dQ waves are done: everything is store slabs now
  {
    float* scr = (float*)smem + w * 32 * 65;
    bf16* DK = (bf16*)a.dk + ((int64_t)b * a.Lk + kb0) * a.lddk + h * DH;
    store_t<bf16>(dk0, dk1, a.scale, scr, DK, a.lddk, a.Lk - kb0);     // waves past Lk: no valid row
    bf16* DV = (bf16*)a.dv + ((int64_t)b * a.Lk + kb0) * a.lddv + h * DH;
    store_t<bf16>(dv0, dv1, dscale, scr, DV, a.lddv, a.Lk - kb0);
  }
  if (g_stamps != nullptr) {
    __syncthreads();
    stamp_part(3, 0);
  }
}

constexpr size_t DQ_LDS = 2 * IMG384 > NTH / 64 * 32 * 65 * 4 ? 2 * IMG384 : NTH / 64 * 32 * 65 * 4;
constexpr size_t DKDV_LDS = 3 * IMG384 + 2 * MAXR * 4;
static_assert(DKDV_LDS <= 160 * 1024 && NTH / 64 * 32 * 65 * 4 <= DKDV_LDS, "dK/dV LDS");

// AVSR_OPT_ATTN_ENC_FUSED = 1: the one-kernel backward; 0: the dQ kernel, then the dK / dV kernel
template <int DM> void launch(const avsr_attn_params* p, const AttnArgs& a, hipStream_t st) {
  const dim3 g(p->B * p->H);
  if (avsr_opt(AVSR_OPT_ATTN_ENC_FUSED) != 0) {
    if (p->dq_out) {
      allow_lds(attn_bwd_kernel<bf16, DM>);
      hipLaunchKernelGGL((attn_bwd_kernel<bf16, DM>), g, dim3(NTH), FUSED_LDS, st, a, (bf16*)p->dq_out, p->lddq_out);
    } else {
      allow_lds(attn_bwd_kernel<float, DM>);
      hipLaunchKernelGGL((attn_bwd_kernel<float, DM>), g, dim3(NTH), FUSED_LDS, st, a, p->dq, p->lddq);
    }
    return;
  }
  if (p->dq_out) {
    allow_lds(attn_bwd_dq_kernel<bf16, DM>);
    hipLaunchKernelGGL((attn_bwd_dq_kernel<bf16, DM>), g, dim3(NTH), DQ_LDS, st, a, (bf16*)p->dq_out, p->lddq_out);
  } else {
    allow_lds(attn_bwd_dq_kernel<float, DM>);
    hipLaunchKernelGGL((attn_bwd_dq_kernel<float, DM>), g, dim3(NTH), DQ_LDS, st, a, p->dq, p->lddq);
  }
  allow_lds(attn_bwd_dkdv_kernel<DM>);
  hipLaunchKernelGGL(attn_bwd_dkdv_kernel<DM>, g, dim3(NTH), DKDV_LDS, st, a);
}
}  // namespace rb

int sq_fwd(const avsr_attn_params* p, const AttnArgs& a, hipStream_t st) {
  const int nqb = (p->Lq + 127) / 128;
  const long nwg = (long)p->B * p->H * nqb;
  if (nwg > 0x7fffffffL) return AVSR_E_SHAPE;
  if (a.mq) hipLaunchKernelGGL(sq::attn_fwd_kernel<true>, dim3((unsigned)nwg), dim3(256), sq::NS * sq::STAGEB, st, a, nqb);
  else hipLaunchKernelGGL(sq::attn_fwd_kernel<false>, dim3((unsigned)nwg), dim3(256), sq::NS * sq::STAGEB, st, a, nqb);
  return (int)hipGetLastError();
}

int enc_bwd(const avsr_attn_params* p, const AttnArgs& a, hipStream_t st) {
  if (!(p->drop_p > 0.f)) rb::launch<0>(p, a, st);
  else if (a.mq) rb::launch<2>(p, a, st);
  else rb::launch<1>(p, a, st);
  return (int)hipGetLastError();
}
int enc_stamps(unsigned long long* buf) { return (int)hipMemcpyToSymbol(HIP_SYMBOL(g_stamps), &buf, sizeof(buf)); }
}  // namespace attn
