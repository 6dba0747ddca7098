// What the translation units of fused attention (attention.hip and attention_*.hip) share: the
// kernel argument block, the dropout function, the fragment / mask / stamp helpers that more than
// one kernel family uses, and the per-family launchers that attention.hip dispatches to.
#pragma once
#include "common.h"
#include <algorithm>
#include <type_traits>

namespace attn {
constexpr int DH = 64;
constexpr float LOG2E = 1.4426950408889634f;
constexpr float LN2 = 0.6931471805599453f;
constexpr int MAXR = 384;           // resident rows per (b, h): the resident and encoder-backward kernels
constexpr uint32_t GOLD = 0x9E3779B1u;   // AttnDrop's index premultiplier (hashG callers)

// accumulator register r of lane half hh -> row of the 32 x 32 tile (every kernel)
AVSR_DEV int qrow(int r, int hh) { return (r & 3) + 8 * (r >> 2) + 4 * hh; }
AVSR_DEV void zacc(f32x16& x) {
#pragma unroll
  for (int r = 0; r < 16; ++r) x[r] = 0.f;
}

// ---- attention-probability dropout ------------------------------------------------------
// One 32-bit hash per (query, key pair) supplies the 16-bit uniforms of both keys of the pair
// (half the hash work of a per-element stream; the hash, two multiply-xorshift rounds, is the
// VALU-dominant cost of the attention kernels). Key k of query q of head (b, h) reads pair
//   g = ((b*H + h) * Lq + q) * ceil(Lk / 2) + k / 2,  u = (k odd ? hi : lo) 16 bits of hash(g),
// dropped iff u < thr = round(p * 65536) (p_eff within 8e-6 of p), kept values scaled by
// 65536 / (65536 - thr) so that E[mask] = 1 exactly. Every attention kernel (forward, dK/dV,
// dQ; bf16 and fp32) evaluates this same function: masks are recomputed, never stored.
struct AttnDrop {
  uint64_t seed; uint32_t pre, thr, npair; float scale; bool small;
  AVSR_DEV AttnDrop(float p, uint64_t seed_, int B, int H, int Lq, int Lk) {
    seed = seed_;
    thr = (uint32_t)(p * 65536.f + 0.5f);
    scale = thr < 65536u ? 65536.f / (float)(65536u - thr) : 0.f;
    npair = (uint32_t)((Lk + 1) >> 1);
    small = (uint64_t)B * H * Lq * npair <= 0xFFFFFFFFull;
    pre = mix32_hi(seed, 0u);
  }
  AVSR_DEV uint64_t index(int bh, int Lq, int q, int k) const {
    return ((uint64_t)bh * Lq + q) * npair + (uint32_t)(k >> 1);
  }
  AVSR_DEV uint32_t hash(uint64_t g) const { return small ? mix32_lo(pre, (uint32_t)g) : mix32(seed, g); }
  AVSR_DEV float keep(uint32_t h, int k) const {
    const uint32_t u = (k & 1) ? (h >> 16) : (h & 0xFFFFu);
    return u >= thr ? scale : 0.f;
  }
  AVSR_DEV float at(int bh, int Lq, int q, int k) const { return keep(hash(index(bh, Lq, q, k)), k); }
};

struct AttnArgs {
  int B, H, Lq, Lk; float scale;
  const void* q; int64_t ldq; const void* k; int64_t ldk; const void* v; int64_t ldv;
  void* o; int64_t ldo; float* lse; const int* klen; int causal; float drop_p; uint64_t seed;
  const void* dout; int64_t lddo; float* delta; float* dq; int64_t lddq;
  void* dk; int64_t lddk; void* dv; int64_t lddv;
  const uint64_t* mq;           // dropout keep masks (avsr_attn_dropmask, query on the lane) or null
  int mnqb, mnkb;               // their 32-row query blocks / (even) 32-row key blocks per head
};

// write a pair of accumulator tiles X[dt] (rows d = dt*32 + qrow, column = lane&31) transposed
// (out row = column index) through the wave's LDS slab st[32][65]; rows r0.. of out (the store
// epilogue of every kernel)
template <typename T>
AVSR_DEV void store_t(const f32x16& x0, const f32x16& x1, float mul, float* st, T* out, int64_t ld, int nvalid) {
  const int l = threadIdx.x & 63, c = l & 31, hh = l >> 5;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    st[c * 65 + qrow(r, hh)] = x0[r] * mul;
    st[c * 65 + 32 + qrow(r, hh)] = x1[r] * mul;
  }
  __syncthreads();
  // each store instruction writes whole 128-byte (bf16) / 256-byte (fp32) output rows: lane l
  // takes row i0 + l / LPR, elements (l % LPR) * VE ..; the slab reads are conflict-free (row
  // stride 65 floats)
  constexpr int VE = 16 / (int)sizeof(T), LPR = 64 / VE, RPI = 64 / LPR;
  const int rr = l / LPR, ch = (l % LPR) * VE;
#pragma unroll
  for (int i0 = 0; i0 < 32; i0 += RPI) {
    const int i = i0 + rr;
    if (i < nvalid) {
      float v[VE];
#pragma unroll
      for (int j = 0; j < VE; ++j) v[j] = st[i * 65 + ch + j];
      stv(out + (int64_t)i * ld + ch, v);
    }
  }
}

// ---- padded row-major bf16 LDS images [rows][ROW] (v2, res) -----------------------------
typedef short s4v __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) s4v lds_s4v;   // ds_read_b64_tr_b16 operand (rdT, sq::ldT)
constexpr int ROW = 72;          // 144-B rows: b128 reads of 16 rows at one column hit distinct banks
// A/B fragment of mfma32 with the operand row on the lane: X[row][col .. col+7] (v2, res)
AVSR_DEV bf16x8 rd8(const bf16* img, int row, int col) { return *(const bf16x8*)&img[row * ROW + col]; }
// Transposed A fragment of mfma32 from a row-major image: lane l gets X^T[c0 + (l&31)][r]
// for r = r0 + 4*(l>>5) + {0..3, 8..11} — the row order of accumulator registers
// 8S..8S+7 used as a B operand (accb), so r0 = (row block of the accumulator) + 16 S. (v2, res)
AVSR_DEV bf16x8 rdT(const bf16* img, int r0, int c0, int lane) {
  const int hh = lane >> 5, g = (lane >> 4) & 1, i = lane & 15;
  const bf16* pa = img + (r0 + 4 * hh + (i >> 2)) * ROW + c0 + 16 * g + 4 * (i & 3);
  union { s4v s[2]; bf16x8 h; } u;
  u.s[0] = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s4v*)pa);
  u.s[1] = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s4v*)(pa + 8 * ROW));
  return u.h;
}
// accumulator registers 8S..8S+7 as a bf16 operand fragment (every bf16 kernel)
AVSR_DEV bf16x8 accb(const f32x16& x, int S) {
  bf16x8 h;
#pragma unroll
  for (int j = 0; j < 8; ++j) h[j] = (bf16)x[8 * S + j];
  return h;
}

// fragment row load without a branch: row index clamped, value selected (res, sq, rb)
AVSR_DEV bf16x8 ldrow_sel(const bf16* base, int64_t ld, int row, int nrows, int col) {
  const v16 x = *(const v16*)(base + (int64_t)min(row, nrows - 1) * ld + col);
  v16 y;
#pragma unroll
  for (int j = 0; j < 4; ++j) y.w[j] = row < nrows ? x.w[j] : 0u;
  return *(const bf16x8*)&y;
}

// AttnDrop's 32-bit-index form (the dispatcher guarantees B*H*Lq*ceil(Lk/2) < 2^32) with the
// golden-ratio premultiply distributed over the index: hash(g) = fmix32(g*G ^ pre) and
// g*G = rowG + (k/2)*G (mod 2^32): per pair only an add, a xor and the finaliser (res, sq, rb)
AVSR_DEV uint32_t hashG(uint32_t gG, uint32_t pre) { return fmix32(gG ^ pre); }
// keep decisions of a score tile held as (query on the lane, keys k0 + qrow(r, hh)): registers
// r, r+1 (r even) are keys 2j, 2j+1 of one pair; tG = ((bh*Lq + q) * npair + k0/2) * G.
// Selection form: dropped elements -> 0, kept ones unscaled (the 1/(1-p) factor is applied once
// to the tile's output sums by the caller) (res, sq, rb)
AVSR_DEV void drop_tile_sel(f32x16& x, uint32_t tG, const AttnDrop& d, int hh) {
#pragma unroll
  for (int r = 0; r < 16; r += 2) {
    const uint32_t kp = (uint32_t)(((r & 3) >> 1) + 4 * (r >> 2) + 2 * hh);     // (qrow(r, hh) >> 1)
    const uint32_t h = hashG(tG + kp * GOLD, d.pre);
    x[r] = (h & 0xFFFFu) >= d.thr ? x[r] : 0.f;
    x[r + 1] = (h >> 16) >= d.thr ? x[r + 1] : 0.f;
  }
}

// stored dropout masks (avsr_attn_dropmask): 16 lane masks per 32 x 32 tile, read through the
// constant address space so that a wave-uniform tile address becomes scalar loads (sq, rb)
typedef const __attribute__((address_space(4))) uint64_t* smask_t;
AVSR_DEV smask_t mask_tile(const uint64_t* base, int64_t tile) { return (smask_t)(base + tile * 16); }
// x on the lanes whose bit of m is set, else 0: one v_cndmask, the scalar mask as condition (sq, rb)
AVSR_DEV float msel(float x, uint64_t m) {
  float r;
  asm("v_cndmask_b32_e64 %0, 0, %1, %2" : "=v"(r) : "v"(x), "s"(m));
  return r;
}
// XCD-aware block order (blocks b, b + 8 share an XCD): consecutive ids on one XCD (sq, rb)
AVSR_DEV int xcd_id(int orig, int nwg) {
  const int xcd = orig & 7, q = nwg >> 3, r = nwg & 7;
  return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (orig >> 3);
}

// diagnostic only (avsr_debug_attn_stamps): per workgroup [start, after loads, after compute,
// end] s_memrealtime ticks (100 MHz) and the hardware id, written by lane 0 of wave 0 to a
// buffer of its own; no output depends on it. Static: each file has its own pointer (device symbols
// are not shared across files); the two whose kernels stamp (res::attn_fwd_kernel, rb::) export a setter
static __device__ unsigned long long* g_stamps = nullptr;
AVSR_DEV void stamp(int slot) {
  unsigned long long* st = g_stamps;
  if (st != nullptr && threadIdx.x == 0) {
    const unsigned long long t = __builtin_amdgcn_s_memrealtime();
    st[(blockIdx.y * gridDim.x + blockIdx.x) * 6 + slot] = t;
    if (slot == 0) {
      st[(blockIdx.y * gridDim.x + blockIdx.x) * 6 + 4] = (unsigned long long)__builtin_amdgcn_s_getreg((4) | (0 << 6) | (31 << 11));
      st[(blockIdx.y * gridDim.x + blockIdx.x) * 6 + 5] = (unsigned long long)__builtin_amdgcn_s_getreg((20) | (0 << 6) | (31 << 11));
    }
  }
}
// the same per workgroup for a 1-D grid at buffer offset `part` x (6 x gridDim.x): the encoder
// backward's fused kernel (part 0), or its dQ (part 0) and dK / dV (part 1) kernels
AVSR_DEV void stamp_part(int slot, int part) {
  unsigned long long* st = g_stamps;
  if (st != nullptr && threadIdx.x == 0) {
    unsigned long long* o = st + ((unsigned long long)part * gridDim.x + blockIdx.x) * 6;
    o[slot] = __builtin_amdgcn_s_memrealtime();
    if (slot == 0) {
      o[4] = (unsigned long long)__builtin_amdgcn_s_getreg((4) | (0 << 6) | (31 << 11));
      o[5] = (unsigned long long)__builtin_amdgcn_s_getreg((20) | (0 << 6) | (31 << 11));
    }
  }
}
// kernels with more than 64 KiB of dynamic LDS (resident and encoder-backward launchers)
template <typename F> void allow_lds(F* f) {
  static bool done = false;                     // once per kernel instantiation
  if (!done) {
    (void)hipFuncSetAttribute((const void*)f, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    done = true;
  }
}

// The launchers attention.hip dispatches to: each takes a checked call whose path attn_path chose
// (dQ goes to p->dq_out if set, else to p->dq) and returns 0, a HIP launch error or an AVSR_E_* code
typedef int Launcher(const avsr_attn_params* p, const AttnArgs& a, hipStream_t st);
Launcher f32_fwd, f32_bwd;                            // attention_f32.hip
Launcher tiled_fwd, tiled_bwd;                        // attention_tiled.hip
Launcher resident_fwd, resident_bwd, resident_mask;   // attention_resident.hip (mask: avsr_attn_dropmask's kernel)
Launcher sq_fwd, enc_bwd;                             // attention_enc.hip
int resident_stamps(unsigned long long* buf), enc_stamps(unsigned long long* buf);   // set g_stamps of their file
}  // namespace attn
