// Fused attention, resident kernels (AVSR_ATTN_PATH_RESIDENT: bf16, forward Lk <= 384, backward
// Lq and Lk <= 384: the decoder's self / source attention, and the encoder's 375-frame attention
// where sq / rb do not take it). One workgroup per (batch, head) and 32-row block range: the
// whole streamed operand pair of that head (K and V for the forward / dQ, Q and dO for
// dK / dV) is loaded into LDS ONCE (<= 2 x 384 x 144 B), then every wave (32 rows of its own
// dimension on the MFMA lanes) sweeps it with no further barrier — nothing to pipeline, waves
// drift freely, 3 waves per SIMD hide each other's MFMA / VALU / LDS latency.
//   forward: one pass per 32-query wave, online softmax against a lazily raised reference max
//            (P = exp2(S - ref), row sum, dropout, O^T += V^T P^T; O is rescaled only when ref moves);
//   dK/dV:   per 32-key wave: S, dP with the key on the lane, dV^T += dO^T P', dK^T += Q^T dS;
//            delta = rowsum(dO * O) is computed here (Q/dO already in LDS) and published for dQ;
//   dQ:      per 32-query wave: S^T, dP^T, dQ^T += K^T dS^T.
// Dropout: AttnDrop pairs — in the forward / dQ layout a lane holds 4 consecutive keys of one
// query per register quad (2 hashes); in the dK/dV layout the key pair sits on lanes c, c^1,
// which split the 16 queries' hashes and swap halves (__shfl_xor 1).
// Also here: attn_mask_kernel, the stored keep masks of avsr_attn_dropmask (read by sq / rb).
#include "attention.h"

namespace attn {
namespace res {
constexpr int MAXW = MAXR / 32;     // waves per workgroup (768 threads)

// Two [n][64] row-major operands -> two padded LDS images (rows >= n zero), every global load
// of a pass issued before any LDS write (one HBM round trip per pass of 4 vectors per thread
// per image instead of one per vector); out-of-range rows load a clamped valid row and are
// zeroed by a select, so no load sits behind a branch
constexpr int LD_IT = 4;
AVSR_DEV void load_pair(bf16* i1, const bf16* s1, int64_t ld1, bf16* i2, const bf16* s2, int64_t ld2, int n, int nz,
                        int tid, int nthr) {
  for (int base = 0; base < nz * 8; base += LD_IT * nthr) {
    v16 x1[LD_IT], x2[LD_IT];
#pragma unroll
    for (int it = 0; it < LD_IT; ++it) {
      const int id = base + it * nthr + tid, row = id >> 3, ch = (id & 7) * 8;
      const int rr = min(row, n - 1);
      x1[it] = *(const v16*)(s1 + (int64_t)rr * ld1 + ch);
      x2[it] = *(const v16*)(s2 + (int64_t)rr * ld2 + ch);
    }
#pragma unroll
    for (int it = 0; it < LD_IT; ++it) {
      const int id = base + it * nthr + tid, row = id >> 3, ch = (id & 7) * 8;
      if (id < nz * 8) {
        const bool ok = row < n;
#pragma unroll
        for (int j = 0; j < 4; ++j) { x1[it].w[j] = ok ? x1[it].w[j] : 0u; x2[it].w[j] = ok ? x2[it].w[j] : 0u; }
        *(v16*)&i1[row * ROW + ch] = x1[it];
        *(v16*)&i2[row * ROW + ch] = x2[it];
      }
    }
  }
}

__global__ __launch_bounds__(768) void attn_fwd_kernel(AttnArgs a) {
  extern __shared__ __attribute__((aligned(16))) bf16 sm[];
  stamp(0);
  const int bh = blockIdx.x, b = bh / a.H, h = bh % a.H;
  const int tid = threadIdx.x, nthr = blockDim.x, w = tid >> 6, l = tid & 63, c = l & 31, hh = l >> 5;
  const int nk = (a.Lk + 31) & ~31;
  bf16* Ks = sm;
  bf16* Vs = sm + nk * ROW;
  const int q0 = (blockIdx.y * (nthr >> 6) + w) * 32, qi = q0 + c;
  const bf16* Q = (const bf16*)a.q + (int64_t)b * a.Lq * a.ldq + h * DH;
  bf16x8 qf[4];
#pragma unroll
  for (int s = 0; s < 4; ++s) qf[s] = ldrow_sel(Q, a.ldq, qi, a.Lq, s * 16 + 8 * hh);
  // K/V images: when one pass of LD_IT vectors per thread covers them, all loads are issued
  // here and the images are written round by round inside the tile loop (round r = rows
  // [r*nthr/8, (r+1)*nthr/8)), so later rounds' HBM latency hides behind the first tiles'
  // compute (one workgroup per head per CU leaves nothing else to hide it); the barriers are
  // raw s_barrier after lgkmcnt(0), which do not drain the outstanding loads
  const bf16* Kg = (const bf16*)a.k + (int64_t)b * a.Lk * a.ldk + h * DH;
  const bf16* Vg = (const bf16*)a.v + (int64_t)b * a.Lk * a.ldv + h * DH;
  const bool pipe = nk * 8 <= LD_IT * nthr;
  const int rtot = pipe ? (nk * 8 + nthr - 1) / nthr : 0;     // rounds to write (uniform)
  const int rpr = nthr >> 3;                                    // image rows per round
  v16 xk[LD_IT], xv[LD_IT];
  if (pipe) {
#pragma unroll
    for (int it = 0; it < LD_IT; ++it) {
      const int id = it * nthr + tid, rr = min(id >> 3, a.Lk - 1), ch = (id & 7) * 8;
      xk[it] = *(const v16*)(Kg + (int64_t)rr * a.ldk + ch);
      xv[it] = *(const v16*)(Vg + (int64_t)rr * a.ldv + ch);
    }
  } else {
    load_pair(Ks, Kg, a.ldk, Vs, Vg, a.ldv, a.Lk, nk, tid, nthr);
  }
  const int klen = a.klen ? min(a.klen[b], a.Lk) : a.Lk;
  const int kend = a.causal ? min(klen, q0 + 32) : klen;
  const int nt = (kend + 31) >> 5;
  const float sl2 = a.scale * LOG2E;
  const AttnDrop drop(a.drop_p, a.seed, a.B, a.H, a.Lq, a.Lk);
  const uint32_t rowG = ((uint32_t)bh * (uint32_t)a.Lq + (uint32_t)min(qi, a.Lq - 1)) * drop.npair * GOLD;
  if (!pipe) __syncthreads();
  f32x16 o0, o1;
  zacc(o0); zacc(o1);
  float lsum = 0.f;
  // reference max (log2 units, scale * log2(e) applied): -inf until the row sees a key; it only
  // moves when a tile's max exceeds it by more than 8, so P = exp2(s - mb) <= 256 and the
  // rescale of O / the row sum (exact: softmax does not depend on the reference) is rare
  float mb = -INFINITY;
  int t = 0;                                    // next key tile
#pragma unroll
  for (int it = 0; it < LD_IT; ++it) {
    if (pipe && it < rtot) {
      const int id = it * nthr + tid, row = id >> 3, ch = (id & 7) * 8;
      if (id < nk * 8) {
        const bool ok = row < a.Lk;
#pragma unroll
        for (int j = 0; j < 4; ++j) { xk[it].w[j] = ok ? xk[it].w[j] : 0u; xv[it].w[j] = ok ? xv[it].w[j] : 0u; }
        *(v16*)&Ks[row * ROW + ch] = xk[it];
        *(v16*)&Vs[row * ROW + ch] = xv[it];
      }
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();
      asm volatile("" ::: "memory");
      if (it == 0) stamp(1);
    }
    // tiles whose 32 keys are all in LDS after this round
    const int tend = (!pipe || it + 1 >= rtot) ? nt : min(nt, ((it + 1) * rpr) >> 5);
    if (q0 >= a.Lq) continue;
    // one pass, online softmax: per 32-key tile S^T = K Q^T, the row max over the tile (the
    // two lane halves hold the same query, different keys), rescale of the running O^T / row
    // sum when the max grows (per-lane scalar: the lane's accumulator column is its query),
    // P = exp2(S*scale*log2e - max), dropout, O^T += V^T P^T
    for (; t < tend; ++t) {
      f32x16 st;
      zacc(st);
#pragma unroll
      for (int s = 0; s < 4; ++s) st = mfma32(rd8(Ks, t * 32 + c, s * 16 + 8 * hh), qf[s], st);
      const bool full = t * 32 + 32 <= klen && (!a.causal || t * 32 + 31 <= q0);
      if (!full) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int k = t * 32 + qrow(r, hh);
          const bool ok = (k < klen) & (!a.causal | (k <= qi));
          st[r] = ok ? st[r] : -INFINITY;
        }
      }
      float mx[8];
#pragma unroll
      for (int r = 0; r < 8; ++r) mx[r] = fmaxf(st[r], st[r + 8]);
#pragma unroll
      for (int w2 = 4; w2 > 0; w2 >>= 1)
#pragma unroll
        for (int r = 0; r < w2; ++r) mx[r] = fmaxf(mx[r], mx[r + w2]);
      float mt = xor32_max(mx[0]) * sl2;
      // a query with no visible key so far keeps mb = -inf (exponent reference 0) and
      // contributes exp2(-inf) = 0; the MFMAs below run for the whole wave
      const bool grow = mt > mb + 8.f;
      if (__any(grow)) {                            // wave-uniform: rare after the first tile
        const float alpha = grow ? (mb == -INFINITY ? 0.f : fexp2(mb - mt)) : 1.f;
        mb = grow ? mt : mb;
        lsum *= alpha;
#pragma unroll
        for (int r = 0; r < 16; ++r) { o0[r] *= alpha; o1[r] *= alpha; }
      }
      const float mbu = mb == -INFINITY ? 0.f : mb;
      float ts[8];
#pragma unroll
      for (int r = 0; r < 16; ++r) st[r] = fexp2(fmaf(st[r], sl2, -mbu));     // masked keys: exp2(-inf) = 0
#pragma unroll
      for (int r = 0; r < 8; ++r) ts[r] = st[r] + st[r + 8];
#pragma unroll
      for (int w2 = 4; w2 > 0; w2 >>= 1)
#pragma unroll
        for (int r = 0; r < w2; ++r) ts[r] += ts[r + w2];
      lsum += ts[0];
      if (a.drop_p > 0.f) drop_tile_sel(st, rowG + (uint32_t)(t * 16) * GOLD, drop, hh);
      const bf16x8 pa = accb(st, 0), pb = accb(st, 1);
      o0 = mfma32(rdT(Vs, t * 32, 0, l), pa, o0);
      o0 = mfma32(rdT(Vs, t * 32 + 16, 0, l), pb, o0);
      o1 = mfma32(rdT(Vs, t * 32, 32, l), pa, o1);
      o1 = mfma32(rdT(Vs, t * 32 + 16, 32, l), pb, o1);
    }
  }
  if (q0 < a.Lq) {
    lsum = xor32_sum(lsum);
    if (hh == 0 && qi < a.Lq)
      a.lse[(int64_t)bh * a.Lq + qi] = lsum > 0.f ? (mb + log2f(lsum)) * LN2 : -INFINITY;
  }
  __syncthreads();                         // K/V images no longer read: reuse LDS as store slabs
  stamp(2);
  if (q0 < a.Lq) {
    const float inv = lsum > 0.f ? (a.drop_p > 0.f ? drop.scale : 1.f) / lsum : 0.f;
    bf16* O = (bf16*)a.o + ((int64_t)b * a.Lq + q0) * a.ldo + h * DH;
    store_t<bf16>(o0, o1, inv, (float*)sm + w * 32 * 65, O, a.ldo, a.Lq - q0);
  }
  __syncthreads();
  stamp(3);
}

// dK / dV (decoder shapes: causal self-attention, source attention), one workgroup per (b, h)
// and up to 12 waves of 32 keys; dropout hashed per key pair
__global__ __launch_bounds__(768) void attn_bwd_dkdv_kernel(AttnArgs a) {
  extern __shared__ __attribute__((aligned(16))) bf16 sm[];
  const int bh = blockIdx.x, b = bh / a.H, h = bh % a.H;
  const int tid = threadIdx.x, nthr = blockDim.x, l = tid & 63, c = l & 31, hh = l >> 5;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int nq = (a.Lq + 31) & ~31;
  bf16* Qs = sm;
  bf16* dOs = sm + nq * ROW;
  float* lss = (float*)(sm + 2 * nq * ROW);          // lse * log2(e) (0 past Lq)
  float* dls = lss + nq;                              // delta (0 past Lq)
  const bf16* Q = (const bf16*)a.q + (int64_t)b * a.Lq * a.ldq + h * DH;
  const bf16* dO = (const bf16*)a.dout + (int64_t)b * a.Lq * a.lddo + h * DH;
  const int kb0 = (blockIdx.y * (nthr >> 6) + w) * 32, key = kb0 + c;
  const bf16* K = (const bf16*)a.k + (int64_t)b * a.Lk * a.ldk + h * DH;
  const bf16* V = (const bf16*)a.v + (int64_t)b * a.Lk * a.ldv + h * DH;
  bf16x8 kf[4], vf[4];
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    kf[s] = ldrow_sel(K, a.ldk, key, a.Lk, s * 16 + 8 * hh);
    vf[s] = ldrow_sel(V, a.ldv, key, a.Lk, s * 16 + 8 * hh);
  }
  // Q / dO images and delta[q] = sum_d dO * O in one pass: every load of a pass is issued
  // first; 8 consecutive lanes hold one query row (one 16-byte chunk each)
  {
    const bf16* O = (const bf16*)a.o + (int64_t)b * a.Lq * a.ldo + h * DH;
    for (int base = 0; base < nq * 8; base += LD_IT * nthr) {
      v16 xq[LD_IT], xd[LD_IT], xo[LD_IT];
      float ls[LD_IT];
#pragma unroll
      for (int it = 0; it < LD_IT; ++it) {
        const int id = base + it * nthr + tid, rr = min(id >> 3, a.Lq - 1), ch = (id & 7) * 8;
        xq[it] = *(const v16*)(Q + (int64_t)rr * a.ldq + ch);
        xd[it] = *(const v16*)(dO + (int64_t)rr * a.lddo + ch);
        xo[it] = *(const v16*)(O + (int64_t)rr * a.ldo + ch);
        ls[it] = a.lse[(int64_t)bh * a.Lq + rr];
      }
#pragma unroll
      for (int it = 0; it < LD_IT; ++it) {
        const int id = base + it * nthr + tid, q = id >> 3, ch = (id & 7) * 8;
        const bool ok = q < a.Lq;
        float sacc = 0.f;
        const bf16x8 ov = *(const bf16x8*)&xo[it], dv = *(const bf16x8*)&xd[it];
#pragma unroll
        for (int j = 0; j < 8; ++j) sacc += (float)ov[j] * (float)dv[j];
        sacc = ok ? sacc : 0.f;
        sacc += __shfl_xor(sacc, 1, 64);
        sacc += __shfl_xor(sacc, 2, 64);
        sacc += __shfl_xor(sacc, 4, 64);
        if (id < nq * 8) {
#pragma unroll
          for (int j = 0; j < 4; ++j) { xq[it].w[j] = ok ? xq[it].w[j] : 0u; xd[it].w[j] = ok ? xd[it].w[j] : 0u; }
          *(v16*)&Qs[q * ROW + ch] = xq[it];
          *(v16*)&dOs[q * ROW + ch] = xd[it];
          if ((id & 7) == 0) {
            dls[q] = sacc;
            lss[q] = ok ? ls[it] * LOG2E : 0.f;
            if (blockIdx.y == 0 && ok) a.delta[(int64_t)bh * a.Lq + q] = sacc;
          }
        }
      }
    }
  }
  const int klen = a.klen ? min(a.klen[b], a.Lk) : a.Lk;
  const float sl2 = a.scale * LOG2E;
  const bool drop_on = a.drop_p > 0.f;
  uint32_t thr = 0, pre = 0, nG = 0, keyG = 0;
  float dscale = 1.f;
  if (drop_on) {
    const AttnDrop drop(a.drop_p, a.seed, a.B, a.H, a.Lq, a.Lk);
    dscale = drop.scale;
    thr = drop.thr; pre = drop.pre; nG = drop.npair * GOLD;
    keyG = ((uint32_t)bh * (uint32_t)a.Lq * drop.npair + (uint32_t)(min(key, a.Lk - 1) >> 1)) * GOLD;
  }
  const bool odd = c & 1;
  __syncthreads();
  f32x16 dv0, dv1, dk0, dk1;
  zacc(dv0); zacc(dv1); zacc(dk0); zacc(dk1);
  if (kb0 < a.Lk && kb0 < klen) {
    const int qstart = a.causal ? kb0 : 0;
    const int nt = (a.Lq - qstart + 31) >> 5;
    const bool kok = key < klen;
    for (int t = 0; t < nt; ++t) {
      const int qt0 = qstart + t * 32;
      f32x16 sc, dp;
      zacc(sc); zacc(dp);
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        sc = mfma32(rd8(Qs, qt0 + c, s * 16 + 8 * hh), kf[s], sc);
        dp = mfma32(rd8(dOs, qt0 + c, s * 16 + 8 * hh), vf[s], dp);
      }
      const uint32_t tG = keyG + (uint32_t)(qt0 + 4 * hh) * nG;
      const bool full = kok && qt0 + 32 <= a.Lq && (!a.causal || key <= qt0);
#pragma unroll
      for (int i = 0; i < 4; ++i) {                 // registers 4i..4i+3 = queries qt0 + 8i + 4hh + 0..3
        const f32x4 ls = *(const f32x4*)&lss[qt0 + 8 * i + 4 * hh];
        const f32x4 ds = *(const f32x4*)&dls[qt0 + 8 * i + 4 * hh];
        // P' = dropout(P) is stored unscaled (the 1/(1-p) factor goes on dV at the store),
        // dP' = dropout(dP) scaled; the softmax scale of dS goes on dK at the store
        {
          // hashed dropout: this lane pair (keys 2j, 2j+1) splits the 4 queries' hashes: even
          // lanes hash queries 0, 1, odd lanes 2, 3, then the two swap (static registers only)
          bool kb[4] = {true, true, true, true};
          if (drop_on) {
#pragma unroll
            for (int u = 0; u < 2; ++u) {
              const uint32_t mine = hashG(tG + (uint32_t)(8 * i + (odd ? 2 : 0) + u) * nG, pre);
              const uint32_t other = __shfl_xor(mine, 1, 64);
              const uint32_t h0 = odd ? other : mine, h1 = odd ? mine : other;
              kb[u] = (odd ? (h0 >> 16) : (h0 & 0xFFFFu)) >= thr;
              kb[u + 2] = (odd ? (h1 >> 16) : (h1 & 0xFFFFu)) >= thr;
            }
          }
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const int r = 4 * i + e, ql = qt0 + 8 * i + 4 * hh + e;
            const bool ok = full || (kok & (ql < a.Lq) & (!a.causal | (key <= ql)));
            const float p = ok ? fexp2(fmaf(sc[r], sl2, -ls[e])) : 0.f;
            sc[r] = kb[e] ? p : 0.f;
            dp[r] = p * fmaf(kb[e] ? dp[r] : 0.f, dscale, -ds[e]);
          }
        }
      }
      const bf16x8 pa = accb(sc, 0), pb = accb(sc, 1), sa = accb(dp, 0), sb = accb(dp, 1);
      dv0 = mfma32(rdT(dOs, qt0, 0, l), pa, dv0);
      dv0 = mfma32(rdT(dOs, qt0 + 16, 0, l), pb, dv0);
      dv1 = mfma32(rdT(dOs, qt0, 32, l), pa, dv1);
      dv1 = mfma32(rdT(dOs, qt0 + 16, 32, l), pb, dv1);
      dk0 = mfma32(rdT(Qs, qt0, 0, l), sa, dk0);
      dk0 = mfma32(rdT(Qs, qt0 + 16, 0, l), sb, dk0);
      dk1 = mfma32(rdT(Qs, qt0, 32, l), sa, dk1);
      dk1 = mfma32(rdT(Qs, qt0 + 16, 32, l), sb, dk1);
    }
  }
  __syncthreads();
  if (kb0 < a.Lk) {
    float* scr = (float*)sm + w * 32 * 65;
    bf16* DK = (bf16*)a.dk + ((int64_t)b * a.Lk + kb0) * a.lddk + h * DH;
    store_t<bf16>(dk0, dk1, a.scale, scr, DK, a.lddk, a.Lk - kb0);
    bf16* DV = (bf16*)a.dv + ((int64_t)b * a.Lk + kb0) * a.lddv + h * DH;
    store_t<bf16>(dv0, dv1, dscale, scr, DV, a.lddv, a.Lk - kb0);
  }
}

// dQ (decoder shapes), one workgroup per (b, h) and up to 12 waves of 32 queries
template <typename OutT>
__global__ __launch_bounds__(768) void attn_bwd_dq_kernel(AttnArgs a, OutT* dq, int64_t lddq) {
  extern __shared__ __attribute__((aligned(16))) bf16 sm[];
  const int bh = blockIdx.x, b = bh / a.H, h = bh % a.H;
  const int tid = threadIdx.x, nthr = blockDim.x, l = tid & 63, c = l & 31, hh = l >> 5;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int nk = (a.Lk + 31) & ~31;
  bf16* Ks = sm;
  bf16* Vs = sm + nk * ROW;
  const int q0 = (blockIdx.y * (nthr >> 6) + w) * 32, qi = q0 + c;
  const bool qok = qi < a.Lq;
  const bf16* Q = (const bf16*)a.q + (int64_t)b * a.Lq * a.ldq + h * DH;
  const bf16* dO = (const bf16*)a.dout + (int64_t)b * a.Lq * a.lddo + h * DH;
  bf16x8 qf[4], of[4];
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    qf[s] = ldrow_sel(Q, a.ldq, qi, a.Lq, s * 16 + 8 * hh);
    of[s] = ldrow_sel(dO, a.lddo, qi, a.Lq, s * 16 + 8 * hh);
  }
  const int64_t bhq = (int64_t)bh * a.Lq + min(qi, a.Lq - 1);
  const float lq0 = a.lse[bhq], dl0 = a.delta[bhq];
  load_pair(Ks, (const bf16*)a.k + (int64_t)b * a.Lk * a.ldk + h * DH, a.ldk,
            Vs, (const bf16*)a.v + (int64_t)b * a.Lk * a.ldv + h * DH, a.ldv, a.Lk, nk, tid, nthr);
  const float lq = qok ? lq0 * LOG2E : 0.f;
  const float dl = qok ? dl0 : 0.f;
  const int klen = a.klen ? min(a.klen[b], a.Lk) : a.Lk;
  const int kend = a.causal ? min(klen, q0 + 32) : klen;
  const int nt = (kend + 31) >> 5;
  const float sl2 = a.scale * LOG2E;
  const AttnDrop drop(a.drop_p, a.seed, a.B, a.H, a.Lq, a.Lk);
  const uint32_t rowG = ((uint32_t)bh * (uint32_t)a.Lq + (uint32_t)min(qi, a.Lq - 1)) * drop.npair * GOLD;
  const float dscale = drop.scale;
  __syncthreads();
  f32x16 dq0, dq1;
  zacc(dq0); zacc(dq1);
  if (q0 < a.Lq) {
    for (int t = 0; t < nt; ++t) {
      f32x16 st, dpt;
      zacc(st); zacc(dpt);
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        st = mfma32(rd8(Ks, t * 32 + c, s * 16 + 8 * hh), qf[s], st);
        dpt = mfma32(rd8(Vs, t * 32 + c, s * 16 + 8 * hh), of[s], dpt);
      }
      // dP' = dropout(dP): kept elements scaled by 1/(1-p) (dscale), dropped ones 0; the
      // softmax scale of dS is applied to dQ once, at the store
      if (a.drop_p > 0.f) {
#pragma unroll
        for (int r = 0; r < 16; ++r) dpt[r] *= dscale;
        drop_tile_sel(dpt, rowG + (uint32_t)(t * 16) * GOLD, drop, hh);
      }
      if (t * 32 + 32 <= klen && (!a.causal || t * 32 + 31 <= q0)) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const float p = fexp2(fmaf(st[r], sl2, -lq));
          dpt[r] = p * (dpt[r] - dl);
        }
      } else {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int k = t * 32 + qrow(r, hh);
          const bool ok = (k < klen) & (!a.causal | (k <= qi));
          const float p = ok ? fexp2(fmaf(st[r], sl2, -lq)) : 0.f;
          dpt[r] = p * (dpt[r] - dl);
        }
      }
      const bf16x8 sa = accb(dpt, 0), sb = accb(dpt, 1);
      dq0 = mfma32(rdT(Ks, t * 32, 0, l), sa, dq0);
      dq0 = mfma32(rdT(Ks, t * 32 + 16, 0, l), sb, dq0);
      dq1 = mfma32(rdT(Ks, t * 32, 32, l), sa, dq1);
      dq1 = mfma32(rdT(Ks, t * 32 + 16, 32, l), sb, dq1);
    }
  }
  __syncthreads();
  if (q0 < a.Lq) {
    OutT* DQ = dq + ((int64_t)b * a.Lq + q0) * lddq + h * DH;
    store_t<OutT>(dq0, dq1, a.scale, (float*)sm + w * 32 * 65, DQ, lddq, a.Lq - q0);
  }
}

// the keep masks of avsr_attn_dropmask: workgroup (qb, bh) of 4 waves, wave w writes the lane
// masks of the tiles (bh, qb, kb = w, w + 4, ..), query on the lane (AttnDrop's bits, 0 past Lq /
// Lk). Register pair (r, r + 1) of a lane holds keys 2j, 2j + 1: one hash per pair, 32-bit
// index arithmetic, no divisions.
__global__ __launch_bounds__(256) void attn_mask_kernel(AttnArgs a, uint64_t* mq) {
  const int l = threadIdx.x & 63, c = l & 31, hh = l >> 5;
  const int w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int qb = blockIdx.x, bh = blockIdx.y;
  const AttnDrop d(a.drop_p, a.seed, a.B, a.H, a.Lq, a.Lk);
  const int q = qb * 32 + c;
  // pair index of register pair (r, r + 1): row (bh, q), pair kb * 16 + ((r & 3) >> 1) + 4 (r >> 2) + 2 hh
  const uint32_t rowG = (((uint32_t)bh * (uint32_t)a.Lq + (uint32_t)min(q, a.Lq - 1)) * d.npair + (uint32_t)(2 * hh)) * GOLD;
  uint64_t* out = mq + ((int64_t)bh * a.mnqb + qb) * a.mnkb * 16;
  auto tile = [&](int kb, auto edge) {
    const uint32_t gG = rowG + (uint32_t)(kb * 16) * GOLD;
    // edge tiles: thresholds that reject keys past Lk and every key of a query past Lq
    const int klim = q < a.Lq ? a.Lk - kb * 32 - 4 * hh : -1;
    uint32_t wlo = 0, whi = 0;                         // lane r < 16: lane mask r
#pragma unroll
    for (int r = 0; r < 16; r += 2) {
      const uint32_t hv = hashG(gG + (uint32_t)(((r & 3) >> 1) + 4 * (r >> 2)) * GOLD, d.pre);
      bool k0 = (hv & 0xFFFFu) >= d.thr, k1 = (hv >> 16) >= d.thr;
      if (edge) {
        const int kr = (r & 3) + 8 * (r >> 2);        // key offset in the tile, minus 4 hh
        k0 = k0 & (kr < klim);
        k1 = k1 & (kr + 1 < klim);
      }
      const uint64_t b0 = __ballot(k0), b1 = __ballot(k1);
      wlo = l == r ? (uint32_t)b0 : wlo;
      whi = l == r ? (uint32_t)(b0 >> 32) : whi;
      wlo = l == r + 1 ? (uint32_t)b1 : wlo;
      whi = l == r + 1 ? (uint32_t)(b1 >> 32) : whi;
    }
    if (l < 16) out[kb * 16 + l] = ((uint64_t)whi << 32) | wlo;
  };
  for (int kb = w; kb < a.mnkb; kb += 4) {
    if (qb * 32 + 32 <= a.Lq && kb * 32 + 32 <= a.Lk) tile(kb, std::false_type());
    else tile(kb, std::true_type());
  }
}

// launch geometry: waves per workgroup (<= 12) covering `rows` 32-row blocks, grid.y chunks
inline int nwaves(int rows) { const int n = (rows + 31) / 32; return n < MAXW ? n : MAXW; }
inline size_t img_lds(int rows) { return (size_t)2 * ((rows + 31) & ~31) * ROW * sizeof(bf16); }
inline size_t slab_lds(int nw) { return (size_t)nw * 32 * 65 * sizeof(float); }
}  // namespace res

int resident_fwd(const avsr_attn_params* p, const AttnArgs& a, hipStream_t st) {
  const int nw = res::nwaves(p->Lq);
  const size_t lds = std::max(res::img_lds(p->Lk), res::slab_lds(nw));
  allow_lds(res::attn_fwd_kernel);
  dim3 g(p->B * p->H, (p->Lq + 32 * nw - 1) / (32 * nw));
  hipLaunchKernelGGL(res::attn_fwd_kernel, g, dim3(64 * nw), lds, st, a);
  return (int)hipGetLastError();
}

int resident_bwd(const avsr_attn_params* p, const AttnArgs& a, hipStream_t st) {
  // dK/dV: one workgroup per (b, h) of up to 12 waves (3 per SIMD), grid.y = 1 for L <= 384
  const int nwk = res::nwaves(p->Lk), nwq = res::nwaves(p->Lq);
  const size_t ldk = std::max(res::img_lds(p->Lq) + (size_t)2 * ((p->Lq + 31) & ~31) * sizeof(float), res::slab_lds(nwk));
  const dim3 gk(p->B * p->H, (p->Lk + 32 * nwk - 1) / (32 * nwk));
  allow_lds(res::attn_bwd_dkdv_kernel);
  hipLaunchKernelGGL(res::attn_bwd_dkdv_kernel, gk, dim3(64 * nwk), ldk, st, a);
  AVSR_CHECK_LAUNCH();
  const size_t ldq = std::max(res::img_lds(p->Lk), res::slab_lds(nwq));
  const dim3 gq(p->B * p->H, (p->Lq + 32 * nwq - 1) / (32 * nwq));
  if (p->dq_out) {
    allow_lds(res::attn_bwd_dq_kernel<bf16>);
    hipLaunchKernelGGL(res::attn_bwd_dq_kernel<bf16>, gq, dim3(64 * nwq), ldq, st, a, (bf16*)p->dq_out, p->lddq_out);
  } else {
    allow_lds(res::attn_bwd_dq_kernel<float>);
    hipLaunchKernelGGL(res::attn_bwd_dq_kernel<float>, gq, dim3(64 * nwq), ldq, st, a, p->dq, p->lddq);
  }
  return (int)hipGetLastError();
}

int resident_mask(const avsr_attn_params* p, const AttnArgs& a, hipStream_t st) {
  hipLaunchKernelGGL(res::attn_mask_kernel, dim3(a.mnqb, p->B * p->H), dim3(256), 0, st, a, const_cast<uint64_t*>(a.mq));
  return (int)hipGetLastError();
}
int resident_stamps(unsigned long long* buf) { return (int)hipMemcpyToSymbol(HIP_SYMBOL(g_stamps), &buf, sizeof(buf)); }
}  // namespace attn
