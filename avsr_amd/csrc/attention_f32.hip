// Fused attention, fp32 storage ("parity mode", AVSR_ATTN_PATH_F32): the round-1 tiles on bf16
// hi/lo splits (3 MFMA products per tile product).
// Forward (one workgroup = 4 waves = 128 queries of one (batch, head); K/V tiles of 32 keys
// staged in LDS and shared by the 4 waves):
//   S^T = K Q^T with the query on the MFMA lane, so each lane owns one query row of the
//   online softmax (16 of the 32 keys in registers, the other 16 on lane^32); P^T is then
//   already the B operand of O^T += V^T P^T (accumulator-as-operand, no LDS round trip);
//   V is staged transposed so its A fragments are two 8-byte LDS reads.
// Backward (one workgroup = 4 waves = 128 keys; each wave owns 32 keys and keeps dK^T,
//   dV^T in accumulators while sweeping all query tiles): S and dP are computed with the
//   key on the lane so they feed dV^T += dO^T P' and dK^T += Q^T dS directly; dS crosses
//   LDS once for dQ = dS K, which is summed over the 4 waves in LDS and added to an fp32
//   accumulator with one atomic per element per workgroup.
#include "attention.h"

namespace attn {
namespace f32 {

struct Frag { bf16x8 hi, lo; };

AVSR_DEV Frag mkfrag(const float* x) {
  Frag f;
  split8(x, f.hi, f.lo);
  return f;
}
AVSR_DEV Frag zfrag() {
  float z[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  return mkfrag(z);
}
// 8 contiguous elements
AVSR_DEV Frag ld8(const float* p) {
  f32x4 a = *(const f32x4*)p, b = *(const f32x4*)(p + 4);
  float x[8] = {a[0], a[1], a[2], a[3], b[0], b[1], b[2], b[3]};
  return mkfrag(x);
}
// two groups of 4 contiguous elements
AVSR_DEV Frag ld4x2(const float* p0, const float* p1) {
  f32x4 a = *(const f32x4*)p0, b = *(const f32x4*)p1;
  float x[8] = {a[0], a[1], a[2], a[3], b[0], b[1], b[2], b[3]};
  return mkfrag(x);
}
// registers 8s..8s+7 of an accumulator as an operand fragment
template <int S> AVSR_DEV Frag accfrag(const f32x16& x) {
  float v[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) v[j] = x[8 * S + j];
  return mkfrag(v);
}
AVSR_DEV void mm(f32x16& acc, const Frag& a, const Frag& b) {
  acc = mfma32(a.hi, b.hi, acc);
  acc = mfma32(a.hi, b.lo, acc);
  acc = mfma32(a.lo, b.hi, acc);
}

constexpr int VE = 4;               // floats per 16-byte vector
constexpr int KROW = DH + VE;       // [rows][64] tiles, b128-aligned rows
constexpr int VROW = 32 + 4;        // [64][32] transposed tiles
constexpr int SROW = 32 + VE;       // [32][32] dS tiles

__global__ __launch_bounds__(256) void attn_fwd_kernel(AttnArgs a) {
  __shared__ __attribute__((aligned(16))) float Ks[32 * KROW];
  __shared__ __attribute__((aligned(16))) float Vt[DH * VROW];
  __shared__ __attribute__((aligned(16))) float Os[4 * 32 * 65];
  const int b = blockIdx.y / a.H, h = blockIdx.y % a.H;
  const int tid = threadIdx.x, w = tid >> 6, l = tid & 63, c = l & 31, hh = l >> 5;
  const int q0 = blockIdx.x * 128 + w * 32, qi = q0 + c;
  const float* Q = (const float*)a.q + (int64_t)b * a.Lq * a.ldq + h * DH;
  const float* K = (const float*)a.k + (int64_t)b * a.Lk * a.ldk + h * DH;
  const float* V = (const float*)a.v + (int64_t)b * a.Lk * a.ldv + h * DH;
  Frag qf[4];
#pragma unroll
  for (int s = 0; s < 4; ++s) qf[s] = qi < a.Lq ? ld8(Q + (int64_t)qi * a.ldq + s * 16 + 8 * hh) : zfrag();
  f32x16 o0, o1;
  zacc(o0); zacc(o1);
  float m = -INFINITY, lsum = 0.f;
  const int klen = a.klen ? min(a.klen[b], a.Lk) : a.Lk;
  int kend = klen;
  if (a.causal) kend = min(kend, (int)blockIdx.x * 128 + 128);
  const float sl2 = a.scale * LOG2E;
  const AttnDrop drop(a.drop_p, a.seed, a.B, a.H, a.Lq, a.Lk);
  for (int kt0 = 0; kt0 < kend; kt0 += 32) {
    __syncthreads();
    for (int v = tid; v < 32 * DH / VE; v += 256) {
      const int key = v / (DH / VE), dv = (v % (DH / VE)) * VE;
      v16 kv, vv;
      if (kt0 + key < a.Lk) {
        kv = *(const v16*)(K + (int64_t)(kt0 + key) * a.ldk + dv);
        vv = *(const v16*)(V + (int64_t)(kt0 + key) * a.ldv + dv);
      } else {
        kv.w[0] = kv.w[1] = kv.w[2] = kv.w[3] = 0u; vv = kv;
      }
      *(v16*)&Ks[key * KROW + dv] = kv;
      const float* ve = (const float*)&vv;
#pragma unroll
      for (int e = 0; e < VE; ++e) Vt[(dv + e) * VROW + key] = ve[e];
    }
    __syncthreads();
    f32x16 st;
    zacc(st);
#pragma unroll
    for (int s = 0; s < 4; ++s) mm(st, ld8(&Ks[c * KROW + s * 16 + 8 * hh]), qf[s]);
    float mt = -INFINITY;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int key = kt0 + qrow(r, hh);
      const bool ok = key < klen && (!a.causal || key <= qi);
      st[r] = ok ? st[r] * sl2 : -INFINITY;
      mt = fmaxf(mt, st[r]);
    }
    mt = xor32_max(mt);
    const float mn = fmaxf(m, mt);
    const float alpha = mn == -INFINITY ? 1.f : exp2f(m - mn);
    float ps = 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const float p = st[r] == -INFINITY ? 0.f : exp2f(st[r] - mn);
      ps += p;
      st[r] = p;
    }
    ps = xor32_sum(ps);
    lsum = lsum * alpha + ps;
    m = mn;
#pragma unroll
    for (int r = 0; r < 16; ++r) { o0[r] *= alpha; o1[r] *= alpha; }
    if (a.drop_p > 0.f) {
#pragma unroll
      for (int r = 0; r < 16; ++r) st[r] *= drop.at(b * a.H + h, a.Lq, qi, kt0 + qrow(r, hh));
    }
    const Frag pf0 = accfrag<0>(st), pf1 = accfrag<1>(st);
#pragma unroll
    for (int dt = 0; dt < 2; ++dt) {
      const float* row = &Vt[(dt * 32 + c) * VROW + 4 * hh];
      const Frag v0 = ld4x2(row, row + 8), v1 = ld4x2(row + 16, row + 24);
      if (dt == 0) { mm(o0, v0, pf0); mm(o0, v1, pf1); }
      else { mm(o1, v0, pf0); mm(o1, v1, pf1); }
    }
  }
  const float inv = lsum > 0.f ? 1.f / lsum : 0.f;
  if (hh == 0 && qi < a.Lq) a.lse[(int64_t)(b * a.H + h) * a.Lq + qi] = lsum > 0.f ? (m + log2f(lsum)) * LN2 : -INFINITY;
  float* O = (float*)a.o + ((int64_t)b * a.Lq + q0) * a.ldo + h * DH;
  store_t<float>(o0, o1, inv, Os + w * 32 * 65, O, a.ldo, a.Lq - q0);
}

__global__ __launch_bounds__(256) void attn_bwd_kernel(AttnArgs a) {
  __shared__ __attribute__((aligned(16))) float Qs[32 * KROW];
  __shared__ __attribute__((aligned(16))) float QsT[DH * VROW];
  __shared__ __attribute__((aligned(16))) float dOs[32 * KROW];
  __shared__ __attribute__((aligned(16))) float dOsT[DH * VROW];
  __shared__ __attribute__((aligned(16))) float dSs[4 * 32 * SROW];
  __shared__ __attribute__((aligned(16))) float red[4 * 32 * 65];
  __shared__ float lse_s[32], dl_s[32];
  const int b = blockIdx.y / a.H, h = blockIdx.y % a.H;
  const int tid = threadIdx.x, w = tid >> 6, l = tid & 63, c = l & 31, hh = l >> 5;
  const int kb0 = blockIdx.x * 128 + w * 32, key = kb0 + c;
  const float* Q = (const float*)a.q + (int64_t)b * a.Lq * a.ldq + h * DH;
  const float* K = (const float*)a.k + (int64_t)b * a.Lk * a.ldk + h * DH;
  const float* V = (const float*)a.v + (int64_t)b * a.Lk * a.ldv + h * DH;
  const float* dO = (const float*)a.dout + (int64_t)b * a.Lq * a.lddo + h * DH;
  const float* LSE = a.lse + (int64_t)(b * a.H + h) * a.Lq;
  const float* DL = a.delta + (int64_t)(b * a.H + h) * a.Lq;
  Frag kf[4], vf[4], ktf[2][2];
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    kf[s] = key < a.Lk ? ld8(K + (int64_t)key * a.ldk + s * 16 + 8 * hh) : zfrag();
    vf[s] = key < a.Lk ? ld8(V + (int64_t)key * a.ldv + s * 16 + 8 * hh) : zfrag();
  }
#pragma unroll
  for (int dt = 0; dt < 2; ++dt)
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      float x[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int kk = kb0 + s * 16 + 8 * hh + j;
        x[j] = kk < a.Lk ? to_f(K[(int64_t)kk * a.ldk + dt * 32 + c]) : 0.f;
      }
      ktf[dt][s] = mkfrag(x);
    }
  f32x16 dv0, dv1, dk0, dk1;
  zacc(dv0); zacc(dv1); zacc(dk0); zacc(dk1);
  const int klen = a.klen ? min(a.klen[b], a.Lk) : a.Lk;
  const float sl2 = a.scale * LOG2E;
  const int qstart = a.causal ? (int)blockIdx.x * 128 : 0;
  const AttnDrop drop(a.drop_p, a.seed, a.B, a.H, a.Lq, a.Lk);
  float* dsw = dSs + w * 32 * SROW;
  float* rw = red + w * 32 * 65;
  for (int qt0 = qstart; qt0 < a.Lq; qt0 += 32) {
    __syncthreads();
    for (int v = tid; v < 32 * DH / VE; v += 256) {
      const int qq = v / (DH / VE), dv = (v % (DH / VE)) * VE;
      v16 qv, ov;
      if (qt0 + qq < a.Lq) {
        qv = *(const v16*)(Q + (int64_t)(qt0 + qq) * a.ldq + dv);
        ov = *(const v16*)(dO + (int64_t)(qt0 + qq) * a.lddo + dv);
      } else {
        qv.w[0] = qv.w[1] = qv.w[2] = qv.w[3] = 0u; ov = qv;
      }
      *(v16*)&Qs[qq * KROW + dv] = qv;
      *(v16*)&dOs[qq * KROW + dv] = ov;
      const float* qe = (const float*)&qv;
      const float* oe = (const float*)&ov;
#pragma unroll
      for (int e = 0; e < VE; ++e) {
        QsT[(dv + e) * VROW + qq] = qe[e];
        dOsT[(dv + e) * VROW + qq] = oe[e];
      }
    }
    if (tid < 32) lse_s[tid] = qt0 + tid < a.Lq ? LSE[qt0 + tid] : 0.f;
    else if (tid < 64) dl_s[tid - 32] = qt0 + tid - 32 < a.Lq ? DL[qt0 + tid - 32] : 0.f;
    __syncthreads();
    f32x16 sc, dp;
    zacc(sc); zacc(dp);
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      mm(sc, ld8(&Qs[c * KROW + s * 16 + 8 * hh]), kf[s]);
      mm(dp, ld8(&dOs[c * KROW + s * 16 + 8 * hh]), vf[s]);
    }
    f32x16 pp, ds;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int ql = qrow(r, hh), q = qt0 + ql;
      const bool ok = q < a.Lq && key < klen && (!a.causal || key <= q);
      const float p = ok ? exp2f(sc[r] * sl2 - lse_s[ql] * LOG2E) : 0.f;
      const float keep = (a.drop_p > 0.f && ok) ? drop.at(b * a.H + h, a.Lq, q, key) : 1.f;
      ds[r] = p * (dp[r] * keep - dl_s[ql]) * a.scale;
      pp[r] = p * keep;
    }
    const Frag pf0 = accfrag<0>(pp), pf1 = accfrag<1>(pp);
    const Frag sf0 = accfrag<0>(ds), sf1 = accfrag<1>(ds);
#pragma unroll
    for (int dt = 0; dt < 2; ++dt) {
      const float* ro = &dOsT[(dt * 32 + c) * VROW + 4 * hh];
      const float* rq = &QsT[(dt * 32 + c) * VROW + 4 * hh];
      const Frag a0 = ld4x2(ro, ro + 8), a1 = ld4x2(ro + 16, ro + 24);
      const Frag b0 = ld4x2(rq, rq + 8), b1 = ld4x2(rq + 16, rq + 24);
      if (dt == 0) { mm(dv0, a0, pf0); mm(dv0, a1, pf1); mm(dk0, b0, sf0); mm(dk0, b1, sf1); }
      else { mm(dv1, a0, pf0); mm(dv1, a1, pf1); mm(dk1, b0, sf0); mm(dk1, b1, sf1); }
    }
    // dQ = dS K : dS through LDS (row q, column key)
#pragma unroll
    for (int r = 0; r < 16; ++r) dsw[qrow(r, hh) * SROW + c] = from_f<float>(ds[r]);
    __syncthreads();
    f32x16 dq0, dq1;
    zacc(dq0); zacc(dq1);
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      const Frag sa = ld8(&dsw[c * SROW + s * 16 + 8 * hh]);
      mm(dq0, sa, ktf[0][s]);
      mm(dq1, sa, ktf[1][s]);
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      rw[qrow(r, hh) * 64 + c] = dq0[r];
      rw[qrow(r, hh) * 64 + 32 + c] = dq1[r];
    }
    __syncthreads();
    for (int e = tid; e < 32 * 64; e += 256) {
      const int qq = e >> 6, d = e & 63;
      const float v = red[e] + red[32 * 65 + e] + red[2 * 32 * 65 + e] + red[3 * 32 * 65 + e];
      if (qt0 + qq < a.Lq && v != 0.f) atomicAdd(a.dq + ((int64_t)b * a.Lq + qt0 + qq) * a.lddq + h * DH + d, v);
    }
  }
  __syncthreads();
  float* DK = (float*)a.dk + ((int64_t)b * a.Lk + kb0) * a.lddk + h * DH;
  store_t<float>(dk0, dk1, 1.f, rw, DK, a.lddk, a.Lk - kb0);
  __syncthreads();
  float* DV = (float*)a.dv + ((int64_t)b * a.Lk + kb0) * a.lddv + h * DH;
  store_t<float>(dv0, dv1, 1.f, rw, DV, a.lddv, a.Lk - kb0);
}
}  // namespace f32
int f32_fwd(const avsr_attn_params* p, const AttnArgs& a, hipStream_t st) {
  hipLaunchKernelGGL(f32::attn_fwd_kernel, dim3((p->Lq + 127) / 128, p->B * p->H), dim3(256), 0, st, a);
  return (int)hipGetLastError();
}
int f32_bwd(const avsr_attn_params* p, const AttnArgs& a, hipStream_t st) {
  hipLaunchKernelGGL(f32::attn_bwd_kernel, dim3((p->Lk + 127) / 128, p->B * p->H), dim3(256), 0, st, a);
  return (int)hipGetLastError();
}
}  // namespace attn
