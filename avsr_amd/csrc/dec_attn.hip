// The decoder's one-query attention of the beam search (declaration and avsr_dec_attn_params under
// "Joint CTC / attention beam search" in include/avsr_hip.h):
//   avsr_dec_attn          one-query multi-head attention per hypothesis over a K/V cache
// fp32 math; latency-bound: one workgroup per (group of hypotheses, head[, key chunk]).
#include "common.h"

namespace {

// block (hyp i, head h), 4 waves: a wave reads 4 keys per instruction (16 lanes x 4 elements
// per 64-wide row: coalesced 256-B rows), scores by 16-lane butterfly sums into LDS, block
// softmax, then o = sum_j p_j v_j with the same row-per-16-lanes reads, reduced over the 4 key
// slots of a wave (shuffles) and the 4 waves (LDS). Rows come through kmap (ancestry-indexed
// self-attention cache), kidx (batched memories) or directly.
template <typename T> AVSR_DEV f32x4 ld4(const T* p) {
  if constexpr (sizeof(T) == 2) {
    const bf16x4 v = *(const bf16x4*)p;
    return f32x4{(float)v[0], (float)v[1], (float)v[2], (float)v[3]};
  } else {
    return *(const f32x4*)p;
  }
}

// G hypotheses per workgroup (p.group; G = 1 for per-hypothesis keys): every key / value row is
// read once for the G queries of the group. 8 waves; key j of iteration it is handled by wave
// (j / 4) % 8, key slot j % 4 (16 lanes x 4 elements); each lane issues DA_UNROLL row loads
// back to back before using them, so a 375-key memory takes two load round trips per phase
// (the one-load-per-iteration loop was latency-bound: 51 us per call at 375 keys, G = 5).
constexpr int DA_WAVES = 8, DA_UNROLL = 8;
// Key split (p.ksplit >= 2, blockIdx.z): workgroup z of a (group, head) takes keys
// [z * chunk, (z + 1) * chunk) of its rows' klen, with nz = min(ksplit, ceil(klen / 192)) chunks
// (a function of klen alone, so a hypothesis's result never depends on the batch); it writes its
// per-query (max, sum of exp, unnormalised o) to p.ws and the last of the nz to arrive merges them
// in split order (write-through partials, drained before the counter add; Guideline 16).
constexpr int DA_SPLIT_KEYS = 192;
template <typename T, int G>
__global__ __launch_bounds__(64 * DA_WAVES) void dec_attn_kernel(avsr_dec_attn_params p) {
  constexpr int NW = DA_WAVES, U = DA_UNROLL, KS = 4 * NW;
  extern __shared__ float sc[];           // [G][kpad] scores, then [NW][G][64] partials
  __shared__ float shr[G][NW];
  __shared__ int last;
  const int h = blockIdx.x, i0 = blockIdx.y * G;
  const int klen = p.klen ? min(p.klen[i0], p.klen_max) : p.klen_max;
  const int kpad = (p.klen_max + 3) & ~3;
  const int nz = p.ksplit > 1 ? max(1, min(p.ksplit, (klen + DA_SPLIT_KEYS - 1) / DA_SPLIT_KEYS)) : 1;
  const int z = blockIdx.z;
  if (z >= nz) return;                    // (no arrival: the merge counts nz workgroups)
  const int chunk = (klen + nz - 1) / nz;
  const int jbeg = z * chunk, jend = min(klen, jbeg + chunk), jn = jend - jbeg;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, sub = lane >> 4, d0 = (lane & 15) * 4;
  const int kb = p.kmap ? 0 : (p.kidx ? p.kidx[i0] : i0);
  const T* K = (const T*)p.k + (int64_t)kb * p.k_bstride + h * 64 + d0;
  const T* Vv = (const T*)p.v + (int64_t)kb * p.v_bstride + h * 64 + d0;
  const int* km = p.kmap ? p.kmap + (int64_t)i0 * p.ldmap : nullptr;  // key j -> row km[j] (G == 1)
  const int ng = min(G, p.n - i0);
  const int jl = 4 * w + sub;             // this lane's key offset within an iteration
  auto rows_of = [&](int it0, int (&row)[U]) {
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int j = jbeg + (it0 + u) * KS + jl;
      row[u] = j < jend ? (km ? km[j] : j) : 0;
    }
  };
  f32x4 q[G];
#pragma unroll
  for (int g = 0; g < G; ++g) q[g] = ld4((const T*)p.q + (int64_t)(i0 + min(g, ng - 1)) * p.ldq + h * 64 + d0);
  float m[G];
#pragma unroll
  for (int g = 0; g < G; ++g) m[g] = -INFINITY;
  for (int it0 = 0; it0 * KS < jn; it0 += U) {
    int row[U];
    rows_of(it0, row);
    f32x4 k[U];
#pragma unroll
    for (int u = 0; u < U; ++u) k[u] = ld4(K + (int64_t)row[u] * p.ldk);
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int j = jbeg + (it0 + u) * KS + jl;
      const bool ok = j < jend;
#pragma unroll
      for (int g = 0; g < G; ++g) {
        float s = q[g][0] * k[u][0] + q[g][1] * k[u][1] + q[g][2] * k[u][2] + q[g][3] * k[u][3];
        s = row_sum16(s);               // over the key's 16 lanes (one DPP row)
        s *= p.scale;
        if (ok) {
          if ((lane & 15) == 0) sc[g * kpad + j] = s;
          m[g] = fmaxf(m[g], s);
        }
      }
    }
  }
  // block max of every group row (one barrier pair for all G)
#pragma unroll
  for (int g = 0; g < G; ++g) {
    const float v = wave_max(m[g]);
    if (lane == 0) shr[g][w] = v;
  }
  __syncthreads();
#pragma unroll
  for (int g = 0; g < G; ++g) {
    float v = shr[g][0];
#pragma unroll
    for (int x = 1; x < NW; ++x) v = fmaxf(v, shr[g][x]);
    m[g] = v;
  }
  __syncthreads();
  float l[G];
#pragma unroll
  for (int g = 0; g < G; ++g) {
    float lg = 0.f;
    for (int j = jbeg + threadIdx.x; j < jend; j += 64 * NW) {
      const float e = expf(sc[g * kpad + j] - m[g]);
      sc[g * kpad + j] = e;
      lg += e;
    }
    lg = wave_sum(lg);
    if (lane == 0) shr[g][w] = lg;
  }
  __syncthreads();                         // every score is final, every wave sum written
#pragma unroll
  for (int g = 0; g < G; ++g) {
    float v = shr[g][0];
#pragma unroll
    for (int x = 1; x < NW; ++x) v += shr[g][x];
    l[g] = v;
  }
  f32x4 acc[G];
#pragma unroll
  for (int g = 0; g < G; ++g) acc[g] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int it0 = 0; it0 * KS < jn; it0 += U) {
    int row[U];
    rows_of(it0, row);
    f32x4 v[U];
#pragma unroll
    for (int u = 0; u < U; ++u) v[u] = ld4(Vv + (int64_t)row[u] * p.ldv);
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int j = jbeg + (it0 + u) * KS + jl;
      const bool ok = j < jend;
#pragma unroll
      for (int g = 0; g < G; ++g) acc[g] += (ok ? sc[g * kpad + j] : 0.f) * v[u];
    }
  }
  float* part = sc + G * kpad;
#pragma unroll
  for (int g = 0; g < G; ++g) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      acc[g][e] += __shfl_xor(acc[g][e], 16, 64);
      acc[g][e] += __shfl_xor(acc[g][e], 32, 64);
    }
    if (sub == 0) *(f32x4*)&part[(w * G + g) * 64 + d0] = acc[g];
  }
  __syncthreads();
  if (nz == 1) {
    for (int t = threadIdx.x; t < ng * 64; t += 64 * NW) {
      const int g = t >> 6, d = t & 63;
      float o = 0.f;
#pragma unroll
      for (int x = 0; x < NW; ++x) o += part[(x * G + g) * 64 + d];
      ((T*)p.o)[(int64_t)(i0 + g) * p.ldo + h * 64 + d] = from_f<T>(o / l[g]);
    }
    return;
  }
  // split: this chunk's (o[64], max, sum) per query -> ws[(group, head)][z][g][66]
  const int64_t slot = (int64_t)blockIdx.y * gridDim.x + h;
  float* wz = p.ws + (slot * p.ksplit) * G * 66;
  for (int t = threadIdx.x; t < ng * 64; t += 64 * NW) {
    const int g = t >> 6, d = t & 63;
    float o = 0.f;
#pragma unroll
    for (int x = 0; x < NW; ++x) o += part[(x * G + g) * 64 + d];
    __hip_atomic_store(wz + ((int64_t)z * G + g) * 66 + d, o, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  if (threadIdx.x < ng) {
    const int g = threadIdx.x;
#pragma unroll
    for (int gg = 0; gg < G; ++gg)
      if (gg == g) {
        __hip_atomic_store(wz + ((int64_t)z * G + g) * 66 + 64, m[gg], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(wz + ((int64_t)z * G + g) * 66 + 65, l[gg], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // every storing wave: its partials are out
  __syncthreads();
  if (threadIdx.x == 0)
    last = __hip_atomic_fetch_add(&p.cnt[slot], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == (unsigned)nz - 1;
  __syncthreads();
  if (!last) return;
  for (int t = threadIdx.x; t < ng * 64; t += 64 * NW) {
    const int g = t >> 6, d = t & 63;
    auto ld = [&](int q, int e) {
      return __hip_atomic_load(wz + ((int64_t)q * G + g) * 66 + e, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    };
    float mx = -INFINITY;
    for (int q = 0; q < nz; ++q) mx = fmaxf(mx, ld(q, 64));
    float lsum = 0.f, o = 0.f;
    for (int q = 0; q < nz; ++q) {
      const float f = expf(ld(q, 64) - mx);
      lsum += ld(q, 65) * f;
      o += ld(q, d) * f;
    }
    ((T*)p.o)[(int64_t)(i0 + g) * p.ldo + h * 64 + d] = from_f<T>(o / lsum);
  }
  if (threadIdx.x == 0) __hip_atomic_store(&p.cnt[slot], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

}  // namespace

extern "C" int avsr_dec_attn(const avsr_dec_attn_params* p, void* stream) {
  if (!p || p->n <= 0 || p->H <= 0) return AVSR_E_ARG;
  if (p->klen_max <= 0 || p->klen_max > 16384) return AVSR_E_SHAPE;
  if (p->ldq % 4 || p->ldk % 4 || p->ldv % 4 || p->k_bstride % 4 || p->v_bstride % 4) return AVSR_E_ALIGN;
  const int G = p->group > 1 ? p->group : 1;
  if (G > 8 || (G > 1 && p->kmap)) return AVSR_E_ARG;
  const int kpad = (p->klen_max + 3) & ~3;
  const size_t lds = ((size_t)G * kpad + (size_t)DA_WAVES * G * 64) * sizeof(float);
  if (lds > 64 * 1024) return AVSR_E_SHAPE;
  const int ks = p->ksplit > 1 ? p->ksplit : 1;
  if (ks > 8 || (ks > 1 && (!p->ws || !p->cnt))) return AVSR_E_ARG;
  const dim3 g(p->H, (p->n + G - 1) / G, ks);
  hipStream_t st = (hipStream_t)stream;
#define DA(T_, G_) hipLaunchKernelGGL((dec_attn_kernel<T_, G_>), g, dim3(64 * DA_WAVES), lds, st, *p)
#define DAG(T_) switch (G) { case 1: DA(T_, 1); break; case 2: DA(T_, 2); break; case 3: DA(T_, 3); break;   \
                              case 4: DA(T_, 4); break; case 5: DA(T_, 5); break; case 6: DA(T_, 6); break;   \
                              case 7: DA(T_, 7); break; default: DA(T_, 8); }
  if (p->dtype == AVSR_BF16) { DAG(bf16) }
  else if (p->dtype == AVSR_F32) { DAG(float) }
  else return AVSR_E_DTYPE;
#undef DAG
#undef DA
  AVSR_CHECK_LAUNCH();
  return 0;
}
