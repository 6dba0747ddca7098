// The few-row (M <= 64) forward linears of avsr_gemm (gemm.hip chooses them) and the C-ABI
// avsr_gemm_skinny_splits. Elementwise epilogue: gemm_core.h.
#include "gemm_dense.h"
#include <algorithm>

using namespace gemmd;

namespace {

// ---------------------------------------------------------------- skinny (M <= 64) linears
// The decoder's per-step linears during beam search have n = utterances x beam rows (<= 40 at
// C5). The tiled cores put one 64 x 256 tile per 256 columns on them (4 workgroups for
// N = 1024, each streaming a 1 MiB weight slab; 63 us per call in fp32 parity mode). Here the
// work is spread over N / 16 workgroups and done with fp32 FMAs on the vector ALUs (exact
// fp32 products and sums, fixed order): a workgroup stages the A rows of a 256-wide K chunk in
// LDS (as fp32), thread (column pair cg, K lane kl) keeps partial sums of 2 columns for every
// row over k = 4kl + 128j .. +3 (one 16-byte weight load per column and k group, 4 FMAs per
// row), then the 32 K lanes are reduced (shuffles within a wave, LDS across the 4 waves) and
// the usual elementwise epilogue (bias / activation / residual / beta) writes the tile.
constexpr int SK_NB = 16;

template <typename T> AVSR_DEV f32x4 ld4f(const T* p) {
  if constexpr (sizeof(T) == 2) {
    const bf16x4 v = *(const bf16x4*)p;
    return f32x4{(float)v[0], (float)v[1], (float)v[2], (float)v[3]};
  } else {
    return *(const f32x4*)p;
  }
}

// K split (part != nullptr): block row blockIdx.y sums k in [y * kchunk, (y + 1) * kchunk) and
// writes the raw sums to part[y][m][n] (N / 16 workgroups alone leave most CUs idle at
// N = 1024); the last of the S workgroups of a column block to arrive (agent-scope counter
// cnt[blockIdx.x]) adds the S partials in a fixed order and runs the epilogue. Hand-off:
// partials stored write-through (sc1, relaxed agent-scope atomic stores), every storing wave
// drains its stores (s_waitcnt vmcnt(0)) before the barrier that precedes the counter add, the
// reducer reads them with sc1 loads (cdna_hip_programming.md Guideline 16, counter form) — no
// fence, no second launch; the reducer resets the counter (zero-initialised by the caller).
template <typename T, typename OutT, int MR>
__global__ __launch_bounds__(256) void skinny_kernel(DenseArgs a, float* part, int kchunk, unsigned* cnt) {
  constexpr int SK_KC = MR <= 32 ? 256 : 128;        // K chunk staged per pass (<= 33 KiB of LDS)
  constexpr int XPT = MR * SK_KC / 4 / 256;           // A vectors per thread per chunk
  constexpr int WJ = SK_KC / 128;                     // k groups per thread per chunk
  __shared__ __attribute__((aligned(16))) float xs[MR][SK_KC + 4];
  static_assert(4 * MR * (SK_NB + 1) <= MR * (SK_KC + 4), "reduction slab reuses the staging buffer");
  float (*red)[MR][SK_NB + 1] = (float (*)[MR][SK_NB + 1])&xs[0][0];
  const int tid = threadIdx.x, cg = tid & 7, kl = tid >> 3, lane = tid & 63, wave = tid >> 6;
  const int n0 = blockIdx.x * SK_NB, c0 = n0 + 2 * cg, c1 = c0 + 1;
  const T* A = (const T*)a.A;
  const T* B0 = (const T*)a.B + (int64_t)min(c0, a.N - 1) * a.ldb;
  const T* B1 = (const T*)a.B + (int64_t)min(c1, a.N - 1) * a.ldb;
  const bool ok0 = c0 < a.N, ok1 = c1 < a.N;
  float acc0[MR], acc1[MR];
#pragma unroll
  for (int m = 0; m < MR; ++m) acc0[m] = acc1[m] = 0.f;
  const int kbeg = part ? blockIdx.y * kchunk : 0;
  const int kend = part ? min(a.K, kbeg + kchunk) : a.K;
  // the next chunk's A rows and weights are loaded into registers while this chunk computes
  f32x4 xr[XPT], w0[WJ], w1[WJ];
  auto load = [&](int k0) {
#pragma unroll
    for (int i = 0; i < XPT; ++i) {
      const int idx = tid + 256 * i, m = idx / (SK_KC / 4), q = idx - m * (SK_KC / 4), k = k0 + 4 * q;
      xr[i] = (m < a.M && k < kend) ? ld4f(A + (int64_t)m * a.lda + k) : f32x4{0.f, 0.f, 0.f, 0.f};
    }
#pragma unroll
    for (int j = 0; j < WJ; ++j) {
      const int k = k0 + 4 * (kl + 32 * j);
      w0[j] = (ok0 && k < kend) ? ld4f(B0 + k) : f32x4{0.f, 0.f, 0.f, 0.f};
      w1[j] = (ok1 && k < kend) ? ld4f(B1 + k) : f32x4{0.f, 0.f, 0.f, 0.f};
    }
  };
  load(kbeg);
  for (int k0 = kbeg; k0 < kend; k0 += SK_KC) {
    __syncthreads();                                // the previous chunk's reads of xs are done
#pragma unroll
    for (int i = 0; i < XPT; ++i) {
      const int idx = tid + 256 * i, m = idx / (SK_KC / 4), q = idx - m * (SK_KC / 4);
      *(f32x4*)&xs[m][4 * q] = xr[i];
    }
    f32x4 wc0[WJ], wc1[WJ];
#pragma unroll
    for (int j = 0; j < WJ; ++j) { wc0[j] = w0[j]; wc1[j] = w1[j]; }
    __syncthreads();
    if (k0 + SK_KC < kend) load(k0 + SK_KC);
#pragma unroll
    for (int j = 0; j < WJ; ++j) {
      const int g = kl + 32 * j;
#pragma unroll
      for (int m = 0; m < MR; ++m) {
        const f32x4 x = *(const f32x4*)&xs[m][4 * g];
        acc0[m] = fmaf(x[0], wc0[j][0], acc0[m]); acc0[m] = fmaf(x[1], wc0[j][1], acc0[m]);
        acc0[m] = fmaf(x[2], wc0[j][2], acc0[m]); acc0[m] = fmaf(x[3], wc0[j][3], acc0[m]);
        acc1[m] = fmaf(x[0], wc1[j][0], acc1[m]); acc1[m] = fmaf(x[1], wc1[j][1], acc1[m]);
        acc1[m] = fmaf(x[2], wc1[j][2], acc1[m]); acc1[m] = fmaf(x[3], wc1[j][3], acc1[m]);
      }
    }
  }
  // sum over the 8 K lanes of a wave (lane bits 3-5), then over the 4 waves
#pragma unroll
  for (int m = 0; m < MR; ++m) {
#pragma unroll
    for (int o = 8; o < 64; o <<= 1) {
      acc0[m] += __shfl_xor(acc0[m], o, 64);
      acc1[m] += __shfl_xor(acc1[m], o, 64);
    }
  }
  __syncthreads();                                  // staging buffer -> reduction slab
  if (lane < 8) {
#pragma unroll
    for (int m = 0; m < MR; ++m) { red[wave][m][2 * cg] = acc0[m]; red[wave][m][2 * cg + 1] = acc1[m]; }
  }
  __syncthreads();
  for (int o = tid; o < MR * SK_NB; o += 256) {
    const int m = o / SK_NB, c = o - m * SK_NB, col = n0 + c;
    if (m < a.M && col < a.N) {
      const float v = (red[0][m][c] + red[1][m][c]) + (red[2][m][c] + red[3][m][c]);
      if (part) __hip_atomic_store(&part[((int64_t)blockIdx.y * a.M + m) * a.N + col], v, __ATOMIC_RELAXED,
                                   __HIP_MEMORY_SCOPE_AGENT);
      else epi_elems<T, OutT, 1>(a.e, m, col, &v);
    }
  }
  if (!part) return;
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // every storing wave: its partials are out
  __shared__ int last;
  __syncthreads();
  if (tid == 0)
    last = __hip_atomic_fetch_add(&cnt[blockIdx.x], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == gridDim.y - 1;
  __syncthreads();
  if (!last) return;
  const int S = gridDim.y;
  const int64_t MN = (int64_t)a.M * a.N;
  for (int o = tid; o < MR * SK_NB; o += 256) {
    const int m = o / SK_NB, c = o - m * SK_NB, col = n0 + c;
    if (m < a.M && col < a.N) {
      const float* pp = part + (int64_t)m * a.N + col;
      float v = __hip_atomic_load(pp, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      for (int s = 1; s < S; ++s) v += __hip_atomic_load(pp + s * MN, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      epi_elems<T, OutT, 1>(a.e, m, col, &v);
    }
  }
  if (tid == 0) __hip_atomic_store(&cnt[blockIdx.x], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// fp32 few-row linears on the fp32-input matrix cores (v_mfma_f32_16x16x4_f32: exact fp32
// products, fp32 accumulation): a workgroup = SKM_WAVES waves over one 16-column block and one K
// chunk; wave w takes the 16-k groups w, w + SKM_WAVES, ... of the chunk; per group a lane loads the
// 4 consecutive weights of its column (16 B) and, per 16-row tile, its row's 4 activations (16 B,
// L2-resident: no LDS staging), then 4 MFMAs per row tile; the chunk is one load batch (all loads
// in flight at once), and the waves' partials are summed in LDS in a fixed order. The decoder's
// weights arrive cold from HBM every step, so the grid is sized to occupy every CU
// (skinny_mma_splits: K chunks until N/16 x S >= 256); the S partials of a column block go
// through the last-arriver hand-off of skinny_kernel. A row's result never depends on M (rows are
// independent in the MFMA, the k order is fixed).
// The epilogue's bias / residual operands are read at the start, beside the weight loads.
// UNR = 4 where the grid exceeds one workgroup per CU (fewer registers, two per CU).
// LNP (LayerNorm prologue, a.ln_c1): the batch holds whole rows of the chunk, so each row's chunk
// mean and M2 (two passes over the registers, partials over the 4 lanes of a row and the 8 waves in
// a fixed order) come for free; split launches hand them over with the partial sums (a.lnst) and
// the last arriver combines them (Chan et al.'s pairwise formula, split order). Everything runs on
// x' = x - s with s = x[m][0], a per-row shift every chunk knows (x - s is exact in fp32 for values
// within a factor 2): the statistics give mean' = mean - s, the MFMAs x' against gamma o W, and the
// epilogue applies rstd * (acc - mean' * c1[n]). Without the shift a row whose |mean| is large next
// to its spread would subtract two large terms (acc ~ mean * c1) and lose the digits the
// reference's normalise-then-project keeps.
constexpr int SKM_WAVES = 8;
template <typename OutT, int MT, int UNR, bool LNP = false>
__global__ __launch_bounds__(64 * SKM_WAVES) void skinny_mma_kernel(DenseArgs a, float* part, int kchunk, unsigned* cnt) {
  constexpr int NW = SKM_WAVES, NE = (16 * MT * SK_NB + 64 * NW - 1) / (64 * NW);
  __shared__ __attribute__((aligned(16))) float red[NW][16 * MT][SK_NB + 1];
  __shared__ float st1[LNP ? NW : 1][16 * MT], st2[LNP ? NW : 1][16 * MT];
  __shared__ float rmean[LNP ? 16 * MT : 1], rrstd[LNP ? 16 * MT : 1];
  __shared__ int last;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, g = lane >> 4, c = lane & 15;
  const int n0 = blockIdx.x * SK_NB, col = n0 + c;
  const Epi& e = a.e;
  const bool fast = !e.bwd && !e.preact && e.drop_p == 0.f && e.beta == 0.f && !e.atomic;
  float pb[NE], pr[NE];
  if (fast) {
#pragma unroll
    for (int i = 0; i < NE; ++i) {
      const int o = tid + 64 * NW * i, m = o / SK_NB, cl = n0 + (o - m * SK_NB);
      const bool ok = o < 16 * MT * SK_NB && m < a.M && cl < a.N;
      pb[i] = ok && e.bias ? e.bias[cl] : 0.f;
      pr[i] = ok && e.res ? ((const float*)e.res)[(int64_t)m * e.ldr + cl] : 0.f;
    }
  }
  const bool cok = col < a.N;
  const float* Wr = (const float*)a.B + (int64_t)min(col, a.N - 1) * a.ldb + 4 * g;
  const float* Ar[MT];
  bool rok[MT];
#pragma unroll
  for (int t = 0; t < MT; ++t) {
    const int m = 16 * t + c;
    rok[t] = m < a.M;
    Ar[t] = (const float*)a.A + (int64_t)min(m, a.M - 1) * a.lda + 4 * g;
  }
  const int kbeg = part ? blockIdx.y * kchunk : 0, kend = part ? min(a.K, kbeg + kchunk) : a.K;
  const int ng = (kend - kbeg) / 16;                  // K % 16 == 0 (host-checked); kchunk % 16 == 0
  f32x4 acc[MT];
#pragma unroll
  for (int t = 0; t < MT; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
  // LNP: exactly one pass for every wave (ng <= NW * UNR, host-checked), so all reach its barrier
  for (int q0 = w; LNP ? q0 == w : q0 < ng; q0 += NW * UNR) {
    f32x4 b[UNR], x[UNR][MT];
#pragma unroll
    for (int u = 0; u < UNR; ++u) {
      const int q = q0 + NW * u;
      const bool ok = q < ng;
      const int k = kbeg + 16 * (ok ? q : 0);
      b[u] = (ok && cok) ? *(const f32x4*)(Wr + k) : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int t = 0; t < MT; ++t) x[u][t] = (ok && rok[t]) ? *(const f32x4*)(Ar[t] + k) : f32x4{0.f, 0.f, 0.f, 0.f};
    }
    if constexpr (LNP) {       // the batch holds the chunk's rows: chunk mean and M2 per row of x - s
      float sft[MT];
#pragma unroll
      for (int t = 0; t < MT; ++t) sft[t] = ((const float*)a.A)[(int64_t)min(16 * t + c, a.M - 1) * a.lda];
#pragma unroll
      for (int u = 0; u < UNR; ++u) {   // loads past the chunk stay 0 (they meet b = 0 and no statistic)
        const bool ok = q0 + NW * u < ng;
#pragma unroll
        for (int t = 0; t < MT; ++t)
#pragma unroll
          for (int e2 = 0; e2 < 4; ++e2) x[u][t][e2] = ok ? x[u][t][e2] - sft[t] : 0.f;
      }
      const float inv_n = 1.f / (float)(kend - kbeg);
#pragma unroll
      for (int t = 0; t < MT; ++t) {
        float s1 = 0.f;
#pragma unroll
        for (int u = 0; u < UNR; ++u) s1 += (x[u][t][0] + x[u][t][1]) + (x[u][t][2] + x[u][t][3]);
        s1 += __shfl_xor(s1, 16, 64);
        s1 += __shfl_xor(s1, 32, 64);
        if (g == 0) st1[w][16 * t + c] = s1;
      }
      __syncthreads();
#pragma unroll
      for (int t = 0; t < MT; ++t) {
        float sm = 0.f;
#pragma unroll
        for (int v = 0; v < NW; ++v) sm += st1[v][16 * t + c];
        const float mu = sm * inv_n;
        float s2 = 0.f;
#pragma unroll
        for (int u = 0; u < UNR; ++u) {
          if (q0 + NW * u >= ng) continue;
#pragma unroll
          for (int e2 = 0; e2 < 4; ++e2) { const float d = x[u][t][e2] - mu; s2 += d * d; }
        }
        s2 += __shfl_xor(s2, 16, 64);
        s2 += __shfl_xor(s2, 32, 64);
        if (g == 0) st2[w][16 * t + c] = s2;
      }
    }
#pragma unroll
    for (int u = 0; u < UNR; ++u)
#pragma unroll
      for (int t = 0; t < MT; ++t)
#pragma unroll
        for (int e2 = 0; e2 < 4; ++e2) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(x[u][t][e2], b[u][e2], acc[t], 0, 0, 0);
  }
  // acc[t][r] = this wave's partial of y[16t + 4g + r][n0 + c]; the waves' in a fixed order
#pragma unroll
  for (int t = 0; t < MT; ++t)
#pragma unroll
    for (int r = 0; r < 4; ++r) red[w][16 * t + 4 * g + r][c] = acc[t][r];
  __syncthreads();
  // row statistics of this chunk (LNP): mean and M2 over the waves' partials in a fixed order
  auto chunk_stats = [&](int m, float& mean, float& m2) {
    float sm = 0.f, sq = 0.f;
#pragma unroll
    for (int v = 0; v < NW; ++v) { sm += st1[v][m]; sq += st2[v][m]; }
    mean = sm / (float)(kend - kbeg);
    m2 = sq;
  };
  const int kvD = a.N / 3;
  auto epi = [&](int i, int m, int cl, float v) {
    if (fast) {                // epi_elems' arithmetic, operands already in registers
      float y = e.alpha * v;
      if (e.bias) y += pb[i];
      y = act_fwd_t<float>(e.act, y);
      if (e.res) y += pr[i];
      if (a.kvk && cl >= kvD) {  // K / V columns: appended to the cache at this step's rows
        const int64_t row = (int64_t)a.kvpos[m * a.kvposs] * a.kvrows + m;
        float* dst = cl < 2 * kvD ? a.kvk : a.kvv;
        dst[row * kvD + (cl < 2 * kvD ? cl - kvD : cl - 2 * kvD)] = y;
      } else {
        ((OutT*)e.C)[(int64_t)m * e.ldc + cl] = from_f<OutT>(y);
      }
    } else {
      epi_elems<float, OutT, 1>(a.e, m, cl, &v);
    }
  };
  if (!part) {
#pragma unroll
    for (int i = 0; i < NE; ++i) {
      const int o = tid + 64 * NW * i;
      if (o >= 16 * MT * SK_NB) break;
      const int m = o / SK_NB, cc = o - m * SK_NB, cl = n0 + cc;
      if (m < a.M && cl < a.N) {
        float v = (red[0][m][cc] + red[1][m][cc]) + (red[2][m][cc] + red[3][m][cc]);
        v += (red[4][m][cc] + red[5][m][cc]) + (red[6][m][cc] + red[7][m][cc]);
        if constexpr (LNP) {
          float mean, m2;
          chunk_stats(m, mean, m2);
          v = (1.f / sqrtf(m2 / (float)a.K + a.ln_eps)) * (v - mean * a.ln_c1[cl]);
        }
        epi(i, m, cl, v);
      }
    }
    return;
  }
  for (int o = tid; o < 16 * MT * SK_NB; o += 64 * NW) {
    const int m = o / SK_NB, cc = o - m * SK_NB, cl = n0 + cc;
    if (m < a.M && cl < a.N) {
      float v = (red[0][m][cc] + red[1][m][cc]) + (red[2][m][cc] + red[3][m][cc]);
      v += (red[4][m][cc] + red[5][m][cc]) + (red[6][m][cc] + red[7][m][cc]);
      __hip_atomic_store(&part[((int64_t)blockIdx.y * a.M + m) * a.N + cl], v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
  if constexpr (LNP) {         // this chunk's (mean, M2) per row, per column block and split
    if (tid < a.M) {
      float mean, m2;
      chunk_stats(tid, mean, m2);
      float* sp = a.lnst + (((int64_t)blockIdx.x * gridDim.y + blockIdx.y) * a.M + tid) * 2;
      __hip_atomic_store(sp, mean, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __hip_atomic_store(sp + 1, m2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // every storing wave: its partials are out
  __syncthreads();
  if (tid == 0)
    last = __hip_atomic_fetch_add(&cnt[blockIdx.x], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == gridDim.y - 1;
  __syncthreads();
  if (!last) return;
  const int S = gridDim.y;
  if constexpr (LNP) {         // combine the S chunks' (n, mean, M2) in split order
    if (tid < a.M) {
      const float* sp = a.lnst + ((int64_t)blockIdx.x * S * a.M + tid) * 2;
      float n = 0.f, mean = 0.f, m2 = 0.f;
      for (int q = 0; q < S; ++q) {
        const float nq = (float)(min(a.K, (q + 1) * kchunk) - q * kchunk);
        const float mq = __hip_atomic_load(sp + (int64_t)q * a.M * 2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const float vq = __hip_atomic_load(sp + (int64_t)q * a.M * 2 + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const float nn = n + nq, d = mq - mean;
        mean += d * (nq / nn);
        m2 += vq + d * d * (n * nq / nn);
        n = nn;
      }
      rmean[tid] = mean;
      rrstd[tid] = 1.f / sqrtf(m2 / (float)a.K + a.ln_eps);
    }
    __syncthreads();
  }
  const int64_t MN = (int64_t)a.M * a.N;
#pragma unroll
  for (int i = 0; i < NE; ++i) {
    const int o = tid + 64 * NW * i;
    if (o >= 16 * MT * SK_NB) break;
    const int m = o / SK_NB, cc = o - m * SK_NB, cl = n0 + cc;
    if (m < a.M && cl < a.N) {
      const float* pp = part + (int64_t)m * a.N + cl;
      float v = __hip_atomic_load(pp, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      for (int q = 1; q < S; ++q) v += __hip_atomic_load(pp + q * MN, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if constexpr (LNP) v = rrstd[m] * (v - rmean[m] * a.ln_c1[cl]);
      epi(i, m, cl, v);
    }
  }
  if (tid == 0) __hip_atomic_store(&cnt[blockIdx.x], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// K split count: enough block rows for >= 512 workgroups, chunks of >= 256 k, and S * 64 * N
// partials within AVSR_SKINNY_WS (S depends on N and K only, never on M: a row's result does
// not depend on how many rows share the launch).
int skinny_splits(int N, int K, int& kchunk) {
  const int nb = (N + SK_NB - 1) / SK_NB;
  int S = (512 + nb - 1) / nb;
  S = std::min(S, std::max(1, K / 256));
  S = std::min(S, (int)std::max<int64_t>(1, AVSR_SKINNY_WS / (64 * (int64_t)N)));
  kchunk = ((K + S - 1) / S + 255) / 256 * 256;
  return (K + kchunk - 1) / kchunk;
}

// the matrix-core kernel's split: enough K chunks for N/16 x S >= 256 workgroups (every CU pulls
// weights from HBM) and chunks of <= 1024 k (one load batch), chunks of >= 256 k, the partials
// plus the LayerNorm chunk statistics within AVSR_SKINNY_WS
int skinny_mma_splits(int N, int K, int& kchunk) {
  const int nb = (N + SK_NB - 1) / SK_NB;
  int S = std::max((256 + nb - 1) / nb, (K + 1023) / 1024);
  S = std::min(S, std::max(1, K / 256));
  while (S > 1 && (int64_t)S * 64 * N + (int64_t)nb * S * 64 * 2 > AVSR_SKINNY_WS) --S;
  kchunk = ((K + S - 1) / S + 15) / 16 * 16;
  return (K + kchunk - 1) / kchunk;
}

template <typename T, typename OutT>
int launch_skinny(const DenseArgs& a, float* ws, hipStream_t st) {
  int kchunk = a.K;
  // fp32 with 16-byte rows and 16-k groups: the matrix-core form
  const bool mma = sizeof(T) == 4 && a.K % 16 == 0 && a.lda % 4 == 0 && a.ldb % 4 == 0;
  const int S = ws ? (mma ? skinny_mma_splits(a.N, a.K, kchunk) : skinny_splits(a.N, a.K, kchunk)) : 1;
  float* part = S > 1 ? ws : nullptr;
  unsigned* cnt = S > 1 ? (unsigned*)(ws + AVSR_SKINNY_WS) : nullptr;   // AVSR_SKINNY_CNT counters
  const int nb = (a.N + SK_NB - 1) / SK_NB;
  if (S > 1 && nb > AVSR_SKINNY_CNT) return AVSR_E_SHAPE;
  const dim3 g((unsigned)nb, (unsigned)S);
  const int unr = nb * S > 256 ? 4 : 8;
  // the cache append and the LayerNorm prologue belong to the matrix-core kernel's fast epilogue
  const bool fast = mma && !a.e.bwd && !a.e.preact && a.e.drop_p == 0.f && a.e.beta == 0.f && !a.e.atomic;
  if (a.kvk && !fast) return AVSR_E_ARG;
  if (a.ln_c1 && !(fast && kchunk <= SKM_WAVES * unr * 16)) return AVSR_E_ARG;   // every chunk one load batch
  if constexpr (sizeof(T) == 4) {
    if (mma) {
      DenseArgs al = a;
      if (a.ln_c1 && S > 1) al.lnst = ws + (int64_t)S * a.M * a.N;   // chunk statistics after the partials
#define SKM(T_, LN_) do { if (unr == 4) hipLaunchKernelGGL((skinny_mma_kernel<OutT, T_, 4, LN_>), g, dim3(64 * SKM_WAVES), 0, st, al, part, kchunk, cnt); \
                          else hipLaunchKernelGGL((skinny_mma_kernel<OutT, T_, 8, LN_>), g, dim3(64 * SKM_WAVES), 0, st, al, part, kchunk, cnt); } while (0)
      // LayerNorm prologue: one row-tile count for every M: the per-row statistics / shift / epilogue
      // arithmetic of the MT = 1..3 instantiations compiled to different roundings (a row's result
      // then depended on how many rows shared the launch: batched decode != per-utterance by 1e-5, and
      // test_skinny_layernorm_prologue_every_row_alone failed); MT = 4 for all is batch-invariant
      if (a.ln_c1) SKM(4, true);
      else if (a.M <= 16) SKM(1, false);
      else if (a.M <= 32) SKM(2, false);
      else if (a.M <= 48) SKM(3, false);
      else SKM(4, false);
#undef SKM
      AVSR_CHECK_LAUNCH();
      return 0;
    }
  }
#define SKL(R) hipLaunchKernelGGL((skinny_kernel<T, OutT, R>), g, dim3(256), 0, st, a, part, kchunk, cnt)
  if (a.M <= 8) SKL(8);
  else if (a.M <= 16) SKL(16);
  else if (a.M <= 24) SKL(24);
  else if (a.M <= 32) SKL(32);
  else if (a.M <= 40) SKL(40);
  else if (a.M <= 48) SKL(48);
  else SKL(64);
#undef SKL
  AVSR_CHECK_LAUNCH();
  return 0;
}

}  // namespace

bool gemmd::skinny_ok(const avsr_gemm_params* p, int splits) {
  const int esz = p->dtype == AVSR_BF16 ? 2 : 4;
  return p->M <= 64 && p->a_kmajor && p->b_kmajor && p->batch == 1 && splits == 1 && !p->epi_bwd && !p->db &&
         (p->K % 4) == 0 && (p->lda % 4) == 0 && (p->ldb % 4) == 0 && ((uintptr_t)p->A % (4 * esz)) == 0 &&
         ((uintptr_t)p->B % (4 * esz)) == 0;
}

int gemmd::skinny_launch(const avsr_gemm_params* p, const DenseArgs& a, hipStream_t st) {
  float* sws = p->skinny_ws;          // optional K-split partials (AVSR_SKINNY_WS floats)
  if (p->dtype == AVSR_F32) return launch_skinny<float, float>(a, sws, st);
  return p->c_f32 ? launch_skinny<bf16, float>(a, sws, st) : launch_skinny<bf16, bf16>(a, sws, st);
}

extern "C" int avsr_gemm_skinny_splits(int dtype, int N, int K) {
  if (N <= 0 || K <= 0) return 1;
  int kchunk;
  if (dtype == AVSR_F32 && K % 16 == 0) return skinny_mma_splits(N, K, kchunk);
  return skinny_splits(N, K, kchunk);
}
