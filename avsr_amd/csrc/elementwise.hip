// Elementwise / data-movement kernels around the GEMMs (declarations, reference call sites:
// include/avsr_hip.h): the elementwise backward (dropout / activation masks with bias-gradient
// column partials) and dropout forward, padded-frame masking, decoder embedding + positional
// encoding, casts, and audio input packing.
// All HBM-bound: 16-byte vectors where the layout allows, grid-stride loops.
#include "common.h"

namespace {

struct EwArgs {
  int rows, N;
  const void* dy; int64_t lddy; void* out; int64_t ldout;
  const void* gate; int64_t ldgate; int act;
  float drop_p; uint64_t seed; float alpha; float* db; float* ws;
};

// block = 64 column vectors x 4 row lanes over a chunk of rows; column partial sums are
// reduced in LDS and written (plain stores) to ws[row_block][N], then colsum_finalize adds
// the row-block partials into db: no atomic contention, deterministic order.
template <typename T>
__global__ __launch_bounds__(256) void ew_bwd_kernel(EwArgs a) {
  constexpr int VE = VecW<T>::VE;
  __shared__ float red[4 * 64 * 8];
  const int nv = a.N / VE;
  const int cvl = threadIdx.x & 63, rl = threadIdx.x >> 6;
  const int cv = blockIdx.x * 64 + cvl;
  const int chunk = (a.rows + gridDim.y - 1) / gridDim.y;
  const int r0 = blockIdx.y * chunk, r1 = min(a.rows, r0 + chunk);
  float acc[VE];
#pragma unroll
  for (int j = 0; j < VE; ++j) acc[j] = 0.f;
  if (cv < nv) {
    for (int r = r0 + rl; r < r1; r += 4) {
      float d[VE], g[VE];
      ldv((const T*)a.dy + (int64_t)r * a.lddy + cv * VE, d);
      if (a.gate) ldv((const T*)a.gate + (int64_t)r * a.ldgate + cv * VE, g);
#pragma unroll
      for (int j = 0; j < VE; ++j) d[j] *= a.alpha;
      if (a.drop_p > 0.f) {
        const uint64_t i0 = (uint64_t)r * a.N + cv * VE;
        if constexpr (VE == 8) drop8(a.drop_p, a.seed, i0, d);
        else {
#pragma unroll
          for (int j = 0; j < VE; ++j) d[j] *= drop_scale(a.drop_p, a.seed, i0 + j);
        }
      }
#pragma unroll
      for (int j = 0; j < VE; ++j) {
        float v = d[j];
        if (a.gate) v *= act_bwd_t<T>(a.act, g[j]);
        acc[j] += v;
        d[j] = v;
      }
      if (a.out) stv((T*)a.out + (int64_t)r * a.ldout + cv * VE, d);
    }
  }
  if (!a.db) return;
#pragma unroll
  for (int j = 0; j < VE; ++j) red[(rl * 64 + cvl) * VE + j] = acc[j];
  __syncthreads();
  if (rl == 0 && cv < nv) {
#pragma unroll
    for (int j = 0; j < VE; ++j) {
      const float t = red[(0 * 64 + cvl) * VE + j] + red[(1 * 64 + cvl) * VE + j] + red[(2 * 64 + cvl) * VE + j] +
                      red[(3 * 64 + cvl) * VE + j];
      a.ws[(int64_t)blockIdx.y * a.N + cv * VE + j] = t;
    }
  }
}

template <typename T>
__global__ __launch_bounds__(256) void mask_rows_kernel(int B, int T_, int N, T* x, int64_t ldx, const int* len) {
  constexpr int VE = VecW<T>::VE;
  const int nv = N / VE;
  const int64_t total = (int64_t)B * T_ * nv;
  for (int64_t i = blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int64_t row = i / nv;
    const int b = (int)(row / T_), t = (int)(row % T_);
    if (t >= len[b]) {
      float z[VE];
#pragma unroll
      for (int j = 0; j < VE; ++j) z[j] = 0.f;
      stv(x + row * ldx + (i % nv) * VE, z);
    }
  }
}

template <typename T>
__global__ __launch_bounds__(256) void embed_kernel(avsr_embed_params p, int bwd) {
  constexpr int VE = VecW<T>::VE;
  const int nv = p.D / VE;
  const int64_t total = (int64_t)p.rows * nv;
  for (int64_t i = blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int r = (int)(i / nv), d0 = (int)(i % nv) * VE;
    const int tok = p.tok[r];
    const int pos = p.pe_row ? p.pe_row[(int64_t)r * p.pe_row_stride] : r % p.L;
    if (!bwd) {
      float e[VE], o[VE];
      ldv((const T*)p.table + (int64_t)tok * p.D + d0, e);
#pragma unroll
      for (int j = 0; j < VE; ++j) {
        float v = e[j] * p.scale + p.pe[(int64_t)pos * p.D + d0 + j];
        if (p.drop_p > 0.f) v *= drop_scale(p.drop_p, p.seed, (uint64_t)r * p.D + d0 + j);
        o[j] = v;
      }
      stv((T*)p.y + (int64_t)r * p.D + d0, o);
    }
  }
}

// embedding backward without atomics (deterministic): block r owns the table row of token
// tok[r] iff r is that token's first occurrence; it adds the row gradients of every occurrence
// in row order. Other blocks exit.
template <typename T>
__global__ __launch_bounds__(256) void embed_bwd_kernel(avsr_embed_params p) {
  constexpr int VE = VecW<T>::VE;
  const int r = blockIdx.x;
  const int tok = p.tok[r];
  __shared__ int seen;
  if (threadIdx.x == 0) seen = 0;
  __syncthreads();
  for (int q = threadIdx.x; q < r; q += 256)
    if (p.tok[q] == tok) seen = 1;
  __syncthreads();
  if (seen) return;
  const int nv = p.D / VE;
  for (int c = threadIdx.x; c < nv; c += 256) {
    const int d0 = c * VE;
    float acc[VE];
#pragma unroll
    for (int j = 0; j < VE; ++j) acc[j] = 0.f;
    for (int q = r; q < p.rows; ++q) {
      if (p.tok[q] != tok) continue;
      float g[VE];
      ldv((const T*)p.dy + (int64_t)q * p.D + d0, g);
#pragma unroll
      for (int j = 0; j < VE; ++j) {
        float v = g[j] * p.scale;
        if (p.drop_p > 0.f) v *= drop_scale(p.drop_p, p.seed, (uint64_t)q * p.D + d0 + j);
        acc[j] += v;
      }
    }
    float* dt = p.dtable + (int64_t)tok * p.D + d0;
#pragma unroll
    for (int j = 0; j < VE; ++j) dt[j] += acc[j];
  }
}

template <typename S, typename D>
__global__ __launch_bounds__(256) void cast_kernel(int rows, int cols, const S* src, int64_t lds, D* dst,
                                                   int64_t ldd, float alpha, float beta) {
  const int64_t c0 = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 4;
  if (c0 >= cols) return;
  for (int r = blockIdx.y; r < rows; r += gridDim.y) {
    const S* s = src + (int64_t)r * lds + c0;
    D* d = dst + (int64_t)r * ldd + c0;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      if (c0 + q < cols) {
        float v = alpha * to_f(s[q]);
        if (beta != 0.f) v += beta * to_f(d[q]);
        d[q] = from_f<D>(v);
      }
    }
  }
}

// contiguous n-element cast, 8 elements per thread per iteration (two 16-byte fp32 loads,
// one 16-byte bf16 store), grid-stride: the arena's fp32 master -> bf16 shadow refresh
// (428 M parameters: 1.7 GB read + 0.86 GB written, HBM-bound).
__global__ __launch_bounds__(256) void cast_flat_f32_bf16_kernel(int64_t n8, const float4* __restrict__ src,
                                                                 bf16x8* __restrict__ dst) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n8; i += (int64_t)gridDim.x * 256) {
    const float4 a = src[2 * i], b = src[2 * i + 1];
    bf16x8 o;
    o[0] = (bf16)a.x; o[1] = (bf16)a.y; o[2] = (bf16)a.z; o[3] = (bf16)a.w;
    o[4] = (bf16)b.x; o[5] = (bf16)b.y; o[6] = (bf16)b.z; o[7] = (bf16)b.w;
    dst[i] = o;
  }
}

// bf16 -> fp32 over 8-element vectors (the compressed gradient all-reduce's decompress,
// parallel.GradReducer(compress="bf16"))
__global__ __launch_bounds__(256) void cast_flat_bf16_f32_kernel(int64_t n8, const bf16x8* __restrict__ src,
                                                                 float4* __restrict__ dst) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n8; i += (int64_t)gridDim.x * 256) {
    const bf16x8 v = src[i];
    dst[2 * i] = float4{(float)v[0], (float)v[1], (float)v[2], (float)v[3]};
    dst[2 * i + 1] = float4{(float)v[4], (float)v[5], (float)v[6], (float)v[7]};
  }
}

template <typename T>
__global__ __launch_bounds__(256) void audio_pack_kernel(int B, int F, int T_, const float* a, T* out) {
  const int64_t total = (int64_t)B * T_ * F;
  for (int64_t i = blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int f = (int)(i % F);
    const int64_t bt = i / F;
    const int b = (int)(bt / T_), t = (int)(bt % T_);
    out[i] = from_f<T>(a[((int64_t)b * F + f) * T_ + t]);
  }
}

template <typename T>
int ew_launch(const avsr_ew_params* p, hipStream_t st) {
  constexpr int VE = VecW<T>::VE;
  if (p->N % VE) return AVSR_E_SHAPE;
  if (p->rows == 0) return 0;
  if (p->db && !p->ws) return AVSR_E_ARG;
  const int nv = p->N / VE;
  dim3 grid((nv + 63) / 64, 1);
  // ~4096 blocks (16 waves per CU) for latency hiding; at most AVSR_EW_ROWBLOCKS row blocks
  // of column partials for colsum_finalize
  int gy = 4096 / (int)grid.x;
  gy = gy < 16 ? 16 : (gy > AVSR_EW_ROWBLOCKS ? AVSR_EW_ROWBLOCKS : gy);
  gy = gy > p->rows ? p->rows : gy;
  grid.y = gy;
  EwArgs a;
  a.rows = p->rows; a.N = p->N; a.dy = p->dy; a.lddy = p->lddy; a.out = p->out; a.ldout = p->ldout;
  a.gate = p->gate; a.ldgate = p->ldgate; a.act = p->act; a.drop_p = p->drop_p; a.seed = p->seed;
  a.alpha = p->alpha; a.db = p->db; a.ws = p->ws;
  hipLaunchKernelGGL(ew_bwd_kernel<T>, grid, dim3(256), 0, st, a);
  AVSR_CHECK_LAUNCH();
  if (p->db) return colsum_launch((const float*)p->ws, (int)grid.y, (int64_t)p->N, p->N, p->db, 0, nullptr, st);
  return 0;
}

int embed_launch(const avsr_embed_params* p, int bwd, hipStream_t st) {
  if (!p) return AVSR_E_ARG;
  return avsr_by_dtype(p->dtype, [&](auto t) -> int {
    using T = decltype(t);
    constexpr int VE = VecW<T>::VE;
    if (p->D % VE) return AVSR_E_SHAPE;
    if (p->rows <= 0) return 0;
    if (bwd) hipLaunchKernelGGL(embed_bwd_kernel<T>, dim3(p->rows), dim3(256), 0, st, *p);
    else hipLaunchKernelGGL(embed_kernel<T>, dim3(avsr_grid((int64_t)p->rows * p->D / VE)), dim3(256), 0, st, *p, bwd);
    AVSR_CHECK_LAUNCH();
    return 0;
  });
}

}  // namespace

extern "C" int avsr_ew_bwd(const avsr_ew_params* p, void* stream) {
  if (!p) return AVSR_E_ARG;
  return avsr_by_dtype(p->dtype, [&](auto t) -> int { return ew_launch<decltype(t)>(p, (hipStream_t)stream); });
}

extern "C" int avsr_dropout_fwd(const avsr_ew_params* p, void* stream) {
  if (!p) return AVSR_E_ARG;
  return avsr_by_dtype(p->dtype, [&](auto t) -> int {
    if (!p->out) return AVSR_E_ARG;
    avsr_ew_params q = *p;
    q.gate = nullptr; q.db = nullptr;
    return ew_launch<decltype(t)>(&q, (hipStream_t)stream);
  });
}

extern "C" int avsr_mask_rows(int dtype, int B, int T, int N, void* x, int64_t ldx, const int* len, void* stream) {
  return avsr_by_dtype(dtype, [&](auto t) -> int {
    using E = decltype(t);
    constexpr int VE = VecW<E>::VE;
    if (N % VE || ldx % VE) return AVSR_E_ALIGN;
    const int g = avsr_grid((int64_t)B * T * N / VE);
    hipLaunchKernelGGL(mask_rows_kernel<E>, dim3(g), dim3(256), 0, (hipStream_t)stream, B, T, N, (E*)x, ldx, len);
    AVSR_CHECK_LAUNCH();
    return 0;
  });
}

extern "C" int avsr_embed_fwd(const avsr_embed_params* p, void* stream) { return embed_launch(p, 0, (hipStream_t)stream); }
extern "C" int avsr_embed_bwd(const avsr_embed_params* p, void* stream) { return embed_launch(p, 1, (hipStream_t)stream); }

extern "C" int avsr_cast(int sd, int dd, int rows, int cols, const void* src, int64_t lds, void* dst, int64_t ldd,
                         float alpha, float beta, void* stream) {
  if (rows <= 0 || cols <= 0) return 0;
  const int64_t gx = ((int64_t)cols + 1023) / 1024;
  int64_t gy = 4096 / gx;
  gy = gy < 1 ? 1 : (gy > rows ? rows : gy);
  gy = gy > 65535 ? 65535 : gy;
  const dim3 g((unsigned)gx, (unsigned)gy);
  hipStream_t st = (hipStream_t)stream;
  if (sd == AVSR_F32 && dd == AVSR_BF16) hipLaunchKernelGGL((cast_kernel<float, bf16>), dim3(g), dim3(256), 0, st, rows, cols, (const float*)src, lds, (bf16*)dst, ldd, alpha, beta);
  else if (sd == AVSR_F32 && dd == AVSR_F32) hipLaunchKernelGGL((cast_kernel<float, float>), dim3(g), dim3(256), 0, st, rows, cols, (const float*)src, lds, (float*)dst, ldd, alpha, beta);
  else if (sd == AVSR_BF16 && dd == AVSR_F32) hipLaunchKernelGGL((cast_kernel<bf16, float>), dim3(g), dim3(256), 0, st, rows, cols, (const bf16*)src, lds, (float*)dst, ldd, alpha, beta);
  else if (sd == AVSR_BF16 && dd == AVSR_BF16) hipLaunchKernelGGL((cast_kernel<bf16, bf16>), dim3(g), dim3(256), 0, st, rows, cols, (const bf16*)src, lds, (bf16*)dst, ldd, alpha, beta);
  else return AVSR_E_DTYPE;
  AVSR_CHECK_LAUNCH();
  return 0;
}

extern "C" int avsr_cast_flat(int sd, int dd, int64_t n, const void* src, void* dst, void* stream) {
  if (n <= 0) return 0;
  hipStream_t st = (hipStream_t)stream;
  if (sd == AVSR_F32 && dd == AVSR_BF16 && n % 8 == 0 && ((uintptr_t)src & 15) == 0 && ((uintptr_t)dst & 15) == 0) {
    const int64_t n8 = n / 8;
    int64_t g = (n8 + 255) / 256;
    g = g > 256 * 32 ? 256 * 32 : g;           // 32 waves-worth of blocks per CU, grid-stride
    hipLaunchKernelGGL(cast_flat_f32_bf16_kernel, dim3((unsigned)g), dim3(256), 0, st, n8, (const float4*)src, (bf16x8*)dst);
    AVSR_CHECK_LAUNCH();
    return 0;
  }
  if (sd == AVSR_BF16 && dd == AVSR_F32 && n % 8 == 0 && ((uintptr_t)src & 15) == 0 && ((uintptr_t)dst & 15) == 0) {
    const int64_t n8 = n / 8;
    int64_t g = (n8 + 255) / 256;
    g = g > 256 * 32 ? 256 * 32 : g;
    hipLaunchKernelGGL(cast_flat_bf16_f32_kernel, dim3((unsigned)g), dim3(256), 0, st, n8, (const bf16x8*)src, (float4*)dst);
    AVSR_CHECK_LAUNCH();
    return 0;
  }
  // general case: a [rows][4096] view of the flat buffer plus a tail row
  const int64_t cols = 4096, rows = n / cols, tail = n - rows * cols;
  const size_t es = sd == AVSR_F32 ? 4 : 2, ed = dd == AVSR_F32 ? 4 : 2;
  if (rows > 0) {
    const int rc = avsr_cast(sd, dd, (int)rows, (int)cols, src, cols, dst, cols, 1.f, 0.f, stream);
    if (rc) return rc;
  }
  if (tail > 0) return avsr_cast(sd, dd, 1, (int)tail, (const char*)src + rows * cols * es, tail,
                                 (char*)dst + rows * cols * ed, tail, 1.f, 0.f, stream);
  return 0;
}

extern "C" int avsr_audio_pack(int dtype, int B, int F, int T, const float* audio, void* out, void* stream) {
  return avsr_by_dtype(dtype, [&](auto t) -> int {
    using E = decltype(t);
    const int g = avsr_grid((int64_t)B * T * F);
    hipLaunchKernelGGL(audio_pack_kernel<E>, dim3(g), dim3(256), 0, (hipStream_t)stream, B, F, T, audio, (E*)out);
    AVSR_CHECK_LAUNCH();
    return 0;
  });
}
