// Row log-softmax and top-k of the beam search (declarations under "Joint
// CTC / attention beam search" in include/avsr_hip.h):
//   avsr_log_softmax_rows  log_softmax over V (decoder output layer, CTC log-probs)
//   avsr_row_topk          pre-beam: top-P decoder tokens per hypothesis
//   avsr_log_softmax_topk  both in one pass over a row held in registers (decode steps)
// All fp32 math; decode runs at batch 1 utterance x beam hypotheses, so these kernels are
// latency-bound: one block per row / hypothesis, no host round trip inside a step.
#include "decode.h"

namespace {

AVSR_DEV float block_max256(float v, float* sh) {
  v = wave_max(v);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  v = fmaxf(fmaxf(sh[0], sh[1]), fmaxf(sh[2], sh[3]));
  __syncthreads();
  return v;
}
AVSR_DEV float block_sum256(float v, float* sh) {
  v = wave_sum(v);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  v = sh[0] + sh[1] + sh[2] + sh[3];
  __syncthreads();
  return v;
}

// ---------------------------------------------------------------- log_softmax rows
template <typename T>
__global__ __launch_bounds__(256) void log_softmax_kernel(int V, const T* x, int64_t ldx, float* out, int64_t ldo) {
  __shared__ float sh[4];
  const T* r = x + (int64_t)blockIdx.x * ldx;
  float m = -INFINITY;
  for (int c = threadIdx.x; c < V; c += 256) m = fmaxf(m, to_f(r[c]));
  m = block_max256(m, sh);
  float s = 0.f;
  for (int c = threadIdx.x; c < V; c += 256) s += expf(to_f(r[c]) - m);
  s = block_sum256(s, sh);
  const float ls = logf(s);
  float* o = out + (int64_t)blockIdx.x * ldo;
  for (int c = threadIdx.x; c < V; c += 256) o[c] = to_f(r[c]) - m - ls;
}

// ---------------------------------------------------------------- pre-beam top-P
// one block per hypothesis row; P rounds of block arg-max over per-thread sorted candidate
// lists (each thread keeps its own top-P of a strided slice)
__global__ __launch_bounds__(256) void row_topk_kernel(avsr_topk_params p) {
  __shared__ float shv[4];
  __shared__ int shi[4];
  const float* x = p.x + (int64_t)blockIdx.x * p.ldx;   // one row per block
  float tv[KMAX];
  int ti[KMAX];
#pragma unroll
  for (int k = 0; k < KMAX; ++k) { tv[k] = -INFINITY; ti[k] = 0x7fffffff; }
  for (int c = threadIdx.x; c < p.V; c += 256) {
    float v = x[c];
    int id = c;
    // insertion into the descending list (ties keep the smaller index first)
#pragma unroll
    for (int k = 0; k < KMAX; ++k) {
      if (k < p.K && (v > tv[k] || (v == tv[k] && id < ti[k]))) {
        const float t = tv[k]; const int u = ti[k];
        tv[k] = v; ti[k] = id; v = t; id = u;
      }
    }
  }
  int head = 0;
  for (int r = 0; r < p.K; ++r) {
    float v = -INFINITY; int id = 0x7fffffff;
#pragma unroll
    for (int k = 0; k < KMAX; ++k) if (k == head) { v = tv[k]; id = ti[k]; }
    const int mine = id;
    block_argmax256(v, id, shv, shi);
    if (threadIdx.x == 0) p.ids[(int64_t)blockIdx.x * p.K + r] = id;
    if (mine == id && id != 0x7fffffff) ++head;
  }
}

// log_softmax_rows + row_topk of the decoder output in one pass (decode steps): the row stays
// in registers (<= 24 values per thread, V <= 6144), the log-probs are written once and the
// top-K runs on the same register values. Per-thread element order, the block reductions and
// top-K order (value desc, index asc) equal the two separate kernels', so the output is
// identical to them.
constexpr int LSM_TOPK_NV = 24;
template <typename T>
__global__ __launch_bounds__(256) void log_softmax_topk_kernel(int V, int K, const T* x, int64_t ldx, float* out,
                                                               int64_t ldo, int* ids) {
  __shared__ float sh[4];
  __shared__ float shv[4];
  __shared__ int shi[4];
  const T* r = x + (int64_t)blockIdx.x * ldx;
  float v[LSM_TOPK_NV];
#pragma unroll
  for (int q = 0; q < LSM_TOPK_NV; ++q) {
    const int c = threadIdx.x + q * 256;
    v[q] = c < V ? to_f(r[c]) : -INFINITY;
  }
  float m = -INFINITY;
#pragma unroll
  for (int q = 0; q < LSM_TOPK_NV; ++q) m = fmaxf(m, v[q]);
  m = block_max256(m, sh);
  float s = 0.f;
#pragma unroll
  for (int q = 0; q < LSM_TOPK_NV; ++q)
    if (threadIdx.x + q * 256 < V) s += expf(v[q] - m);
  s = block_sum256(s, sh);
  const float ls = logf(s);
  float* o = out + (int64_t)blockIdx.x * ldo;
#pragma unroll
  for (int q = 0; q < LSM_TOPK_NV; ++q) {
    const int c = threadIdx.x + q * 256;
    if (c < V) { v[q] = v[q] - m - ls; o[c] = v[q]; }
  }
  // top-K by K rounds of "largest element below the previous pick" in the order (value desc,
  // index asc) -- the order row_topk's insertion lists produce, so the ids are the same; a
  // round is one register scan plus a block arg-max (the unrolled 24 x 16 insertion network
  // with its divergent swaps took ~30 us per call)
  // Each wave first takes the top-K of its own elements (rounds of wave arg-max, DPP only, no
  // barrier); the block's top-K is among those 4K candidates, which wave 0 then ranks the same way
  // (one barrier instead of two per round).
  __shared__ float cv[4 * KMAX];
  __shared__ int ci[4 * KMAX];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  float pv = INFINITY;
  int pi = -1;
  for (int rr = 0; rr < K; ++rr) {
    float bv = -INFINITY; int bi = 0x7fffffff;
#pragma unroll
    for (int q = 0; q < LSM_TOPK_NV; ++q) {
      const int c = threadIdx.x + q * 256;
      const bool below = c < V && (v[q] < pv || (v[q] == pv && c > pi));
      if (below && (v[q] > bv || bi == 0x7fffffff)) { bv = v[q]; bi = c; }
    }
    dwave_argmax(bv, bi);
    if (lane == 0) { cv[wv * KMAX + rr] = bv; ci[wv * KMAX + rr] = bi; }
    pv = bv; pi = bi;
  }
  __syncthreads();
  if (wv != 0) return;
  const bool have = lane < 4 * KMAX && (lane % KMAX) < K;
  const float mv = have ? cv[lane] : -INFINITY;
  const int mi = have ? ci[lane] : 0x7fffffff;
  pv = INFINITY; pi = -1;
  for (int rr = 0; rr < K; ++rr) {
    const bool below = have && mi != 0x7fffffff && (mv < pv || (mv == pv && mi > pi));
    float bv = below ? mv : -INFINITY; int bi = below ? mi : 0x7fffffff;
    dwave_argmax(bv, bi);
    if (lane == 0) ids[(int64_t)blockIdx.x * K + rr] = bi;
    pv = bv; pi = bi;
  }
}

}  // namespace

extern "C" int avsr_log_softmax_rows(int dtype, int rows, int V, const void* x, int64_t ldx, float* out, int64_t ldo,
                                     void* stream) {
  if (rows <= 0) return 0;
  if (V <= 0 || !x || !out) return AVSR_E_ARG;
  if (dtype == AVSR_BF16)
    hipLaunchKernelGGL(log_softmax_kernel<bf16>, dim3(rows), dim3(256), 0, (hipStream_t)stream, V, (const bf16*)x, ldx, out, ldo);
  else if (dtype == AVSR_F32)
    hipLaunchKernelGGL(log_softmax_kernel<float>, dim3(rows), dim3(256), 0, (hipStream_t)stream, V, (const float*)x, ldx, out, ldo);
  else return AVSR_E_DTYPE;
  AVSR_CHECK_LAUNCH();
  return 0;
}

extern "C" int avsr_row_topk(const avsr_topk_params* p, void* stream) {
  if (!p || p->rows <= 0) return p ? 0 : AVSR_E_ARG;
  if (p->K < 1 || p->K > KMAX || p->K > p->V) return AVSR_E_SHAPE;
  hipLaunchKernelGGL(row_topk_kernel, dim3(p->rows), dim3(256), 0, (hipStream_t)stream, *p);
  AVSR_CHECK_LAUNCH();
  return 0;
}

extern "C" int avsr_log_softmax_topk(int dtype, int rows, int V, const void* x, int64_t ldx, float* out,
                                     int64_t ldo, int K, int* ids, void* stream) {
  if (rows <= 0) return 0;
  if (V <= 0 || !x || !out || !ids) return AVSR_E_ARG;
  if (K < 1 || K > KMAX || K > V) return AVSR_E_SHAPE;
  if (V > LSM_TOPK_NV * 256) {             // row does not fit the registers: the two passes
    const int e = avsr_log_softmax_rows(dtype, rows, V, x, ldx, out, ldo, stream);
    if (e) return e;
    avsr_topk_params tp{rows, V, K, out, ldo, ids};
    return avsr_row_topk(&tp, stream);
  }
  if (dtype == AVSR_BF16)
    hipLaunchKernelGGL(log_softmax_topk_kernel<bf16>, dim3(rows), dim3(256), 0, (hipStream_t)stream, V, K,
                       (const bf16*)x, ldx, out, ldo, ids);
  else if (dtype == AVSR_F32)
    hipLaunchKernelGGL(log_softmax_topk_kernel<float>, dim3(rows), dim3(256), 0, (hipStream_t)stream, V, K,
                       (const float*)x, ldx, out, ldo, ids);
  else return AVSR_E_DTYPE;
  AVSR_CHECK_LAUNCH();
  return 0;
}
