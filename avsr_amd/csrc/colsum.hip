// Column sums of row-block partial workspaces (the bias and LayerNorm parameter gradients):
// colsum_launch (common.h) reduces one workspace at once or queues it, and the C-ABI
// avsr_colsum_defer / _inline / _flush (include/avsr_hip.h) drive the queue.
#include <vector>

#include "common.h"

namespace {

// Column sums of a row-block partial workspace: out[c] += sum_b ws[b*ld + c] for c < N, or,
// when out1 != nullptr, columns [N1, N) go to out1[c - N1] (LayerNorm dgamma/dbeta in one
// launch). Block = 32 columns (one 128-byte line per row) x 32 row lanes (1024 threads): each
// thread adds nb/32 partial rows with four independent accumulators, then the row lanes are
// summed in a fixed order (deterministic). (8 row lanes: ~6.7 us per 256 x 1024 workspace,
// a latency-bound chain of 32 loads per thread.)
constexpr int COLSUM_THREADS = 1024;
AVSR_DEV void colsum_block(const float* ws, int nb, int64_t ld, int N, float* out, int N1, float* out1, int cb) {
  __shared__ float red[32][33];
  const int cl = threadIdx.x & 31, rl = threadIdx.x >> 5;
  const int c = cb * 32 + cl;
  float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
  if (c < N) {
    int b = rl;
    for (; b + 96 < nb; b += 128) {
      s0 += ws[(int64_t)b * ld + c];
      s1 += ws[(int64_t)(b + 32) * ld + c];
      s2 += ws[(int64_t)(b + 64) * ld + c];
      s3 += ws[(int64_t)(b + 96) * ld + c];
    }
    for (; b < nb; b += 32) s0 += ws[(int64_t)b * ld + c];
  }
  red[rl][cl] = (s0 + s1) + (s2 + s3);
  __syncthreads();
  if (rl == 0 && c < N) {
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < 32; ++i) s += red[i][cl];
    if (out1 && c >= N1) out1[c - N1] += s;
    else out[c] += s;
  }
}
__global__ __launch_bounds__(COLSUM_THREADS) void colsum_finalize_kernel(const float* ws, int nb, int64_t ld, int N,
                                                                          float* out, int N1, float* out1) {
  colsum_block(ws, nb, ld, N, out, N1, out1, blockIdx.x);
}
dim3 colsum_grid(int N) { return dim3((N + 31) / 32); }

// ---- deferred column-sum finalisation (one launch per flush) ----------------------------
constexpr int COLSUM_BATCH = 32;
struct ColsumBatch {
  const float* ws[COLSUM_BATCH]; float* out[COLSUM_BATCH]; float* out1[COLSUM_BATCH];
  int64_t ld[COLSUM_BATCH]; int nb[COLSUM_BATCH], N[COLSUM_BATCH], N1[COLSUM_BATCH];
};
__global__ __launch_bounds__(COLSUM_THREADS) void colsum_batch_kernel(ColsumBatch b) {
  const int d = blockIdx.y;
  if ((int)blockIdx.x * 32 >= b.N[d]) return;          // block-uniform
  colsum_block(b.ws[d], b.nb[d], b.ld[d], b.N[d], b.out[d], b.N1[d], b.out1[d], blockIdx.x);
}
struct ColsumQueue { bool on = false, inl = false; std::vector<ColsumBatch> full; ColsumBatch cur; int n = 0; int maxn = 0; };
ColsumQueue g_colsum;

}  // namespace

int colsum_launch(const float* ws, int nb, int64_t ld, int N, float* out, int N1, float* out1, hipStream_t st) {
  if (!g_colsum.on || g_colsum.inl) {
    hipLaunchKernelGGL(colsum_finalize_kernel, colsum_grid(N), dim3(COLSUM_THREADS), 0, st, ws, nb, ld, N, out, N1, out1);
    AVSR_CHECK_LAUNCH();
    return 0;
  }
  ColsumQueue& q = g_colsum;
  const int i = q.n % COLSUM_BATCH;
  q.cur.ws[i] = ws; q.cur.nb[i] = nb; q.cur.ld[i] = ld; q.cur.N[i] = N; q.cur.out[i] = out; q.cur.N1[i] = N1;
  q.cur.out1[i] = out1;
  q.n++;
  q.maxn = q.maxn > N ? q.maxn : N;
  if (q.n % COLSUM_BATCH == 0) q.full.push_back(q.cur);
  return 0;
}

extern "C" int avsr_colsum_defer(int on) {
  const int was = g_colsum.on ? 1 : 0;
  g_colsum.on = on != 0;
  if (!g_colsum.on && g_colsum.n) {   // switched off with passes still queued (an aborted step):
    g_colsum.full.clear();            // drop them rather than reduce workspaces that may be gone
    g_colsum.n = 0; g_colsum.maxn = 0;
  }
  return was;
}

extern "C" int avsr_colsum_inline(int on) {
  const int was = g_colsum.inl ? 1 : 0;
  g_colsum.inl = on != 0;
  return was;
}

extern "C" int avsr_colsum_flush(void* stream) {
  ColsumQueue& q = g_colsum;
  hipStream_t st = (hipStream_t)stream;
  const dim3 gx = colsum_grid(q.maxn > 0 ? q.maxn : 1);
  for (const ColsumBatch& b : q.full) hipLaunchKernelGGL(colsum_batch_kernel, dim3(gx.x, COLSUM_BATCH), dim3(COLSUM_THREADS), 0, st, b);
  const int rest = q.n % COLSUM_BATCH;
  if (rest) hipLaunchKernelGGL(colsum_batch_kernel, dim3(gx.x, rest), dim3(COLSUM_THREADS), 0, st, q.cur);
  q.full.clear(); q.n = 0; q.maxn = 0;
  AVSR_CHECK_LAUNCH();
  return 0;
}
