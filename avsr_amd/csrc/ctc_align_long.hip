// avsr_ctc_align_long (include/avsr_hip.h): the CTC Viterbi of avsr_ctc_align for label sequences
// of up to 16383 tokens (S = 2L + 1 <= 32767 states), for whole recordings (avsr_amd/longform.py).
//   One workgroup of 1024 threads per recording. The DP row lives in REGISTERS, not in LDS:
//   thread i owns the P contiguous states [i P, i P + P) (P = 4 / 8 / 16 / 32, a template
//   parameter chosen from 2 Lmax + 1, so every array below is statically indexed): their d, the
//   P/2 label ids (P is even, so a thread's even states are blanks and share one emission) and the
//   P/2 skip flags as a bit mask. A frame is P max-of-three steps per thread on registers; the only
//   value a thread needs from another one is its left neighbour's last d (the state s - 1 of its
//   first state; s - 2 is a blank's skip, which does not exist), which goes through a one-float
//   LDS halo, double-buffered by frame parity: ONE barrier per frame. An LDS row, as in
//   ctc_align_kernel, would be three LDS reads and one write per STATE and frame (0.5 MB of LDS
//   traffic a frame at 32767 states, on one CU), and its two rows (256 KB) exceed a CU's LDS.
//   Emissions: a thread gathers its P/2 label logits, the blank logit and the row lse of a frame
//   D frames ahead into registers; no LDS-DMA is pending, so the frame's barrier waits for LDS
//   only and the gathers stay in flight across it.
//   Back-pointers: 2 bits per (frame, state). A thread's P pointers of a frame are P/4 whole
//   bytes at byte i P/4 of the frame's row (one byte, one ushort, one dword or two dwords per
//   thread, coalesced); rows are padded to 16 bytes.
//   Backtrack, the structure of ctc_align_kernel's: a path moves at most 2 states a frame, so for
//   a chunk of n frames that ends in state s only the columns [s - 2(n - 1), s] matter; the block
//   copies that window of the chunk's rows to LDS as dwords (16 states each), one lane walks it,
//   the block writes the chunk's tokens together.
// avsr_ctc_align_gaps is the same kernel with GAPS = true: flagged blank states may read a frame as
//   the caller's filler (free ends and gaps for transcripts that cover part of a recording).
#include "common.h"
#include <type_traits>

namespace {

constexpr float NINF = -__builtin_inff();
constexpr int NT = 1024;                    // threads per workgroup
constexpr int BT_FRAMES = 256;              // frames per backtrack chunk
constexpr int BT_W = BT_FRAMES / 8 + 2;     // dwords of a pointer row that a chunk's path can touch

// bytes of one frame's pointer row: 2 bits per state, padded to 16 bytes
__host__ __device__ inline int row_bytes(int Lmax) { return ((2 * Lmax + 1 + 63) >> 6) << 4; }

// GAPS: avsr_ctc_align_gaps. A flagged blank state may emit filler[t] + gap_penalty instead of the
// blank's log-probability; everything it adds is behind `if constexpr (GAPS)`, so the GAPS = false
// instantiations are the code of before.
template <bool GAPS>
using params_t = std::conditional_t<GAPS, avsr_ctc_align_gaps_params, avsr_ctc_align_params>;

template <typename T, int P, int D, bool GAPS>
__global__ __launch_bounds__(NT) void ctc_align_long_kernel(params_t<GAPS> p) {
  constexpr int H = P / 2;                  // labels per thread
  const int b = blockIdx.x, tid = threadIdx.x;
  const int L = p.label_len[b], Tb = min(p.in_len[b], p.T), S = 2 * L + 1;
  const int RB = row_bytes(p.Lmax);
  const int* lab = p.labels + (int64_t)b * p.Lmax;
  const T* X = (const T*)p.x + (int64_t)b * p.T * p.ldx;
  const float* LSE = p.lse + (int64_t)b * p.T;
  unsigned char* BP = p.ws + (int64_t)b * p.T * RB;
  int* ALI = p.ali + (int64_t)b * p.T;
  __shared__ float halo[2][NT + 1];         // cell i + 1: thread i's last d; cell 0 stays -inf
  __shared__ uint32_t win[BT_FRAMES * BT_W];
  __shared__ int path[BT_FRAMES];
  __shared__ float fin[2];
  __shared__ int bad, cur_s;
  if (tid == 0) { bad = 0; halo[0][0] = halo[1][0] = NINF; }
  __syncthreads();
  const bool shape_ok = L >= 0 && L <= p.Lmax && Tb > 0;
  const int s0 = tid * P, l0 = tid * H;     // first state, first label of this thread
  const bool active = shape_ok && s0 < S;
  uint32_t ko[H];                           // byte offset of each label's logit in a row of x
  uint32_t skipm = 0;                       // bit h: the label state 2h + 1 may be entered from s - 2
  uint32_t gapm = 0;                        // GAPS, bit h: the blank state 2h (position l0 + h) is a gap state
  if (shape_ok) {
    bool mybad = false;
    int prev = p.blank;
    if (l0 >= 1 && l0 - 1 < L) prev = lab[l0 - 1];
#pragma unroll
    for (int h = 0; h < H; ++h) {
      int k = p.blank;
      if (l0 + h < L) {
        k = lab[l0 + h];
        if (k < 0 || k >= p.V) { mybad = true; k = p.blank; }
        if (l0 + h >= 1 && k != p.blank && k != prev) skipm |= 1u << h;
      }
      ko[h] = (uint32_t)k * (uint32_t)sizeof(T);
      prev = k;
    }
    if (mybad) bad = 1;
    if constexpr (GAPS) {
      const unsigned char* gap = p.gap + (int64_t)b * (p.Lmax + 1);
#pragma unroll
      for (int h = 0; h < H; ++h)
        if (l0 + h <= L && gap[l0 + h]) gapm |= 1u << h;      // position L is state S - 1
    }
  }
  __syncthreads();
  auto infeasible = [&]() {
    for (int t = tid; t < p.T; t += NT) ALI[t] = -1;
    if (tid == 0) { p.score[b] = 0.f; p.feasible[b] = 0; }
  };
  if (!shape_ok || bad) { infeasible(); return; }

  // emissions of D frames in registers: slot u holds frame t with t % D == u
  float ex[D][H], eb[D], el[D];
  float eg[GAPS ? D : 1];                   // GAPS: the frame's filler
  auto fetch = [&](int f, int u) {
    if (!active) return;
    f = min(f, Tb - 1);                     // clamped, not branched around: never out of bounds
    const T* row = X + (int64_t)f * p.ldx;
    // buffer loads: the row's descriptor is scalar and a gather is one 32-bit lane offset (as
    // flat loads the compiler kept a 64-bit address pair per label and spilled at P = 32)
    const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<T*>(row), (short)0,
                                                                          p.V * (int)sizeof(T), 0x00020000);
#pragma unroll
    for (int h = 0; h < H; ++h) {
      if constexpr (sizeof(T) == 2) ex[u][h] = to_f(__builtin_bit_cast(bf16, __builtin_amdgcn_raw_buffer_load_b16(rs, ko[h], 0, 0)));
      else ex[u][h] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rs, ko[h], 0, 0));
    }
    eb[u] = to_f(row[p.blank]);
    el[u] = LSE[f];
    if constexpr (GAPS) eg[u] = p.filler[(int64_t)b * p.T + f];
  };
  float d[P];
#pragma unroll
  for (int u = 0; u < D; ++u) fetch(u, u);
  for (int tb = 0; tb < Tb; tb += D) {
#pragma unroll
    for (int u = 0; u < D; ++u) {
      const int t = tb + u;
      if (t < Tb) {                         // uniform over the block
        if (active) {
          const float lse = el[u], ebk = eb[u] - lse;
          float egm = ebk;                  // GAPS: what a gap state emits, ef where ef > eb (strictly)
          if constexpr (GAPS) {
            const float egk = eg[u] + p.gap_penalty;
            if (egk > ebk) egm = egk;
          }
          if (t == 0) {
#pragma unroll
            for (int j = 0; j < P; ++j) d[j] = NINF;
            if (tid == 0) {
              d[0] = ebk;
              if constexpr (GAPS) if (gapm & 1u) d[0] = egm;
              if (S > 1) d[1] = ex[u][0] - lse;
            }
          } else {
            const float left = halo[(t - 1) & 1][tid];
            uint32_t bits[2] = {0u, 0u};
            // downwards, so that d[j - 1] and d[j - 2] are still those of frame t - 1
#pragma unroll
            for (int j = P - 1; j >= 0; --j) {
              const float c1 = j >= 1 ? d[j - 1] : left;
              float m = d[j];
              uint32_t k = 0;
              if (c1 > m) { m = c1; k = 1; }
              float es = ebk;
              if constexpr (GAPS) if (!(j & 1) && ((gapm >> (j >> 1)) & 1u)) es = egm;
              if (j & 1) {
                const float c2r = j >= 2 ? d[j - 2] : left;
                const float c2 = (skipm >> (j >> 1)) & 1u ? c2r : NINF;
                if (c2 > m) { m = c2; k = 2; }
                es = ex[u][j >> 1] - lse;
              }
              d[j] = m + es;                // -inf stays -inf: an unreachable state never wins, no NaN
              bits[j >> 4] |= k << ((j & 15) * 2);
            }
            unsigned char* bp = BP + (int64_t)t * RB;
            if constexpr (P == 4) bp[tid] = (unsigned char)bits[0];
            else if constexpr (P == 8) ((unsigned short*)bp)[tid] = (unsigned short)bits[0];
            else if constexpr (P == 16) ((uint32_t*)bp)[tid] = bits[0];
            else ((uint2*)bp)[tid] = make_uint2(bits[0], bits[1]);
          }
          halo[t & 1][tid + 1] = d[P - 1];
        }
        __syncthreads();
      }
      fetch(t + D, u);
    }
  }
  if (active) {
#pragma unroll
    for (int j = 0; j < P; ++j) {
      if (s0 + j == S - 1) fin[1] = d[j];
      if (s0 + j == S - 2) fin[0] = d[j];
    }
  }
  __syncthreads();                          // also: every back-pointer store is visible to the block
  if (tid == 0) {
    const bool hi = S == 1 || fin[1] > fin[0];
    const float v = hi ? fin[1] : fin[0];
    const bool ok = v > NINF;
    cur_s = ok ? (hi ? S - 1 : S - 2) : -1;
    if (ok) { p.score[b] = v; p.feasible[b] = 1; }
  }
  __syncthreads();
  if (cur_s < 0) { infeasible(); return; }
  for (int t = Tb + tid; t < p.T; t += NT) ALI[t] = -1;
  for (int t1 = Tb - 1; t1 >= 0; t1 -= BT_FRAMES) {
    const int c0 = max(0, t1 - BT_FRAMES + 1), n = t1 - c0 + 1;
    const int sc = cur_s;
    const int w0 = max(0, sc - 2 * (n - 1)) >> 4, W = (sc >> 4) - w0 + 1;     // W <= BT_W
    for (int i = tid; i < n * W; i += NT) {
      const int r = i / W, c = i - r * W;
      win[i] = ((const uint32_t*)(BP + (int64_t)(c0 + r) * RB))[w0 + c];
    }
    __syncthreads();
    if (tid == 0) {
      int s = sc;
      for (int t = t1; t >= c0; --t) {
        path[t - c0] = s;
        if (t > 0) s = max(s - (int)((win[(t - c0) * W + (s >> 4) - w0] >> ((s & 15) * 2)) & 3u), 0);   // frame 0 has no pointers
      }
      cur_s = s;
    }
    __syncthreads();
    for (int i = tid; i < n; i += NT) {
      const int s = path[i];
      int tok = (s & 1) ? lab[s >> 1] : p.blank;
      if constexpr (GAPS) {
        // the DP's own operands and fp32 operations, so the mark agrees with the score
        const int t = c0 + i;
        if (!(s & 1) && p.gap[(int64_t)b * (p.Lmax + 1) + (s >> 1)] &&
            p.filler[(int64_t)b * p.T + t] + p.gap_penalty > to_f(X[(int64_t)t * p.ldx + p.blank]) - LSE[t])
          tok = AVSR_CTC_ALIGN_GAP;
      }
      ALI[c0 + i] = tok;
    }
  }
}

template <typename T, int P, int D, bool GAPS>
void launch(const params_t<GAPS>* p, void* stream) {
  hipLaunchKernelGGL((ctc_align_long_kernel<T, P, D, GAPS>), dim3(p->B), dim3(NT), 0, (hipStream_t)stream, *p);
}

// the argument checks and the choice of P that both entry points share
template <bool GAPS>
int run(const params_t<GAPS>* p, void* stream) {
  if (!p || p->B < 0 || p->T < 0 || p->Lmax < 0 || p->V <= 0 || p->ldx < p->V || p->blank < 0 || p->blank >= p->V)
    return AVSR_E_ARG;
  if constexpr (GAPS)
    if (!(p->gap_penalty <= 0.f)) return AVSR_E_ARG;            // NaN or > 0
  return avsr_by_dtype(p->dtype, [&](auto t) -> int {
    using T = decltype(t);
    if (p->Lmax > AVSR_CTC_ALIGN_LONG_LMAX) return AVSR_E_SHAPE;
    if (p->B == 0) return 0;
    if (!p->label_len || !p->in_len || !p->ali || !p->score || !p->feasible || (p->Lmax > 0 && !p->labels))
      return AVSR_E_ARG;
    if (p->T > 0 && (!p->x || !p->lse || !p->ws)) return AVSR_E_ARG;
    if constexpr (GAPS)
      if (p->T > 0 && (!p->gap || !p->filler)) return AVSR_E_ARG;
    if (!avsr_aligned16(p->ws)) return AVSR_E_ALIGN;
    static_assert(AVSR_CTC_ALIGN_LONG_WS(1, 1, 100) == 64, "header macro and row_bytes agree");
    const int SS = 2 * p->Lmax + 1;
    if (SS <= 4 * NT) launch<T, 4, 4, GAPS>(p, stream);
    else if (SS <= 8 * NT) launch<T, 8, 4, GAPS>(p, stream);
    else if (SS <= 16 * NT) launch<T, 16, 4, GAPS>(p, stream);
    else launch<T, 32, GAPS ? 1 : 2, GAPS>(p, stream);      // GAPS at D = 2 spills more
    AVSR_CHECK_LAUNCH();
    return 0;
  });
}

}  // namespace

extern "C" int avsr_ctc_align_long(const avsr_ctc_align_params* p, void* stream) { return run<false>(p, stream); }

extern "C" int avsr_ctc_align_gaps(const avsr_ctc_align_gaps_params* p, void* stream) { return run<true>(p, stream); }
