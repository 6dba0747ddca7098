// Fused multi-head attention (head dim 64) forward / backward on bf16 MFMA 32x32x16 tiles: the
// C ABI avsr_attn_fwd / avsr_attn_bwd_prep / avsr_attn_bwd / avsr_attn_dropmask / avsr_attn_path
// (include/avsr_hip.h), the choice of kernel family (attn_path) and the two element-wise passes
// (delta, bias gradients). The kernels, by AVSR_ATTN_PATH_* (shared pieces: attention.h):
//   SQ        attention_enc.hip       sq::  forward of the encoder's self-attention: bf16, non-causal,
//                                           Lq >= 128, query-tiled, K / V through an LDS-DMA ring
//   ENC       attention_enc.hip       rb::  its backward: bf16, non-causal, 128 <= Lq, Lk <= 384
//   RESIDENT  attention_resident.hip  res:: bf16 with the streamed operands of a head resident in
//                                           LDS (<= 384 rows): the decoder's self / source attention
//   TILED     attention_tiled.hip     v2::  every other bf16 shape (longer clips, causal or short Lq)
//   F32       attention_f32.hip       f32:: fp32 storage (parity mode), any shape
#include "attention.h"

namespace attn {
namespace {
// delta[b][h][i] = sum_d dO * O (avsr_attn_bwd_prep: the F32 and TILED backward read it)
template <typename T>
__global__ __launch_bounds__(256) void attn_prep_kernel(AttnArgs a) {
  constexpr int VE = 16 / (int)sizeof(T);
  const int64_t n = (int64_t)a.B * a.Lq * a.H;
  for (int64_t t = blockIdx.x * 256 + threadIdx.x; t < n; t += (int64_t)gridDim.x * 256) {
    const int h = (int)(t % a.H);
    const int64_t row = t / a.H;                 // b*Lq + i
    const T* o = (const T*)a.o + row * a.ldo + h * DH;
    const T* d = (const T*)a.dout + row * a.lddo + h * DH;
    float s = 0.f;
#pragma unroll
    for (int e = 0; e < DH; e += VE) {
      float x[VE], y[VE];
      ldv(o + e, x); ldv(d + e, y);
#pragma unroll
      for (int j = 0; j < VE; ++j) s += x[j] * y[j];
    }
    const int64_t b = row / a.Lq, i = row % a.Lq;
    a.delta[(b * a.H + h) * a.Lq + i] = s;
  }
}

// column sums per utterance of the stored dQ / dK / dV (avsr_attn_params.db, every path):
// ws[b][s][c], thread = one of the 3 * HD columns, rows in order
template <typename TQ, typename T>
__global__ __launch_bounds__(256) void attn_db_kernel(const TQ* dq, int64_t lddq, const T* dk, int64_t lddk, const T* dv,
                                                      int64_t lddv, int Lq, int Lk, int HD, float* ws) {
  const int b = blockIdx.y, col = blockIdx.x * 256 + threadIdx.x;
  if (col >= 3 * HD) return;
  const int s = col / HD, c = col % HD;
  float acc = 0.f;
  if (s == 0) {
    for (int i = 0; i < Lq; ++i) acc += (float)dq[((int64_t)b * Lq + i) * lddq + c];
  } else {
    const T* x = s == 1 ? dk : dv;
    const int64_t ld = s == 1 ? lddk : lddv;
    for (int i = 0; i < Lk; ++i) acc += (float)x[((int64_t)b * Lk + i) * ld + c];
  }
  ws[(int64_t)b * 3 * HD + col] = acc;
}

AttnArgs args(const avsr_attn_params* p) {
  AttnArgs a;
  a.B = p->B; a.H = p->H; a.Lq = p->Lq; a.Lk = p->Lk; a.scale = p->scale;
  a.q = p->q; a.ldq = p->ldq; a.k = p->k; a.ldk = p->ldk; a.v = p->v; a.ldv = p->ldv;
  a.o = p->o; a.ldo = p->ldo; a.lse = p->lse; a.klen = p->klen; a.causal = p->causal;
  a.drop_p = p->drop_p; a.seed = p->seed; a.dout = p->dout; a.lddo = p->lddo; a.delta = p->delta;
  a.dq = p->dq; a.lddq = p->lddq; a.dk = p->dk; a.lddk = p->lddk; a.dv = p->dv; a.lddv = p->lddv;
  a.mnqb = (p->Lq + 31) / 32;
  a.mnkb = 2 * ((p->Lk + 63) / 64);
  const bool m = p->drop_mask != nullptr && p->drop_p > 0.f && !p->causal && p->dtype == AVSR_BF16;
  a.mq = m ? p->drop_mask : nullptr;
  return a;
}

int check(const avsr_attn_params* p) {
  if (!p) return AVSR_E_ARG;
  const int ve = p->dtype == AVSR_BF16 ? 8 : 4;
  if (p->ldq % ve || p->ldk % ve || p->ldv % ve || p->ldo % ve) return AVSR_E_ALIGN;
  if (p->dtype != AVSR_BF16 && p->dtype != AVSR_F32) return AVSR_E_DTYPE;
  return 0;
}
// the dropout pair index fits 32 bits (AttnDrop::small): what hashG's callers (res, sq, rb) assume
bool small_index(const avsr_attn_params* p) {
  return (uint64_t)p->B * p->H * p->Lq * (uint64_t)((p->Lk + 1) / 2) <= 0xFFFFFFFFull;
}

// The kernel family of a checked call: the one place that decides it. AVSR_OPT_ATTN_SQ_FWD = 0
// sends the encoder's forward to the resident kernels (A/B runs).
int attn_path(const avsr_attn_params* p, int pass) {
  if (p->dtype != AVSR_BF16) return AVSR_ATTN_PATH_F32;
  const bool small = small_index(p);
  if (pass == AVSR_ATTN_FWD) {
    if (!p->causal && p->Lq >= 128 && small && avsr_opt(AVSR_OPT_ATTN_SQ_FWD) != 0) return AVSR_ATTN_PATH_SQ;
    return p->Lk <= MAXR && small ? AVSR_ATTN_PATH_RESIDENT : AVSR_ATTN_PATH_TILED;
  }
  const bool fits = p->Lq <= MAXR && p->Lk <= MAXR && small;
  if (fits && !p->causal && p->Lq >= 128 && p->Lk >= 128 && (p->lddo % 8) == 0) return AVSR_ATTN_PATH_ENC;
  return fits ? AVSR_ATTN_PATH_RESIDENT : AVSR_ATTN_PATH_TILED;
}

}  // namespace
}  // namespace attn
using namespace attn;

extern "C" int avsr_attn_path(const avsr_attn_params* p, int pass) {
  const int rc = check(p);
  if (rc) return rc;
  return pass == AVSR_ATTN_FWD || pass == AVSR_ATTN_BWD ? attn_path(p, pass) : AVSR_E_ARG;
}

// diagnostic: device buffer of 6 x uint64 per workgroup for the resident forward kernel and the
// encoder backward (nullptr: off), set in both files that stamp. Not part of the product path.
extern "C" int avsr_debug_attn_stamps(unsigned long long* buf) {
  const int rc = resident_stamps(buf);
  return rc ? rc : enc_stamps(buf);
}

extern "C" int avsr_attn_fwd(const avsr_attn_params* p, void* stream) {
  int rc = check(p);
  if (rc) return rc;
  if (p->B * p->H == 0 || p->Lq == 0) return 0;
  const AttnArgs a = args(p);
  switch (attn_path(p, AVSR_ATTN_FWD)) {
    case AVSR_ATTN_PATH_SQ: return sq_fwd(p, a, (hipStream_t)stream);
    case AVSR_ATTN_PATH_RESIDENT: return resident_fwd(p, a, (hipStream_t)stream);
    case AVSR_ATTN_PATH_TILED: return tiled_fwd(p, a, (hipStream_t)stream);
    default: return f32_fwd(p, a, (hipStream_t)stream);
  }
}

extern "C" int avsr_attn_dropmask(const avsr_attn_params* p, void* stream) {
  if (!p || !p->drop_mask) return AVSR_E_ARG;
  if (!(p->drop_p > 0.f) || !small_index(p)) return AVSR_E_ARG;
  if (p->B * p->H == 0 || p->Lq == 0 || p->Lk == 0) return 0;
  avsr_attn_params q = *p;
  q.dtype = AVSR_BF16; q.causal = 0;                    // the layout args() fills for the mask readers
  if ((int64_t)p->B * p->H > 65535) return AVSR_E_SHAPE;
  return resident_mask(p, args(&q), (hipStream_t)stream);
}

// only the F32 and TILED backward read a precomputed delta: the encoder backward computes it in
// its prologue (fused kernel) or its dQ kernel, the resident backward inside its dK/dV kernel
extern "C" int avsr_attn_bwd_prep(const avsr_attn_params* p, void* stream) {
  int rc = check(p);
  if (rc) return rc;
  const int path = attn_path(p, AVSR_ATTN_BWD);
  if (path != AVSR_ATTN_PATH_F32 && path != AVSR_ATTN_PATH_TILED) return 0;
  AttnArgs a = args(p);
  const int g = avsr_grid((int64_t)p->B * p->Lq * p->H);
  if (p->dtype == AVSR_BF16) hipLaunchKernelGGL(attn_prep_kernel<bf16>, dim3(g), dim3(256), 0, (hipStream_t)stream, a);
  else hipLaunchKernelGGL(attn_prep_kernel<float>, dim3(g), dim3(256), 0, (hipStream_t)stream, a);
  AVSR_CHECK_LAUNCH();
  return 0;
}

extern "C" int avsr_attn_bwd(const avsr_attn_params* p, void* stream) {
  int rc = check(p);
  if (rc) return rc;
  if (p->db && !p->db_ws) return AVSR_E_ARG;
  if (p->B * p->H == 0 || p->Lk == 0) return 0;
  hipStream_t st = (hipStream_t)stream;
  const AttnArgs a = args(p);
  if (p->dtype == AVSR_BF16) {
    if (p->dq_out && (p->lddq_out % 8 || !avsr_aligned16(p->dq_out))) return AVSR_E_ALIGN;
    if (!p->dq_out && (p->lddq % 4 || !avsr_aligned16(p->dq))) return AVSR_E_ALIGN;
  }
  switch (attn_path(p, AVSR_ATTN_BWD)) {
    case AVSR_ATTN_PATH_ENC: rc = enc_bwd(p, a, st); break;
    case AVSR_ATTN_PATH_RESIDENT: rc = resident_bwd(p, a, st); break;
    case AVSR_ATTN_PATH_TILED: rc = tiled_bwd(p, a, st); break;
    default: rc = f32_bwd(p, a, st);
  }
  if (rc || !p->db) return rc;
  const int HD = p->H * DH;
  const dim3 g((3 * HD + 255) / 256, p->B);
  if (p->dtype == AVSR_BF16 && p->dq_out)
    hipLaunchKernelGGL((attn_db_kernel<bf16, bf16>), g, dim3(256), 0, st, (const bf16*)p->dq_out, p->lddq_out,
                       (const bf16*)p->dk, p->lddk, (const bf16*)p->dv, p->lddv, p->Lq, p->Lk, HD, p->db_ws);
  else if (p->dtype == AVSR_BF16)
    hipLaunchKernelGGL((attn_db_kernel<float, bf16>), g, dim3(256), 0, st, (const float*)p->dq, p->lddq,
                       (const bf16*)p->dk, p->lddk, (const bf16*)p->dv, p->lddv, p->Lq, p->Lk, HD, p->db_ws);
  else
    hipLaunchKernelGGL((attn_db_kernel<float, float>), g, dim3(256), 0, st, (const float*)p->dq, p->lddq,
                       (const float*)p->dk, p->lddk, (const float*)p->dv, p->lddv, p->Lq, p->Lk, HD, p->db_ws);
  AVSR_CHECK_LAUNCH();
  return colsum_launch(p->db_ws, p->B, (int64_t)3 * HD, 3 * HD, p->db, 0, nullptr, st);
}
