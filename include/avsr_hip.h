/*
 * avsr_hip.h — C-ABI of libavsr_hip.so, the MI355X (gfx950) kernel library behind the
 * AV-HuBERT AVSR forward/backward hot path.
 *
 * Boundary contract:
 *   - every entry point is `extern "C"`, takes plain device pointers + sizes (in a POD
 *     params struct) and a hipStream_t passed as `void*`; returns 0 on success or a
 *     hipError_t / AVSR_E_* code.
 *   - the caller owns every buffer (the PyTorch caching allocator in the Python host);
 *     kernels never allocate, free or synchronise the host, so every launch is
 *     graph-capturable.
 *   - dtype tag: AVSR_F32 = fp32 storage ("parity mode": operands are split into
 *     bf16 hi+lo and fed to the same bf16 MFMA tiles, 3 products per step),
 *     AVSR_BF16 = bf16 storage (throughput mode). Accumulation is always fp32.
 *
 * Each entry point names the reference operation it replaces (file:line in
 * quanpn90/avsr @ 2025-08-29 unless prefixed HF: = transformers 4.52.4
 * models/wav2vec2/modeling_wav2vec2.py, or ATen: = torch 2.7.1 operator).
 */
#ifndef AVSR_HIP_H
#define AVSR_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum { AVSR_F32 = 0, AVSR_BF16 = 1 };
enum { AVSR_ACT_NONE = 0, AVSR_ACT_GELU = 1, AVSR_ACT_RELU = 2 };
enum { AVSR_E_SHAPE = 1001, AVSR_E_ALIGN = 1002, AVSR_E_DTYPE = 1003, AVSR_E_ARG = 1004 };

/* library identity: returns a static string ("avsr_hip <version> gfx950") */
const char* avsr_version(void);

/* ------------------------------------------------------------------------------------
 * Process-wide kernel-selection options. These are the only switches that change which
 * kernel an entry point launches; the library reads no environment variables. Every option
 * defaults to the measured production choice (value in brackets); the others exist for A/B
 * measurements (tools/) and the tests that pin each variant. Set them between launches, not
 * while another host thread is enqueueing work. Results of the variants are identical
 * unless an option says otherwise.
 *   AVSR_OPT_GEMM_TILE      [0]  0: automatic tile choice (gemm.hip tile_cfg); k + 1 forces
 *                                 tile configuration k (AVSR_TILE_* below) on the bf16 core
 *   AVSR_OPT_ATTN_SQ_FWD    [1]  1: query-tiled streamed self-attention forward for bf16,
 *                                 L >= 128; 0: the resident-K/V kernel (same rows to 1e-2)
 *   AVSR_OPT_ATTN_SQ_BWD    [0]  retired: accepts 0 only (the small-footprint dQ kernel it
 *                                 selected measured 0.4 % slower in the step and was removed)
 *   AVSR_OPT_WGRAD_DUAL     [1]  1: two-wave-group weight-gradient kernel (fp32 C, both
 *                                 operands r-contiguous); 0: the 4-wave core
 *   AVSR_OPT_CONV_192       [1]  1: 192x128 tiles for conv fwd / data-grad where they still
 *                                 run >= 2 blocks per CU; 0: 128x128 (bit-identical)
 *   AVSR_OPT_CONV_S2PHASE   [1]  1: stride-2 data-grads as four parity-class GEMMs; 0: one
 *                                 col2im GEMM over all taps (bit-identical)
 *   AVSR_OPT_CONV_PATCH     [1]  1: patch-resident 3x3 kernel for 64-channel stride-1 fwd /
 *                                 data-grad; 0: the general implicit GEMM (bit-identical)
 *   AVSR_OPT_CONV_WPATCH    [1]  1: patch-resident weight-grad (ResNet stage 1-4 geometries);
 *                                 0: the general split-K weight-grad (fp32 re-association)
 *   AVSR_OPT_STEM_POOL_2X2  [1]  1: stem max-pool forward / backward apply over 2x2 output
 *                                 blocks; 0: one output pixel per thread (bit-identical)
 *   AVSR_OPT_STEM_WPATCH    [1]  1: patch-resident stem weight-grad (packed 8-channel input,
 *                                 7x7 / stride 2); 0: the general split-K weight-grad (fp32
 *                                 re-association)
 *   AVSR_OPT_ATTN_ENC_FUSED [1]  1: encoder attention backward in one kernel (dQ from the
 *                                 dK / dV pass); 0: the dQ kernel, then the dK / dV kernel
 *                                 (dK, dV, delta bit-identical; dQ within one rounding of dS)
 * avsr_set_option returns 0, or AVSR_E_ARG for an unknown option or a value out of range;
 * avsr_get_option returns the value, or -1 for an unknown option.
 * ------------------------------------------------------------------------------------ */
enum {
  AVSR_OPT_GEMM_TILE = 0,
  AVSR_OPT_ATTN_SQ_FWD = 1,
  AVSR_OPT_ATTN_SQ_BWD = 2,
  AVSR_OPT_WGRAD_DUAL = 3,
  AVSR_OPT_CONV_192 = 4,
  AVSR_OPT_CONV_S2PHASE = 5,
  AVSR_OPT_CONV_PATCH = 6,
  AVSR_OPT_CONV_WPATCH = 7,
  AVSR_OPT_STEM_POOL_2X2 = 8,
  AVSR_OPT_STEM_WPATCH = 9,
  AVSR_OPT_ATTN_ENC_FUSED = 10,
  AVSR_OPT_COUNT = 11
};
/* tile configurations of the bf16 GEMM core (AVSR_OPT_GEMM_TILE = k + 1): rows x columns, wN =
 * N waves, sN = N LDS stages, PP = the 256x256 ping-pong core. One row each in gemm.hip's tile
 * table, one name each in avsr_amd/_lib.py TILES (tests/test_lib_abi.py compares them). The ids
 * are not persistent (tools, tests and profiles use the names): measured-and-dropped
 * configurations leave and the rest are renumbered. */
enum {
  AVSR_TILE_128 = 0, AVSR_TILE_256 = 1, AVSR_TILE_256x128 = 2, AVSR_TILE_128x256 = 3, AVSR_TILE_128s3 = 4,
  AVSR_TILE_128w8s3 = 5, AVSR_TILE_PP = 6, AVSR_TILE_192 = 7, AVSR_TILE_192x256 = 8, AVSR_TILE_192w8s3 = 9,
  AVSR_TILE_64 = 10, AVSR_TILE_64s4 = 11, AVSR_TILE_COUNT = 12
};
int avsr_set_option(int option, int64_t value);
int64_t avsr_get_option(int option);

/* ------------------------------------------------------------------------------------
 * GEMM with fused epilogue, fp32 accumulate: v_mfma_f32_16x16x32_bf16 on the LDS-DMA core
 * (128x128 / 192x128 tiles, bf16), v_mfma_f32_32x32x16_bf16 on the register-staged core
 * (fp32 parity mode: bf16 hi/lo split; shapes under 128 rows / columns).
 *   C[b][m][n] = epi( alpha * sum_k A(b,m,k) * B(b,n,k) )
 *   A(m,k) = A[m*lda + k] if a_kmajor else A[k*lda + m]
 *   B(n,k) = B[n*ldb + k] if b_kmajor else B[k*ldb + n]
 * Forward epilogue (epi_bwd = 0):  h = alpha*acc + bias[n];  if (preact) preact[m][n] = h;
 *   y = act(h); y = dropout(y; drop_p, seed); y += res[m][n]; C = y (+ beta*C_old)
 * Backward epilogue (epi_bwd = 1): g = alpha*acc; g = dropout_mask(g; drop_p, seed);
 *   g *= act'(gate[m][n]); C = g (+ beta*C_old)
 * Replaces: torch.nn.Linear (ATen addmm) everywhere on the path — encoder q/k/v/out
 *   (HF:Wav2Vec2Attention), FFN (HF:Wav2Vec2FeedForward :551-572), post_extract_proj
 *   (src/nets/backend/backbones/avhubert.py:259-263), SubModel.proj (:187-198),
 *   ctc_lo (src/nets/backend/ctc.py:25), decoder linears
 *   (src/nets/backend/transformer/attention.py:31-34, positionwise_feed_forward.py:25-30,
 *   decoder.py:117) — forward, input-grad and weight-grad.
 * Requirements: lda/ldb/ldc and the contiguous extent multiples of 8 elements, pointers
 *   16-byte aligned (AVSR_E_ALIGN otherwise).
 * ------------------------------------------------------------------------------------ */
typedef struct {
  int M, N, K, batch;
  int dtype;                 /* AVSR_F32 / AVSR_BF16: storage of A, B, res, preact, gate */
  int a_kmajor, b_kmajor;
  int c_f32;                 /* 1: C is fp32 regardless of dtype (weight grads) */
  const void* A; int64_t lda, strideA;
  const void* B; int64_t ldb, strideB;
  void* C;       int64_t ldc, strideC;
  float alpha, beta;
  const float* bias;         /* [N] fp32 or NULL (forward only) */
  int act;                   /* AVSR_ACT_* */
  int epi_bwd;               /* 0 forward epilogue, 1 backward (gate) epilogue */
  void* preact;              /* forward: store pre-activation h (dtype, ld = ldc) or NULL */
  const void* res;  int64_t ldr, strideR;   /* residual (dtype) or NULL */
  const void* gate;          /* backward: pre-activation h (dtype, ld = ldc) or NULL */
  float drop_p;              /* dropout probability (0 = off) */
  uint64_t seed;             /* counter-based dropout stream id */
  int splitk;                /* >1: K split over blocks (C must be fp32) */
  float* ws;                 /* split-K slab workspace, AVSR_GEMM_SLAB_WS(batch, splitk, M, N) fp32:
                                each split stores its partial tile, a reduce pass writes
                                C = alpha*sum + beta*C (plain epilogue only). NULL: C += alpha*acc
                                by fp32 atomics. Ignored when splitk <= 1. */
  float* db;                 /* optional: db[n] += sum_m C[m][n] of the stored tile values (the
                                bias gradient of the layer whose output gradient C is, e.g.
                                FFN1's bias from the FFN2 data-grad); bf16, N % 8 == 0, no split */
  float* db_ws;              /* its row-tile partials, AVSR_GEMM_COLSUM_WS(M, N) fp32 */
  unsigned long long* stamp; /* optional diagnostic (bench.py roofline probe; bf16 LDS-DMA path):
                                {min start, max end} in s_memrealtime ticks (100 MHz) — every
                                workgroup folds its first / last instant in by vector atomics.
                                Caller initialises {~0ull, 0}. No output depends on it. */
  float* skinny_ws;          /* optional, AVSR_SKINNY_WS_BYTES: with splitk <= 1 and M <= 64 (the
                                vector-ALU path of decoder steps) the launch splits K over
                                avsr_gemm_skinny_splits(N, K) workgroup rows: AVSR_SKINNY_WS fp32
                                partials, then AVSR_SKINNY_CNT uint32 arrival counters that the
                                caller zeroes once (every launch leaves them zero); the last
                                workgroup of a column block adds the partials in a fixed order
                                and runs the epilogue. NULL: one workgroup row. */
  const float* ln_c1;        /* optional LayerNorm prologue (fp32, M <= 64, K <= 1024, K % 16 == 0,
                                unsplit): A holds the LayerNorm inputs x and B = gamma o W (W's
                                columns scaled by the LayerNorm weight); per row the kernel takes
                                mean and 1/sqrt(var + ln_eps) of x and computes
                                C = epilogue(rstd * (x B^T - mean * ln_c1[n])) with ln_c1[n] =
                                sum_k B[n][k] and bias = W beta + b — LayerNorm followed by the
                                linear (decoder.py:98-134 norm1/2/3 + linear) in one launch */
  float ln_eps;
  void* kv_k;                /* optional KV-cache append (fp32 few-row path, N % 3 == 0, D = N / 3):
                                output columns [D, 2D) of row m go to kv_k row (*kv_pos * kv_rows +
                                m) instead of C, columns [2D, 3D) to kv_v (the self-attention K / V
                                cache of the device-side beam search; avsr_beam_kv_put fused into
                                the QKV projection); columns [0, D) to C as usual */
  void* kv_v;
  const int* kv_pos;
  int kv_rows;
  unsigned* slab_cnt;        /* optional, AVSR_SLAB_CNT uint32 arrival counters for the slab split-K
                                weight-gradient path (splitk > 1 with ws, both operands r-contiguous,
                                fp32 C, plain epilogue): the last-arriving split of each output
                                tile reduces the slabs inside the GEMM (no separate reduction pass).
                                The caller zeroes them once; every launch leaves them zero. Launches
                                that share a counter buffer must be ordered (one stream). NULL: a
                                separate reduction pass. */
  int kv_pos_stride;         /* KV-cache append: 0 = one shared position *kv_pos (above); 1 = one
                                position per row, row m appends at cache row kv_pos[m] * kv_rows + m
                                (the rows of a decode session stand at different steps) */
} avsr_gemm_params;
#define AVSR_GEMM_COLSUM_WS(M, N) ((int64_t)(((M) + 63) / 64) * (N))
/* slabs are AVSR_GEMM_SLAB_PAD floats apart beyond M*N: power-of-two slab strides put the
 * reduce pass's split-many reads of one vector on the same HBM channels (measured 0.55 TB/s for
 * 8 slabs of 4 MiB) */
#define AVSR_GEMM_SLAB_PAD 1088
#define AVSR_SKINNY_WS (1 << 19)
#define AVSR_SKINNY_CNT 4096
#define AVSR_SLAB_CNT 4096
#define AVSR_SKINNY_WS_BYTES ((int64_t)AVSR_SKINNY_WS * 4 + AVSR_SKINNY_CNT * 4)
#define AVSR_GEMM_SLAB_WS(batch, splitk, M, N) ((int64_t)(batch) * (splitk) * ((int64_t)(M) * (N) + AVSR_GEMM_SLAB_PAD))

int avsr_gemm(const avsr_gemm_params* p, void* stream);
/* n <= 4 weight-gradient GEMMs (C fp32 += alpha * A^T B with both operands r-contiguous bf16, no
 * epilogue, no split: the avsr_gemm weight-gradient shape) in ONE launch whose grid holds every
 * problem's output tiles — problems that each fill part of the chip fill it together (encoder
 * out-proj 64 + QKV 192 tiles = 256 = one block per CU). Results equal avsr_gemm's per problem
 * bit for bit; problems of another shape run one by one through avsr_gemm. Replaces the
 * nn.Linear weight-gradients of Wav2Vec2Attention (avhubert.py:747-768). */
int avsr_gemm_wgrad_group(const avsr_gemm_params* p, int n, void* stream);
/* K-split count the few-row path uses for an N x K weight of this dtype when skinny_ws is given
 * (depends on dtype, N and K only, never on M: a row's result does not depend on how many rows
 * share the launch; fp32 with K % 16 == 0 and 16-byte aligned rows runs the matrix-core kernel) */
int avsr_gemm_skinny_splits(int dtype, int N, int K);

/* ------------------------------------------------------------------------------------
 * Implicit-GEMM convolution over NHWC activations (no im2col buffer), grouped.
 *   x [nimg][hin][win][ldx] (group g uses channels g*cin .. g*cin+cin-1)
 *   y [nimg][hout][wout][ldy] (group g: channels g*cout ..)
 *   w [groups*cout][kh][kw][cin]  (= torch channels_last physical order)
 * fwd:         y  = conv(x, w)                          (+ BN partial statistics if stats)
 * bwd_data:    dx = alpha * conv_transpose(dy, w) (+ beta * dx)
 * bwd_weight:  dw (fp32) += conv_wgrad(x, dy)   (split-K over pixels: fp32 slabs in ws, reduced
 *              by a second kernel; without ws, fp32 atomics)
 * Replaces: nn.Conv2d in src/nets/backend/backbones/resnet.py:10-22 (3x3 and 1x1
 *   downsample, ResNet-18 trunk), nn.Conv3d stem resnet.py:132 (as a 2-D conv over 5
 *   time-stacked channels, see avsr_stem_pack), and the grouped pos-conv Conv1d
 *   (k=128, groups 16) of HF:Wav2Vec2PositionalConvEmbedding (:326-369) as a 1-D conv
 *   (win = wout = kw = 1).
 * Requirements: cin, cout powers of two >= 8; ldx, ldy multiples of 8; 16-B aligned.
 * ------------------------------------------------------------------------------------ */
typedef struct {
  int dtype;
  int nimg, hin, win, cin;
  int hout, wout, cout;
  int kh, kw, sh, sw, ph, pw;
  int groups;
  int64_t ldx, ldy;
  const void* x; const void* w; void* y;   /* forward operands / output */
  void* dx; const void* dy; float* dw;     /* backward */
  float* stats;   /* fwd only: [cout][avsr_conv_stat_tiles()][3] (count, mean, M2) or NULL */
  float alpha, beta;                       /* bwd_data scaling */
  int splitk;     /* bwd_weight: 0 = auto */
  /* fwd epilogue (optional): h = conv + bias[c]; preact = h; y = act(h) + res  (res/preact
   * laid out like y; used by the pos-conv: x + GELU(conv(x) + b)) */
  const float* bias; int act; void* preact; const void* res;
  float* ws;      /* bwd_weight split-K workspace of avsr_conv_wgrad_ws() floats, or NULL */
  /* bwd_data, optional (bf16, groups 1): BatchNorm+PReLU backward reduction in the epilogue.
   * The value v = alpha*conv_transpose(dy, w) + beta*dx is the gradient of prelu(z),
   * z = h*scale + shift (+ res | + res*scale2 + shift2); dx receives dz = prelu'(z)*v and
   * bnr_ws[avsr_conv_bnr_tiles()][4][cin] the per-tile column sums (sum dz, sum dz*xhat,
   * sum dz*xhat2, sum v*z*[z<=0]) that avsr_bn_bwd_finalize folds. h / res laid out like dx.
   * Replaces the separate avsr_bn_act_bwd_reduce pass over dx (resnet.py:45-62 backward). */
  const void* bnr_h; const void* bnr_res;
  const float* bnr_scale; const float* bnr_shift; const float* bnr_prelu;
  const float* bnr_mean; const float* bnr_invstd;
  const float* bnr_scale2; const float* bnr_shift2; const float* bnr_mean2; const float* bnr_invstd2;
  float* bnr_ws;
} avsr_conv_params;

int avsr_conv_fwd(const avsr_conv_params* p, void* stream);
int avsr_conv_bwd_data(const avsr_conv_params* p, void* stream);
int avsr_conv_bwd_weight(const avsr_conv_params* p, void* stream);
/* number of row tiles the forward partial statistics are split into */
int avsr_conv_stat_tiles(const avsr_conv_params* p);
/* number of row tiles of a bwd_data with the BN-backward epilogue (rows of bnr_ws) */
int avsr_conv_bnr_tiles(const avsr_conv_params* p);
/* fp32 workspace (floats) bwd_weight uses when p->ws is given (0: it needs none) */
int64_t avsr_conv_wgrad_ws(const avsr_conv_params* p);
/* the kernel family avsr_conv_fwd (pass = AVSR_CONV_FWD), avsr_conv_bwd_data (AVSR_CONV_DGRAD) or
 * avsr_conv_bwd_weight (AVSR_CONV_WGRAD) runs for this call under the current options: an
 * AVSR_CONV_PATH_* id, or the AVSR_E_* code the call returns for its geometry or dtype
 * (AVSR_E_ARG: p NULL or no such pass). It reads what the call reads, so whether bias / act / res /
 * preact (forward) and ws (weight-grad) are set, and splitk, count. The three size queries above
 * follow the same choice. Host-only: dereferences no pointer of the struct and touches no device.
 *   REG          fp32 storage: register-staged implicit GEMM
 *   GLDS         bf16: LDS-DMA implicit GEMM
 *   PATCH        bf16 3x3 / stride 1 / pad 1 with 64 channels on both sides, forward without an
 *                epilogue beyond the BN statistics, or data-grad: the input patch resident in LDS
 *   S2           bf16 stride-2 data-grad as four parity-class GLDS GEMMs (data-grad only)
 *   WPATCH       bf16 weight-grad of the ResNet stage 1-4 geometries with a workspace
 *   STEM_WPATCH  bf16 weight-grad of the stem geometry on the packed input with a workspace */
enum { AVSR_CONV_FWD = 0, AVSR_CONV_DGRAD = 1, AVSR_CONV_WGRAD = 2 };
enum {
  AVSR_CONV_PATH_REG = 0, AVSR_CONV_PATH_GLDS = 1, AVSR_CONV_PATH_PATCH = 2, AVSR_CONV_PATH_S2 = 3,
  AVSR_CONV_PATH_WPATCH = 4, AVSR_CONV_PATH_STEM_WPATCH = 5
};
int avsr_conv_path(const avsr_conv_params* p, int pass);

/* ------------------------------------------------------------------------------------
 * LayerNorm over the last dim (rows of N), fp32 statistics.
 * fwd: y = (x - mean) * rstd * gamma + beta; stores mean/rstd per row (fp32).
 * bwd: dx = (dres ? dres : 0) + rstd * (g - mean(g) - xhat * mean(g * xhat)), g = dy * gamma;
 *      dgamma += sum dy * xhat, dbeta += sum dy   (fp32, atomics)
 * Replaces: torch.nn.LayerNorm at avhubert.py:184-185/:484 (2048, eps 1e-5),
 *   HF:Wav2Vec2EncoderLayer layer_norm / final_layer_norm and encoder layer_norm (1e-5),
 *   src/nets/backend/transformer/layer_norm.py:12-33 (decoder, eps 1e-12).
 * ------------------------------------------------------------------------------------ */
typedef struct {
  int dtype, rows, N;
  float eps;
  const void* x; int64_t ldx;
  void* y; int64_t ldy;
  const float* gamma; const float* beta;
  float* mean; float* rstd;                 /* [rows] */
  const void* dy; int64_t lddy;             /* bwd */
  void* dx; int64_t lddx;                   /* bwd output */
  const void* dres; int64_t lddres;         /* bwd: residual gradient added to dx (may alias dx) */
  float* dgamma; float* dbeta;              /* bwd: fp32 accumulators [N] or NULL */
  float* ws;                                /* bwd with dgamma: workspace >= AVSR_LN_WS(N) floats */
  /* bwd, optional: the next elementwise backward of the chain fused in (avsr_ew_bwd with out,
   * drop_p, seed, db): g = dropout-backward(dx as stored) and db += column sums of g. The
   * reference applies dropout to the sublayer output that is added to this LayerNorm's input
   * (HF Wav2Vec2EncoderLayer), so its gradient is the residual gradient dx masked. With db the
   * workspace needs AVSR_LN_WS3(N) floats. */
  void* g; int64_t ldg; float drop_p; uint64_t seed; float* db;
} avsr_layernorm_params;
#define AVSR_LN_BLOCKS 256
#define AVSR_LN_WS(N) (AVSR_LN_BLOCKS * 2 * (N))
#define AVSR_LN_WS3(N) (AVSR_LN_BLOCKS * 3 * (N))
int avsr_layernorm_fwd(const avsr_layernorm_params* p, void* stream);
int avsr_layernorm_bwd(const avsr_layernorm_params* p, void* stream);

/* ------------------------------------------------------------------------------------
 * BatchNorm (NHWC, per-channel) for the ResNet-18 lip frontend, resnet.py:30-164.
 * finalize: combine conv-epilogue partials (count, mean, M2) -> mean / invstd; scale =
 *   gamma*invstd, shift = beta - mean*scale; training also updates running stats
 *   (momentum 0.1, unbiased running_var, as torch.nn.BatchNorm2d/3d). Eval mode builds
 *   scale/shift from the running statistics.
 * act_fwd: y = prelu(h*scale + shift + r), r = res (identity) or res*scale2 + shift2
 *   (downsample BN) or 0;  prelu weight per channel (nn.PReLU(num_parameters=C)).
 * act_bwd_reduce: z recomputed; dz = dy * prelu'(z) (stored); accumulates per channel
 *   sum dz, sum dz*xhat (and for the downsample BN), prelu-weight grad sum dy*z*[z<=0];
 *   also dgamma/dbeta of both BNs.
 * bwd_apply: dh = scale*(dz - sum dz/M - xhat*sum(dz xhat)/M) (+beta*dh), same for the
 *   downsample BN into dhd.
 * ------------------------------------------------------------------------------------ */
typedef struct {
  int tiles, C;               /* partial tiles, channels */
  const float* partials;      /* [C][tiles][3] or NULL (eval) */
  const float* gamma; const float* beta;
  float* running_mean; float* running_var;
  float momentum, eps;
  int training;
  float* mean; float* invstd; float* scale; float* shift;   /* [C] outputs */
} avsr_bn_finalize_params;
int avsr_bn_finalize(const avsr_bn_finalize_params* p, void* stream);

typedef struct {
  int dtype, M, C;
  const void* h;                                   /* conv output (pre-BN) [M][C] */
  const float* scale; const float* shift;          /* BN of h */
  const void* res;                                 /* residual [M][C] or NULL */
  const float* scale2; const float* shift2;        /* BN of res (downsample) or NULL (identity) */
  const float* prelu;                              /* [C] */
  void* y;                                         /* fwd output */
  /* backward */
  const void* dy; void* dz;
  const float* mean; const float* invstd;          /* BN of h (for xhat) */
  const float* mean2; const float* invstd2;        /* BN of res when scale2 */
  float* sums;    /* [C][3] out: sum dz, sum dz*xhat, sum dz*xhat2 (fp32; written, not accumulated) */
  float* dprelu;  /* [C] fp32 grad accumulator */
  float* dgamma; float* dbeta; float* dgamma2; float* dbeta2;   /* fp32 grad accumulators or NULL */
  void* dh; void* dh2; float beta_acc;             /* bwd_apply outputs (dh2 for the downsample BN) */
  float* ws;                                       /* bwd_reduce workspace >= AVSR_BN_WS(C) floats */
} avsr_bn_act_params;
/* partial sums of `tiles` row blocks [tiles][4][C] plus the fold area finalize uses */
#define AVSR_BN_FIN_WS(tiles, C) (((int64_t)(tiles) + ((tiles) > 256 ? ((tiles) + 15) / 16 : 0)) * 4 * (C))
#define AVSR_BN_WS(C) AVSR_BN_FIN_WS(2048, C)
int avsr_bn_act_fwd(const avsr_bn_act_params* p, void* stream);
/* reduce + finalize (sums, dgamma/dbeta, dprelu) */
int avsr_bn_act_bwd_reduce(const avsr_bn_act_params* p, void* stream);
/* finalize only, from partials ws[tiles][4][C] written by a data-grad BN epilogue
 * (avsr_conv_params.bnr_ws, tiles = avsr_conv_bnr_tiles) */
int avsr_bn_bwd_finalize(const avsr_bn_act_params* p, int tiles, void* stream);
int avsr_bn_bwd_apply(const avsr_bn_act_params* p, void* stream);

/* stem: y[n][oh][ow][c] = max_{3x3, s2, p1} prelu(bn(h)) (+argmax index, + hmax = h at the
 * argmax), resnet.py:132-136 (BatchNorm3d + PReLU + MaxPool3d((1,3,3),(1,2,2),(0,1,1))).
 * Backward in the pooled domain: the BN/PReLU reduction is avsr_bn_act_bwd_reduce (or a
 * data-grad BN epilogue) over the POOLED grid with h = hmax, dy = pooled gradient, giving the
 * pooled dz and the sums over input pixels (dz vanishes off the argmax positions);
 * bwd_apply: dh[n][h][w][c] = scale*(dz - S0/M - xhat*S1/M), dz routed back through the
 * argmax (M = m_total, or nimg*H*W). */
typedef struct {
  int dtype, nimg, H, W, C, Ho, Wo;
  const void* h; const float* scale; const float* shift; const float* prelu;
  void* y; uint8_t* argmax;
  const void* dy; void* dz;                        /* bwd_apply: dz = pooled dz [n][Ho][Wo][C] */
  const float* mean; const float* invstd;
  float* sums; float* dprelu; float* dgamma; float* dbeta;
  float* ws;
  void* hmax;                                      /* fwd output [n][Ho][Wo][C] (optional) */
  void* dh;                                        /* bwd_apply output [n][H][W][C] */
  int64_t m_total;                                 /* bwd_apply: pixels M the BN statistics
                                                      cover (0: nimg*H*W); a launch over a range
                                                      of images passes the whole batch's M */
} avsr_stem_pool_params;
int avsr_stem_pool_fwd(const avsr_stem_pool_params* p, void* stream);
int avsr_stem_pool_bwd_apply(const avsr_stem_pool_params* p, void* stream);

/* global average pool over P pixels: y[n][c] = mean_p x[n][p][c] (nn.AdaptiveAvgPool2d(1),
 * resnet.py:83,121); bwd: dx[n][p][c] = dy[n][c] / P */
int avsr_avgpool_fwd(int dtype, int nimg, int P, int C, const void* x, void* y, void* stream);
int avsr_avgpool_bwd(int dtype, int nimg, int P, int C, const void* dy, void* dx, void* stream);

/* ------------------------------------------------------------------------------------
 * Fused multi-head attention, head dim 64, fp32 online softmax (flash-style; the Lq x Lk
 * score matrix is never stored).  o = softmax(scale * q k^T + mask) v  per (batch, head).
 *   q row (b, i), head h: q[(b*Lq + i)*ldq + h*64 .. +63]; likewise k, v (Lk rows), o.
 *   mask: key j of batch b valid iff j < klen[b] (klen NULL: all Lk valid) and, if causal,
 *   j <= i.  Optional dropout on the probabilities (counter-based; bwd recomputes it).
 * fwd stores lse[b][h][i] (natural log) for the backward.
 * bwd: dq (fp32 accumulator [B*Lq][ldq_f32], atomics, caller zeroes) or dq_out (dtype),
 *   dk, dv (dtype); call avsr_attn_bwd_prep first (delta[b][h][i] = sum_d dO*O where the
 *   backward kernels do not compute it themselves).
 * Five kernel families (AVSR_ATTN_PATH_*; avsr_attn_path tells which one a call runs):
 *   F32       fp32 storage: one forward kernel, one backward kernel (dQ by atomics)
 *   TILED     bf16, any shape: 64-row tiles streamed through LDS; dK/dV per key block, dQ per
 *             query block, no atomics
 *   RESIDENT  bf16, the streamed operands of a whole head resident in LDS: forward Lk <= 384,
 *             backward Lq and Lk <= 384 (the decoder's self / source attention)
 *   SQ        bf16 forward, non-causal, Lq >= 128: query-tiled, K / V through an LDS-DMA ring
 *             (the encoder's self-attention; with AVSR_OPT_ATTN_SQ_FWD off: RESIDENT / TILED instead)
 *   ENC       bf16 backward, non-causal, 128 <= Lq, Lk <= 384, lddo % 8 == 0 (its backward)
 *   SQ, RESIDENT and ENC also need B*H*Lq*ceil(Lk/2) < 2^32; other bf16 calls run TILED.
 * Replaces: HF:eager_attention_forward + Wav2Vec2Attention core (:438-548; encoder, key
 *   padding mask from avhubert.py:688-696) and MultiHeadedAttention.forward_attention
 *   (src/nets/backend/transformer/attention.py:56-106; decoder causal self-attention and
 *   memory-masked source attention).
 * ------------------------------------------------------------------------------------ */
typedef struct {
  int dtype, B, H, Lq, Lk;
  float scale;
  const void* q; int64_t ldq;
  const void* k; int64_t ldk;
  const void* v; int64_t ldv;
  void* o; int64_t ldo;
  float* lse;                 /* [B][H][Lq] */
  const int* klen;            /* [B] or NULL */
  int causal;
  float drop_p; uint64_t seed;
  /* backward */
  const void* dout; int64_t lddo;
  float* delta;               /* [B][H][Lq] */
  float* dq; int64_t lddq;    /* fp32 */
  void* dk; int64_t lddk;
  void* dv; int64_t lddv;
  /* bf16 only: if non-NULL, dQ is written here in the activation dtype (dq unused);
   * otherwise bf16 writes dq (fp32) with plain stores (= accumulate onto a zeroed buffer) */
  void* dq_out; int64_t lddq_out;
  /* optional (backward): db[s*H*64 + h*64 + d] += column sums over all B*L rows of the dQ
   * (s = 0), dK (s = 1), dV (s = 2) values as stored (bf16-rounded in bf16) — the fused q/k/v
   * projection bias gradients. db_ws: AVSR_ATTN_DB_WS(B, H) floats of per-utterance partials,
   * finalised through the column-sum path (deferred like avsr_gemm db: keep it alive until the
   * flush). Every path computes them in one extra pass over the stored dq/dk/dv after the
   * backward kernels. NULL: off. */
  float* db; float* db_ws;
  /* optional probability-dropout keep mask (bf16, non-causal): written once per (seed, shape)
   * by avsr_attn_dropmask, then read by avsr_attn_fwd / avsr_attn_bwd in place of re-hashing
   * the counter dropout per element (same bits: the mask IS the hash's keep decision). 64-bit
   * lane masks, AVSR_ATTN_MASK_WORDS(B, H, Lq, Lk) words, per (b, h) and 32 x 32 tile (query
   * block qb of 32, key block kb of 32, kb padded to an even count NKB = 2 * ceil(Lk / 64)), 16
   * words per tile, query on the lane: word ((bh * NQB + qb) * NKB + kb) * 16 + r, bit l keeps
   * (q = 32 qb + (l & 31), k = 32 kb + (r & 3) + 8 (r >> 2) + 4 (l >> 5)); 0 past Lq / Lk.
   * NULL: the kernels hash (decoder attention, fp32). */
  uint64_t* drop_mask;
} avsr_attn_params;
#define AVSR_ATTN_DB_WS(B, H) ((int64_t)(B) * 3 * (H) * 64)
#define AVSR_ATTN_MASK_WORDS(B, H, Lq, Lk) \
  ((int64_t)(B) * (H) * (((Lq) + 31) / 32) * (2 * (((Lk) + 63) / 64)) * 16)
/* diagnostic (not product path): per-workgroup s_memrealtime stamps (start, first round
 * landed, compute done, end, HW_ID, XCC_ID) of the resident attention forward into
 * buf[6 * workgroups], and of the encoder backward's dQ / dK-dV kernels into buf[6 * B * H]
 * / buf[6 * B * H ..]; buf = NULL turns them off */
int avsr_debug_attn_stamps(unsigned long long* buf);
int avsr_attn_fwd(const avsr_attn_params* p, void* stream);
int avsr_attn_bwd_prep(const avsr_attn_params* p, void* stream);   /* delta = rowsum(dO * O) */
int avsr_attn_bwd(const avsr_attn_params* p, void* stream);
/* the kernel family avsr_attn_fwd (pass = AVSR_ATTN_FWD) or avsr_attn_bwd_prep / avsr_attn_bwd
 * (AVSR_ATTN_BWD) run for this call under the current options: an AVSR_ATTN_PATH_* id, or the
 * AVSR_E_* code those calls return for it. Host-only: reads the struct's integers, dereferences
 * no pointer and touches no device. */
enum { AVSR_ATTN_FWD = 0, AVSR_ATTN_BWD = 1 };
enum {
  AVSR_ATTN_PATH_F32 = 0, AVSR_ATTN_PATH_TILED = 1, AVSR_ATTN_PATH_RESIDENT = 2, AVSR_ATTN_PATH_SQ = 3,
  AVSR_ATTN_PATH_ENC = 4
};
int avsr_attn_path(const avsr_attn_params* p, int pass);
/* fills p->drop_mask (AVSR_ATTN_MASK_WORDS words) with the keep decisions of drop_p / seed for
 * (B, H, Lq, Lk): the data-independent half of the attention dropout, runnable ahead of the
 * forward on another stream. Same replacement as avsr_attn_fwd (the dropout of
 * Wav2Vec2Attention / eager_attention_forward, avhubert.py:747-768). */
int avsr_attn_dropmask(const avsr_attn_params* p, void* stream);

/* ------------------------------------------------------------------------------------
 * Losses on logits [rows][ldx] (V valid columns; columns V..ldx-1 of every gradient row are
 * written as 0 so padded GEMM operands stay finite).
 * avsr_row_lse:   lse[row] = log sum_k exp(x[row][k])
 * avsr_lsm_fwd:   LabelSmoothingLoss rows (src/nets/backend/transformer/label_smoothing_loss.py
 *   :41-63, KL(q || softmax) with q = smoothing/(V-1) off-target, 1-smoothing on target,
 *   target -1 ignored) -> row_loss, and th_accuracy's argmax match (nets_utils.py:303-323)
 *   At smoothing = 0 the row loss is exactly lse[row] - float(x[row][target[row]]) (e = 0 and
 *   conf = 1: the q*log q terms are skipped or log 1, and 0 * (sum x - xt) is 0), 0 on ignored
 *   rows: the negated log-probability of the target, which the rescoring pass of two-pass
 *   decoding sums per hypothesis (ops.token_logp) — no separate kernel.
 * avsr_lsm_bwd:   dx = (*dloss * coef) * (softmax - q), 0 on ignored rows
 * avsr_ctc_fwd:   torch.nn.CTCLoss(blank=0, reduction none, zero_infinity=True) per utterance
 *   (ctc.py:64-81): log-space alpha and beta over the extended label sequence; nll[b] and the
 *   state occupancies gamma[b][t][s] = P(path at state s at t | x) (0 if infeasible)
 * avsr_ctc_bwd:   dx[b,t,k] = (*dloss * coef) * (softmax_t(k) - sum_{s: ext_s = k} gamma_t(s))
 *   for t < in_len[b] (0 otherwise and for infeasible utterances); softmax_t is exp(x - lse)
 *   divided by its own row sum, so the rounding of the stored fp32 lse does not reach it
 * avsr_loss_finalize: loss_ctc = sum nll / B, loss_att = sum row_loss / B (att_per_token = 0) or
 *   / the number of target tokens, i.e. rows with row_correct >= 0 (att_per_token = 1:
 *   transformer_length_normalized_loss, label_smoothing_loss.py:61; needs row_correct),
 *   loss = mtl*ctc + (1-mtl)*att, acc = correct / valid  (e2e_asr_avhubert.py:150-159)
 *   out[4] = {loss, loss_ctc, loss_att, acc}, all on device (no host sync)
 * ------------------------------------------------------------------------------------ */
typedef struct {
  int dtype, rows, V;
  const void* x; int64_t ldx;
  const int* target;        /* [rows], -1 = ignore */
  float smoothing;
  float* lse; float* row_loss; int* row_correct;   /* [rows]; row_correct: 1/0, -1 ignored */
  const float* dloss; float coef;
  void* dx; int64_t lddx;
} avsr_xent_params;
int avsr_row_lse(const avsr_xent_params* p, void* stream);
int avsr_lsm_fwd(const avsr_xent_params* p, void* stream);
int avsr_lsm_bwd(const avsr_xent_params* p, void* stream);

typedef struct {
  int dtype, B, T, V, Lmax;
  const void* x; int64_t ldx;          /* rows b*T + t */
  const float* lse;                    /* [B*T] */
  const int* labels;                   /* [B][Lmax] */
  const int* label_len; const int* in_len;   /* [B] */
  float* alpha; float* gamma;          /* workspaces [B][T][2*Lmax+1] */
  float* nll;                          /* [B] */
  const float* dloss; float coef;
  void* dx; int64_t lddx;
} avsr_ctc_params;
int avsr_ctc_fwd(const avsr_ctc_params* p, void* stream);
int avsr_ctc_bwd(const avsr_ctc_params* p, void* stream);

int avsr_loss_finalize(int B, const float* nll, int rows, const float* row_loss, const int* row_correct,
                       float mtlalpha, int att_per_token, float* out, void* stream);

/* ------------------------------------------------------------------------------------
 * avsr_ctc_align: CTC forced alignment, the best (Viterbi) path of CTC.forced_align_batch
 *   (ctc.py:246-328) for B utterances in one launch, on raw logits x (rows b*T + t) and their
 *   row log-sum-exp. Over the extended sequence ext = blank, y1, blank, ..., yL, blank
 *   (S = 2L + 1 states), in fp32, with e(t, s) = float(x[t][ext_s]) - lse[t]:
 *     d[0][0] = e(0, 0), d[0][1] = e(0, 1), every other state unreachable (-inf)
 *     d[t][s] = max(c0, c1, c2) + e(t, s),  c0 = d[t-1][s],  c1 = d[t-1][s-1] (s >= 1),
 *               c2 = d[t-1][s-2] (s >= 2, ext_s != blank, ext_s != ext_{s-2})
 *   back-pointer = the FIRST maximum in the order (s, s-1, s-2); the final state is the first
 *   maximum of (S-2, S-1) (state 0 for L = 0) at t = in_len[b] - 1, as in the reference. Every
 *   rounding and tie is fixed, so a float32 host Viterbi reproduces ali and score bit for bit.
 *   ali[b][t] = token of the best path (-1 at t >= in_len[b]); score[b] = its log-probability;
 *   feasible[b] = 0 with ali[b][:] = -1 and score[b] = 0 when in_len[b] <= 0, when no path
 *   exists (in_len[b] < L + number of adjacent equal labels; the reference returns garbage
 *   there) or when a label is outside [0, V). Other utterances of the launch are unaffected.
 *   ws: caller-owned back-pointers, AVSR_CTC_ALIGN_WS(B, T, Lmax) BYTES (one byte per
 *   (b, t, state), rounded up to whole dwords; 4-byte aligned, AVSR_E_ALIGN otherwise);
 *   contents on entry are irrelevant. Label-length bound as avsr_ctc_fwd:
 *   2*Lmax + 1 <= 1024 (AVSR_E_SHAPE beyond it); T is not bounded. No allocation, no sync.
 * ------------------------------------------------------------------------------------ */
typedef struct {
  int dtype, B, T, V, Lmax, blank;     /* dtype of x: AVSR_F32 or AVSR_BF16 */
  const void* x; int64_t ldx;          /* logits, rows b*T + t, V valid columns */
  const float* lse;                    /* [B*T] */
  const int* labels;                   /* [B][Lmax] */
  const int* label_len; const int* in_len;   /* [B] */
  unsigned char* ws;                   /* AVSR_CTC_ALIGN_WS(B, T, Lmax) bytes */
  int* ali;                            /* [B][T] */
  float* score;                        /* [B] */
  int* feasible;                       /* [B] */
} avsr_ctc_align_params;
#define AVSR_CTC_ALIGN_WS(B, T, Lmax) (((int64_t)(B) * (T) * (2 * (int64_t)(Lmax) + 1) + 3) & ~(int64_t)3)
int avsr_ctc_align(const avsr_ctc_align_params* p, void* stream);

/* ------------------------------------------------------------------------------------
 * avsr_ctc_align_long: avsr_ctc_align for whole recordings (avsr_amd/longform.py): the same
 *   parameter struct and the same definition -- emissions, recursion, skip rule, first-maximum
 *   back-pointer and final state, the ali / score / feasible fills and every infeasibility rule
 *   (label_len[b] outside [0, Lmax] included) -- so a float32 host Viterbi reproduces ali and
 *   score bit for bit, and where both kernels apply they return the same. The differences:
 *   Label-length bound: Lmax <= AVSR_CTC_ALIGN_LONG_LMAX = 16383 (S <= 32767 states;
 *   AVSR_E_SHAPE beyond it); T is not bounded. One 1024-thread workgroup per recording.
 *   ws: AVSR_CTC_ALIGN_LONG_WS(B, T, Lmax) BYTES: back-pointers of 2 bits per (b, t, state), a
 *   (b, t) row padded to 16 bytes (T = 30000, Lmax = 6000: 90 MB); 16-byte aligned,
 *   AVSR_E_ALIGN otherwise; contents on entry are irrelevant.
 *   No allocation, no sync, no atomics.
 * ------------------------------------------------------------------------------------ */
#define AVSR_CTC_ALIGN_LONG_LMAX 16383
#define AVSR_CTC_ALIGN_LONG_WS(B, T, Lmax) \
  ((int64_t)(B) * (T) * (((2 * (int64_t)(Lmax) + 1 + 63) >> 6) << 4))
int avsr_ctc_align_long(const avsr_ctc_align_params* p, void* stream);

/* ------------------------------------------------------------------------------------
 * avsr_ctc_align_gaps: avsr_ctc_align_long for a transcript that covers only PART of its
 *   recording (avsr_amd/longform.py, align_partial): material before the first word, after the
 *   last one, or between two words that nobody transcribed. The gap sits ON THE BLANK STATES, so
 *   the 2L + 1 topology, the back-pointers, the workspace (AVSR_CTC_ALIGN_LONG_WS, 16-byte
 *   aligned) and the bound (AVSR_CTC_ALIGN_LONG_LMAX) are those of avsr_ctc_align_long. Inputs
 *   beyond its:
 *     gap[b][i], i = 0..label_len[b] (row stride Lmax + 1): non-zero marks the blank state 2i as
 *       a GAP STATE. Flag 0 frees the start, flag L the end, flag i says that something
 *       untranscribed may have been said between token i and token i + 1 (1-based tokens).
 *     filler[b*T + t] (<= 0): the log-probability a gap state may take at frame t instead of the
 *       blank's; the Python layer passes the greedy reading max_v float(x[t][v]) - lse[t].
 *     gap_penalty (<= 0, -inf allowed): added to the filler per frame.
 *   With eb = float(x[t][blank]) - lse[t] and ef = filler[t] + gap_penalty (ONE fp32 add), a gap
 *   state emits ef where ef > eb (strictly), else eb. That is the only change: every other
 *   emission, the recursion, the skip rule, the first-maximum back-pointer order (s, s-1, s-2),
 *   the start states (0, 1), the final-state rule and every infeasibility rule are those of
 *   avsr_ctc_align; the minimum number of frames stays L + adjacent repeats. A skip across a gap
 *   state stays legal, so a flagged gap that holds nothing costs nothing.
 *   ali[b][t] as before, except that a frame spent in a gap state with ef > eb is written as
 *   AVSR_CTC_ALIGN_GAP; score[b] counts those frames at ef. With all flags 0, or with
 *   gap_penalty = -inf, ali and score equal avsr_ctc_align_long's bit for bit; a float32 host
 *   Viterbi reproduces everything bit for bit.
 *   AVSR_E_ARG beyond avsr_ctc_align_long's: gap or filler NULL with B > 0 and T > 0;
 *   gap_penalty NaN or > 0. A NaN or positive filler VALUE is not checked: the result for that
 *   recording is then unspecified (other recordings of the launch are unaffected).
 *   No allocation, no sync, no atomics.
 * ------------------------------------------------------------------------------------ */
#define AVSR_CTC_ALIGN_GAP (-2)
typedef struct {
  int dtype, B, T, V, Lmax, blank;     /* the fields of avsr_ctc_align_params ... */
  const void* x; int64_t ldx;
  const float* lse;
  const int* labels;
  const int* label_len; const int* in_len;
  unsigned char* ws;                   /* AVSR_CTC_ALIGN_LONG_WS(B, T, Lmax) bytes */
  int* ali;
  float* score;
  int* feasible;
  const unsigned char* gap;            /* ... followed by: [B][Lmax + 1] */
  const float* filler;                 /* [B*T] */
  float gap_penalty;
} avsr_ctc_align_gaps_params;
int avsr_ctc_align_gaps(const avsr_ctc_align_gaps_params* p, void* stream);

/* ------------------------------------------------------------------------------------
 * avsr_ctc_neighbors: the exact CTC log-likelihood of every ONE-EDIT NEIGHBOUR of a label
 *   sequence, for B utterances in one call (the reference has no counterpart; token and word
 *   confidences, avsr_amd/confidence.py). For y = y_1..y_L over n = min(in_len[b], T) frames and a
 *   slot l, the neighbours are y with y_l replaced by v, for every vocabulary token v, and y with
 *   y_l deleted. Setup, all in fp32:
 *     e(t,k) = float(x[t][k]) - lse[t]
 *     ext = blank, y_1, blank, ..., y_L, blank with S = 2L + 1 states; y_j sits at state 2j - 1
 *     alpha_t(s), beta_t(s): the CTC forward / backward variables of y; beta_t(s) includes
 *     e(t, ext_s); frames run 0..n-1
 *   Substitution at slot l, state m = 2l - 1, token v (v != blank, v != eos, 0 <= v < V):
 *     a_0 = e(0,v) if l == 1 else -inf
 *     a_t = e(t,v) + LSE( a_{t-1}, alpha_{t-1}(m-1), [l >= 2 and v != y_{l-1}] alpha_{t-1}(m-2) )
 *     sub[l][v] = LSE_{t <= n-2}( a_t + LSE( beta_{t+1}(m+1), [l < L and v != y_{l+1}] beta_{t+1}(m+2) ) )
 *                 (+) a_{n-1} if l == L
 *   so sub[l][v] = log p_ctc(y_1..y_{l-1}, v, y_{l+1}..y_L | x), and sub[l][y_l] = log p_ctc(y | x)
 *   for every l (up to rounding). Deletion at slot l, del[l] = log p_ctc(y without y_l | x):
 *     1 < l < L:  LSE_{t <= n-2}( LSE( alpha_t(2l-2), [y_{l-1} != y_{l+1}] alpha_t(2l-3) ) + beta_{t+1}(2l+1) )
 *     l = 1 < L:  the same without the alpha_t(2l-3) term, (+) beta_0(3)
 *     l = L > 1:  LSE( alpha_{n-1}(2L-2), alpha_{n-1}(2L-3) )
 *     L = 1:      alpha_{n-1}(0), the all-blank path
 *   A neighbour with no CTC path (a substitute that creates an adjacent repeat the frames cannot
 *   separate) is -inf exactly, not an error: unreachable states are -inf, never a large negative.
 *   Slot posterior: Z_l = LSE( sub[l][v] over allowed v, del[l] ); conf_ctc(l) =
 *   exp(sub[l][y_l] - Z_l) in (0, 1]; an alternative v has exp(sub[l][v] - Z_l), the deletion
 *   exp(del[l] - Z_l). lz[b][l] (optional, NULL: not computed) = Z_l - base[b], accumulated
 *   relative to the row maximum so that it carries fp32 rounding of a value near 0, not of Z_l.
 *   Insertions (a token between two slots) are not neighbours here.
 *   Outputs, slots 0-based in memory (slot l above is row l - 1); EVERY element is written:
 *     sub[b][l][0..lds): -inf in the blank and eos columns (eos = -1: none excluded), in columns
 *       V..lds-1 and in rows l >= label_len[b];  del[b][l], lz[b][l]: -inf for l >= label_len[b];
 *     base[b] = log p_ctc(y | x);  feasible[b] = 1 if the utterance was computed.
 *   feasible[b] = 0, base[b] = 0 and -inf everywhere else when in_len[b] <= 0, when y has no path
 *   (in_len[b] < L + number of adjacent equal labels), when a label is outside [0, V) or equals
 *   blank, or when label_len[b] is outside [0, Lmax] (avsr_ctc_align's rules). label_len[b] = 0 is
 *   feasible and has no slots. Frames t >= in_len[b] and columns >= V of x are never read.
 *   Utterances do not influence each other, and the result for an utterance is a function of its
 *   own inputs alone: no atomics, every reduction in a fixed order (time ascending per (slot, v);
 *   lz by a fixed tree over the row).
 *   ws: caller-owned alpha and beta, AVSR_CTC_NEIGHBORS_WS(B, T, Lmax) BYTES ([B][T][2*Lmax+1]
 *   floats each), 16-byte aligned (AVSR_E_ALIGN otherwise); contents on entry are irrelevant.
 *   Limits: 2*Lmax + 1 <= 1024 (AVSR_E_SHAPE beyond it) as avsr_ctc_fwd; T is not bounded;
 *   lds >= V. No allocation, no host sync.
 * ------------------------------------------------------------------------------------ */
typedef struct {
  int dtype, B, T, V, Lmax, blank, eos;   /* dtype of x: AVSR_F32 or AVSR_BF16; eos -1: none */
  const void* x; int64_t ldx;          /* logits, rows b*T + t, V valid columns */
  const float* lse;                    /* [B*T] */
  const int* labels;                   /* [B][Lmax] */
  const int* label_len; const int* in_len;   /* [B] */
  void* ws;                            /* AVSR_CTC_NEIGHBORS_WS(B, T, Lmax) bytes */
  float* sub; int64_t lds;             /* [B][Lmax][lds] */
  float* del;                          /* [B][Lmax] */
  float* base;                         /* [B] */
  int* feasible;                       /* [B] */
  float* lz;                           /* [B][Lmax] or NULL */
} avsr_ctc_neighbors_params;
#define AVSR_CTC_NEIGHBORS_WS(B, T, Lmax) \
  ((((int64_t)(B) * (T) * (2 * (int64_t)(Lmax) + 1) * 2 * 4) + 15) & ~(int64_t)15)
int avsr_ctc_neighbors(const avsr_ctc_neighbors_params* p, void* stream);

/* ------------------------------------------------------------------------------------
 * avsr_ctc_beam: time-synchronous CTC prefix beam search (the first pass of two-pass decoding,
 *   avsr_amd/rescore.py; the reference has no such search) of U utterances in one launch, over
 *   fp32 CTC log-probs logp (rows u*Tm + t, ldp floats apart) and C candidate tokens per frame
 *   cand[u][t][0..C) (avsr_row_topk / avsr_log_softmax_topk order). Defined as if `next` were a
 *   dictionary keyed by the token string; a (+)= b is a = logaddexp(a, b), all in fp32:
 *     beam = {(): pb = 0, pnb = -inf}
 *     for t < tlen[u], for every prefix l of the beam in rank order, tot = logaddexp(pb, pnb):
 *       next[l].pb (+)= tot + logp[t][blank]                (blank need not be in cand)
 *       for each candidate c in column order, p = logp[t][c]; c == blank, c == eos (never a
 *       CTC label) and c outside [0, V) are skipped:
 *         c == last(l):  next[l].pnb (+)= pnb + p;  next[l + c].pnb (+)= pb + p
 *         otherwise:     next[l + c].pnb (+)= tot + p
 *         (no extension beyond Lcap tokens)
 *       beam = the N entries of next with the largest logaddexp(pb, pnb); ties go to the entry
 *       created first (parent rank ascending, stay before extend, candidate column ascending;
 *       an entry that was already in the beam counts as created by its own stay)
 *   Outputs, best first: n_out[u] <= N; len[u][r]; score[u][r] = logaddexp(pb, pnb);
 *   tokens[u][r][0..len). Fill values: tokens -1 beyond len and for r >= n_out, len 0 and score
 *   -inf for r >= n_out. tlen[u] <= 0 gives n_out[u] = 0; tlen[u] > Tm is read as Tm. Padding
 *   frames (t >= tlen[u]) are never read. Utterances do not influence each other: one
 *   workgroup each, and the result is a function of that utterance's inputs alone (selection by
 *   rank counting, no atomics).
 *   Identity of a prefix is (length, 64-bit hash of the token string), so equal strings merge
 *   however they were reached: an extension that is already in the beam, and a prefix that left
 *   the beam and is re-created while an old extension of it survived. Two different strings of
 *   one length collide with probability 2^-64 per comparison, at most Tm * N * (N + N*C)
 *   comparisons per utterance (< 1e-12 at Tm = 1000, N = C = 16); the strings are therefore not
 *   compared token by token (that walk would cost a dependent chain of len global reads per
 *   comparison, every frame).
 *   ws: caller-owned prefix tree (parent node, token) of the kept extensions,
 *   AVSR_CTC_BEAM_WS(U, Tm, N) BYTES, 8-byte aligned (AVSR_E_ALIGN otherwise); contents on entry
 *   are irrelevant. Limits: 1 <= N <= 16, 1 <= C <= 16, 0 <= Lcap <= 511 (so that a returned
 *   hypothesis fits avsr_ctc_fwd's 2L + 1 <= 1024), AVSR_E_SHAPE beyond them. No allocation,
 *   no host sync.
 * ------------------------------------------------------------------------------------ */
typedef struct {
  int U, Tm, V, N, C, blank, eos, Lcap;
  const float* logp; int64_t ldp;      /* [U*Tm][ldp], V valid columns */
  const int* tlen;                     /* [U] */
  const int* cand;                     /* [U][Tm][C] */
  void* ws;                            /* AVSR_CTC_BEAM_WS(U, Tm, N) bytes */
  int* n_out;                          /* [U] */
  int* tokens;                         /* [U][N][Lcap] */
  int* len;                            /* [U][N] */
  float* score;                        /* [U][N] */
} avsr_ctc_beam_params;
#define AVSR_CTC_BEAM_WS(U, Tm, N) ((int64_t)(U) * ((int64_t)(Tm) * (N) + 1) * 8)
int avsr_ctc_beam(const avsr_ctc_beam_params* p, void* stream);

/* ------------------------------------------------------------------------------------
 * avsr_ctc_kws: keyword spotting on CTC posteriors (avsr_amd/kws.py; the reference has no
 *   counterpart): the CTC Viterbi of each of K keywords with a FREE START and a FREE END inside
 *   each of U utterances, one launch, over fp32 CTC log-probs logp (rows u*Tm + t, ldp floats
 *   apart, V valid columns, as for avsr_ctc_beam). For a pair (u, k), all in fp32, with
 *   y = labels[k][0..L), L = label_len[k], n = min(tlen[u], Tm):
 *     ext = y1, blank, y2, blank, ..., yL              S = 2L - 1 states (no outer blanks)
 *     f(t)   = logp[t][top[t]]  (0 when top == NULL)    the filler: the frame's best token
 *     r(t,s) = logp[t][ext_s] - f(t)                    a log-ratio, <= 0 with a filler
 *     skip(s) = s >= 2 and ext_s != blank and ext_s != ext_{s-2}
 *     before frame 0 every state is -inf with start -1; for t = 0 .. n-1:
 *       m, b = d[t-1][s], st[t-1][s]
 *       if s >= 1 and d[t-1][s-1] > m: m, b = d[t-1][s-1], st[t-1][s-1]
 *       if skip(s) and d[t-1][s-2] > m: m, b = d[t-1][s-2], st[t-1][s-2]
 *       if s == 0 and 0 > m:            m, b = 0, t     the keyword may begin at any frame; the
 *                                                       filler before it costs nothing
 *       d[t][s] = m + r(t,s);  st[t][s] = b  (-1 where d[t][s] is -inf)
 *     score = max over t of d[t][S-1]; on ties the LAST such t wins (update on >=)
 *     end = t* + 1;  start = st[t*][S-1]               the keyword spans frames [start, end)
 *   Every comparison is strict and the order is stay, s-1, s-2, enter, so a run of frames that
 *   tie (the keyword's own argmax run) falls wholly inside the span. The only arithmetic is one
 *   subtraction and one addition per cell: a float32 host DP reproduces score, start and end bit
 *   for bit. With a filler the score is the log-ratio of the keyword's best path over its span to
 *   the frame-wise best tokens over the same span (0 when the keyword IS the greedy reading).
 *   top[u*Tm + t] is the row argmax (avsr_log_softmax_topk with K = 1); a value outside [0, V) is
 *   read as the nearest valid column.
 *   Outputs, EVERY element is written: score[u][k], start[u][k], end[u][k]; optional
 *   trace[u][k][t] = d[t][S-1] and tstart[u][k][t] = st[t][S-1] (both or neither; -inf / -1 for
 *   t >= n). A pair with no path gets score = -inf, start = end = -1 (trace -inf, tstart -1):
 *   n <= 0, n < L + the number of adjacent equal labels, L outside [1, Lmax], a label outside
 *   [0, V) or equal to blank. Other pairs of the launch are unaffected.
 *   Frames t >= tlen[u], columns >= V and labels[k][l >= L] are never read. Pairs do not
 *   influence each other (one wavefront each, one state per lane, no LDS); no atomics, no
 *   allocation, no host sync.
 *   Limits: 1 <= Lmax <= 32 (S <= 63: one state per lane), K >= 1, 1 <= U <= 65535, Tm >= 1,
 *   AVSR_E_SHAPE beyond them; p NULL, a NULL required pointer, blank outside [0, V), ldp < V, or
 *   trace given without tstart (or the reverse): AVSR_E_ARG.
 * ------------------------------------------------------------------------------------ */
typedef struct {
  int U, Tm, V, K, Lmax, blank;
  const float* logp; int64_t ldp;      /* [U*Tm][ldp], V valid columns */
  const int* tlen;                     /* [U] */
  const int* top;                      /* [U*Tm] row argmax, or NULL: no filler */
  const int* labels;                   /* [K][Lmax] */
  const int* label_len;                /* [K] */
  float* score; int* start; int* end;  /* [U][K] */
  float* trace; int* tstart;           /* [U][K][Tm], or both NULL */
} avsr_ctc_kws_params;
int avsr_ctc_kws(const avsr_ctc_kws_params* p, void* stream);

/* ------------------------------------------------------------------------------------
 * Elementwise / data-movement kernels around the GEMMs.
 * avsr_ew_bwd:     out = alpha * dy * dropmask(drop_p, seed; idx = row*N + col) * act'(gate),
 *                  db[n] += sum_rows out  (bias gradients of the Linear layers; out optional)
 * avsr_dropout_fwd: out = dy * dropmask (nn.Dropout on a [rows][N] view: CTC input dropout
 *                  ctc.py:27,98, encoder dropout after pos-conv avhubert.py:704)
 * avsr_mask_rows:  x[b*T + t][:] = 0 for t >= len[b]   (avhubert.py:683-686)
 * avsr_embed_fwd:  y[r] = dropout(table[tok[r]] * scale + pe[r % L])  (decoder embed +
 *                  PositionalEncoding, decoder.py:89-93, embedding.py:80-87); bwd: dtable
 *                  += per-token sums of the row gradients in row order (no atomics)
 * avsr_cast:       dst = alpha * src + beta * dst over a [rows][cols] strided view
 * avsr_cast_flat:  dst = src over n contiguous elements (fp32 <-> bf16 vectorised: the arena's
 *                  master -> compute-shadow refresh after load_state_dict / optimizer steps; the
 *                  bf16-compressed gradient all-reduce's compress / decompress)
 * avsr_stem_pack:  videos (B,1,T,88,88) fp32 -> (B*T, 88, 88, 8): channel c = frame t+c-2
 *                  (c < 5, zero outside [0,T)), the Conv3d(k=5x7x7, pad 2x3x3) stem as a 2-D conv
 * avsr_stem_wpack / avsr_stem_wgrad_unpack: Conv3d weight (64,1,5,7,7) <-> [64][7][7][8]
 * avsr_audio_pack: audios (B, F, T) fp32 -> (B*T, F)  (SubModel.proj input, avhubert.py:194-196)
 * avsr_weightnorm_fwd/bwd: w = g * v / ||v|| per tap k, v stored [o][k][c] (HF weight_norm
 *                  dim=2 of the pos-conv, modeling_wav2vec2.py:336-356)
 * avsr_sumsq / avsr_adamw: fused clip_grad_norm_(max_norm) + torch.optim.AdamW step over a
 *                  flat fp32 parameter range; optionally refreshes the bf16 shadow copy
 * ------------------------------------------------------------------------------------ */
typedef struct {
  int dtype, rows, N;
  const void* dy; int64_t lddy;
  void* out; int64_t ldout;
  const void* gate; int64_t ldgate; int act;
  float drop_p; uint64_t seed;
  float alpha;
  float* db;
  float* ws;                                       /* with db: workspace >= AVSR_EW_WS(N) floats */
} avsr_ew_params;
#define AVSR_EW_ROWBLOCKS 256
#define AVSR_EW_WS(N) (AVSR_EW_ROWBLOCKS * (N))
int avsr_ew_bwd(const avsr_ew_params* p, void* stream);
/* Deferred finalisation of the column-sum partials (bias gradients of avsr_ew_bwd /
 * avsr_gemm db, LayerNorm dgamma/dbeta): between avsr_colsum_defer(1) and avsr_colsum_flush the
 * finalise passes are queued on the host and a flush reduces all of them in one batched launch
 * on `stream` (stream-ordered after the producers). The caller keeps the partial workspaces
 * alive until the flush. avsr_colsum_defer returns the previous setting. (A training step's
 * ~200 separate 5 us finalise launches become one per encoder layer.) */
int avsr_colsum_defer(int on);
int avsr_colsum_flush(void* stream);
/* avsr_colsum_inline(1): finalise passes launch at once on their producer's stream even while
 * deferral is on (the queue is left untouched) -- for a column sum issued on another stream
 * than the flush (the weight-grad side stream); returns the previous setting */
int avsr_colsum_inline(int on);
int avsr_dropout_fwd(const avsr_ew_params* p, void* stream);
int avsr_mask_rows(int dtype, int B, int T, int N, void* x, int64_t ldx, const int* len, void* stream);

typedef struct {
  int dtype, rows, L, D;
  const int* tok; const void* table; const float* pe; float scale;
  void* y; float drop_p; uint64_t seed;
  const void* dy; float* dtable;
  const int* pe_row;         /* forward, optional: device int, every row adds pe[pe_row[0]] (L ignored):
                                the position of a beam-search step kept on the device */
  int pe_row_stride;         /* 0: the one shared position above; 1: row r adds pe[pe_row[r]] */
} avsr_embed_params;
int avsr_embed_fwd(const avsr_embed_params* p, void* stream);
int avsr_embed_bwd(const avsr_embed_params* p, void* stream);

int avsr_cast(int src_dtype, int dst_dtype, int rows, int cols, const void* src, int64_t lds,
              void* dst, int64_t ldd, float alpha, float beta, void* stream);
int avsr_cast_flat(int src_dtype, int dst_dtype, int64_t n, const void* src, void* dst, void* stream);
int avsr_stem_pack(int dtype, int B, int T, const float* video, void* out, void* stream);
int avsr_stem_wpack(int dtype, const float* w, void* wp, void* stream);
/* avsr_stem_conv_fwd (bf16): the stem Conv3d (resnet.py:132) read straight from videos
 *                  (B,1,T,88,88) fp32 (zero frames outside the clip) -> h [B*T][44][44][64] bf16,
 *                  and (stats != NULL) BN partials stats[64][avsr_stem_conv_tiles(B, T)][3]
 *                  (count, mean, M2) as avsr_conv_fwd writes them; wk from avsr_stem_wpack2:
 *                  [64][288] bf16, k = (dt*7 + kh)*8 + kw (kw = 7 and k >= 280 zero) */
int avsr_stem_conv_tiles(int B, int T);
int avsr_stem_wpack2(const float* w, void* wk, void* stream);
int avsr_stem_conv_fwd(int B, int T, const float* video, const void* wk, void* h, float* stats, void* stream);
int avsr_stem_wgrad_unpack(const float* gp, float* gw, void* stream);
int avsr_audio_pack(int dtype, int B, int F, int T, const float* audio, void* out, void* stream);

int avsr_weightnorm_fwd(int dtype, int O, int K, int C, const float* v, const float* g, float* norm,
                        void* w, void* stream);
int avsr_weightnorm_bwd(int O, int K, int C, const float* v, const float* g, const float* norm,
                        const float* dw, float* dv, float* dg, float* scratch, void* stream);

/* *out += sum x^2 in a fixed summation order (deterministic); ws: AVSR_SUMSQ_WS floats */
#define AVSR_SUMSQ_WS 1024
int avsr_sumsq(const float* x, int64_t n, float* out, float* ws, void* stream);
typedef struct {
  int64_t n;
  float* param; const float* grad; float* exp_avg; float* exp_avg_sq;
  void* shadow; int shadow_dtype;        /* bf16 copy of the updated params, or NULL */
  float lr, beta1, beta2, eps, weight_decay;
  float bias_corr1, bias_corr2;          /* 1 - beta^t */
  const float* sumsq; float max_norm;    /* clip: coef = min(1, max_norm / (sqrt(*sumsq) + 1e-6)); sumsq NULL = no clip */
  float grad_scale;                      /* extra multiplier on the gradient (1/accumulation etc.) */
  int max_blocks;                        /* grid cap (0: 4096 = the whole chip). An update running
                                            beside other work on another stream takes fewer, so its
                                            grid-stride blocks leave CU slots to that work; the
                                            result does not depend on it */
  float* grad_clear;                     /* NULL, or = grad: each gradient element is set to 0 after the
                                            update has read it (the next step's gradient clear done
                                            by the update, e.g. while it overlaps the next forward) */
} avsr_adamw_params;
int avsr_adamw(const avsr_adamw_params* p, void* stream);

/* ------------------------------------------------------------------------------------
 * Joint CTC / attention beam search. Replaces, for the decoder
 * that get_beam_search_decoder builds (src/avhubert_avsr/avhubert_avsr_model.py:12-36):
 *   Decoder.batch_score / forward_one_step    src/nets/backend/transformer/decoder.py:153-227
 *     (one query per hypothesis; the reference recomputes the cross-attention K/V of the
 *      memory every step, here they are computed once per utterance)
 *   CTCPrefixScoreTH.__call__                 src/nets/ctc_prefix_score.py:65-187
 *   BatchBeamSearch.search / batch_beam       src/nets/batch_beam_search.py:102-260
 *   index_select of the hypothesis states     src/nets/batch_beam_search.py:53-66
 * avsr_log_softmax_rows: out[r][c] = x[r][c] - max - log(sum exp(x - max)), c < V (fp32 out)
 * avsr_dec_attn: o[i][h*64..] = softmax(scale * q_i k_j^T, j < klen[i]) v  per hypothesis i
 *   and head h; key j of hypothesis i at k[i*k_bstride + j*ldk + h*64] (bstride 0: the keys
 *   are shared, e.g. the encoder memory). dynamic LDS: (klen_max + 256) * 4 bytes.
 * avsr_row_topk: ids[r][0..K) = indices of the K largest x[r][c], c < V, descending
 *   (ties: smaller index first); K <= 16.
 * avsr_ctc_prefix: for hypothesis h (prefix length out_len + 1 incl. sos, last token
 *   last[h], CTC forward variables r_prev[h][T][2] or NULL at the first step) and its P
 *   scored tokens ids[h][:]: r_new[h][j][T][2] and psi[h][j] = log prefix probability
 *   (LOGZERO for blank, r_sum[T-1] for eos), psi[h][P] = r_sum[T-1] (the eos score).
 *   A prefix longer than the utterance (out_len > T: a dead row of a search that runs past its
 *   frames) is scored as one of length T: both kernels keep every frame index below T.
 * avsr_beam_select: weighted[h][v] = w_dec*dec[h][v] + w_ctc*(psi(h,v) - s_prev[h]) +
 *   score[h]; the beam best (h, v) in descending order -> out_prev/out_tok/out_score,
 *   out_dec = dec[h][v], out_ctc = psi - s_prev, out_s = psi, out_col = column of v in
 *   ids[h] (P-1 when v was not scored, the reference's scoring_idmap -1 index).
 * Batched decoding (several utterances per step, avsr_amd.decode.BatchBeamSearch.decode_batch):
 *   the optional kidx / uidx+tlen / nseg+seg fields route each hypothesis to its utterance's
 *   memory, CTC log-probs and beam selection; the reference decodes one utterance at a time
 *   (script/evaluation.py:280-296), results are identical per utterance.
 * avsr_gather_rows: dst[g][i] = src[g][idx[i]] for i < n, rows of row_bytes; sizes, strides and
 *   pointers multiples of 4 bytes (16-byte words when everything is 16-byte aligned).
 * ------------------------------------------------------------------------------------ */
int avsr_log_softmax_rows(int dtype, int rows, int V, const void* x, int64_t ldx, float* out, int64_t ldo,
                          void* stream);

typedef struct {
  int dtype, n, H, klen_max;
  float scale;
  const void* q; int64_t ldq;
  const void* k; int64_t ldk, k_bstride;
  const void* v; int64_t ldv, v_bstride;
  const int* klen;            /* [n] or NULL (= klen_max) */
  void* o; int64_t ldo;
  const int* kidx;            /* [n] or NULL: hypothesis i reads key block kidx[i] (base kidx[i]*k_bstride,
                                 v likewise) instead of block i — batched decoding of several
                                 utterances whose memories sit in one [U][T][..] buffer */
  const int* kmap; int64_t ldmap;   /* optional [n][ldmap]: key j of hypothesis i is row kmap[i*ldmap + j]
                                 of k (v likewise; bstride / kidx ignored) — the self-attention
                                 cache of a device-side beam search, [step][row] rows addressed
                                 through each hypothesis's ancestry instead of being reordered */
  int group;                  /* >= 1 (0 = 1): hypotheses i0 .. i0+group-1 (i0 % group == 0) share one
                                 key block and klen (kidx / klen equal within a group, no kmap; the
                                 beams of one utterance over its memory): one workgroup reads each
                                 key / value row once for all of them */
  int ksplit;                 /* >= 2: a workgroup row's keys split over up to ksplit workgroups
                                 (min(ksplit, ceil(klen / 192)) of them: a function of the row's
                                 klen only), each writing (max, sum, unnormalised o) partials to
                                 ws; the last-arriving one (counter cnt[group][head], zeroed by
                                 the caller once, left zero) merges them in split order. 0 / 1: none */
  float* ws;                  /* ksplit >= 2: ceil(n / group) * H * ksplit * group * 66 floats */
  unsigned* cnt;              /* ksplit >= 2: ceil(n / group) * H counters */
} avsr_dec_attn_params;
int avsr_dec_attn(const avsr_dec_attn_params* p, void* stream);

typedef struct {
  int rows, V, K;
  const float* x; int64_t ldx;
  int* ids;                   /* [rows][K] */
} avsr_topk_params;
int avsr_row_topk(const avsr_topk_params* p, void* stream);
/* avsr_log_softmax_topk: avsr_log_softmax_rows followed by avsr_row_topk on its output, in one
 * pass over each row (decode steps: the decoder output layer's log-probs and the pre-beam,
 * batch_beam_search.py:228-236 + scorers/ctc.py pre-beam); results identical to the two calls */
int avsr_log_softmax_topk(int dtype, int rows, int V, const void* x, int64_t ldx, float* out, int64_t ldo,
                          int K, int* ids, void* stream);

typedef struct {
  int n, T, V, P;
  int blank, eos, out_len;
  const float* logp;          /* [T][V] CTC log-probs */
  const float* r_prev;        /* [n][T][2] or NULL (first step) */
  const int* last;            /* [n] */
  const int* ids;             /* [n][P] */
  float* r_new;               /* [n][P][T][2] */
  float* psi;                 /* [n][P+1] */
  /* batched utterances (uidx NULL: one utterance): hypothesis h scores utterance uidx[h],
   * whose log-probs start at logp + uidx[h]*logp_ustride and whose length is tlen[uidx[h]]
   * (<= T, the row stride of r_prev / r_new) */
  const int* uidx; int64_t logp_ustride; const int* tlen;
  const int* out_len_dev;     /* optional device int overriding out_len (graph-captured steps) */
  int out_len_stride;         /* 0: out_len_dev is one shared int; 1: one length per hypothesis row,
                                 out_len_dev[h]. In that form a row of length 0 computes what a launch
                                 with r_prev == NULL computes (the blank cumulative sum as the previous
                                 state, r0(0) = logp[id]) whatever r_prev holds: "first step" is a
                                 property of the row, not of the launch */
} avsr_ctc_prefix_params;
int avsr_ctc_prefix(const avsr_ctc_prefix_params* p, void* stream);

typedef struct {
  int n, V, P, beam;
  int blank, eos;
  float w_dec, w_ctc;
  const float* dec; int64_t ld;        /* decoder log-probs [n][ld] */
  const int* ids;                      /* [n][P] */
  const float* psi;                    /* [n][P+1] */
  const float* s_prev;                 /* [n] */
  const float* score;                  /* [n] */
  int* out_prev; int* out_tok; int* out_col;
  float* out_score; float* out_dec; float* out_ctc; float* out_s;
  /* batched utterances (nseg 0: one selection over all n rows): selection u runs over rows
   * [seg[u], seg[u+1]) and writes out_*[u*beam + r]; out_prev is the global row index */
  int nseg; const int* seg;
  /* hot-word biasing (NULL: off, the selection above unchanged). bonus / next [n][P+1] as
   * avsr_hotword_step writes them for this launch's ids (P counts its continuation columns):
   * weighted[h][v] = w_dec*dec + w_ctc*(psi - s_prev) + bonus[h][c] + score[h], the four terms
   * added in this order, c = the column of v in ids[h], or P for eos and for every token outside
   * ids[h] (such a token leaves a started phrase like eos does). out_bonus = the selected bonus,
   * out_next = next[h][c]; both set together with bonus (next may be NULL with out_next). */
  const float* bonus; const int* next;
  float* out_bonus; int* out_next;
  /* n-gram LM shallow fusion and the length bonus (lm NULL and w_len 0: off, the selection above
   * unchanged, arithmetic included). lm / lm_next [n][P+1] as avsr_ngram_step writes them for this
   * launch's ids. The sum follows the reference's order (batch_beam_search.py:222-245: full scorers
   * in the order of its scorer dict, then partial scorers, then the running score):
   *   weighted[h][v] = w_dec*dec + w_len*1 + w_lm*lm[h][c] + w_ctc*(psi - s_prev) [+ bonus] + score[h]
   * c = the column of v in ids[h], or P for eos. A token outside ids[h] takes an LM term of 0: it
   * sits at w_ctc*LOGZERO ~ -1e9*w_ctc, where one fp32 step exceeds any LM score. lm_hi: an upper
   * bound on any lm value (NgramLM.lm_hi), for the bound of the candidates-only pass.
   * out_lm = the selected (unweighted) LM score, out_lm_next = lm_next[h][c]; for a token outside
   * ids[h] 0 and -1 (out of range, which avsr_ngram_step reads as the <s> state). */
  const float* lm; const int* lm_next;
  float w_lm, w_len, lm_hi;
  float* out_lm; int* out_lm_next;
} avsr_beam_select_params;
int avsr_beam_select(const avsr_beam_select_params* p, void* stream);

/* ------------------------------------------------------------------------------------
 * Hot-word biasing of the beam search (avsr_amd/hotwords.py builds the tree; the reference has
 * no counterpart: its scorers are host objects, src/nets/scorer_interface.py). A prefix tree over
 * the user's phrases in CSR form: the children of node n are entries [child_off[n],
 * child_off[n+1]) of child_tok (ascending) / child_node; node 0 is the root; pend[n] = depth(n)
 * minus the depth of the nearest terminal ancestor-or-self (0 without one); terminal[n] = a phrase
 * ends at n. Row r of the search stands at node[r] (the root for sos).
 * avsr_hotword_step, once per step after the pre-beam: the row's candidate ids
 *   ids[r][0..P) = ids_pre[r][:], ids[r][P + j] = the j-th child token of node[r] for a non-root
 *   node (j < C = AVSR_HOTWORD_C), or blank when there is none or the pre-beam already holds it
 *   (no candidate twice); and for every column c < P + C and the eos column c = P + C:
 *   bonus[r][c] = beta * (float)k and next[r][c], where for the column's token v
 *     child(node, v) = m exists:  k = 1, next = m, or the root if m is terminal without children
 *     v is eos or blank:          k = -pend[node], next = root
 *     otherwise:                  k = -pend[node]; then child(root, v) = m exists: k += 1 and
 *                                 next = m (same terminal rule), else next = root
 *   A node outside [0, nodes) is read as the root. The CTC prefix scores, the selection and the
 *   bookkeeping then run over P + C columns. */
enum { AVSR_HOTWORD_C = 8 };
typedef struct {
  int R, P, C, nodes;
  int blank, eos;
  float beta;
  const int* child_off;       /* [nodes + 1] */
  const int* child_tok;       /* [nodes - 1] */
  const int* child_node;      /* [nodes - 1] */
  const int* pend;            /* [nodes] */
  const int* terminal;        /* [nodes] */
  const int* node;            /* [R] */
  const int* ids_pre;         /* [R][P] */
  int* ids;                   /* [R][P + C] */
  float* bonus;               /* [R][P + C + 1] */
  int* next;                  /* [R][P + C + 1] */
} avsr_hotword_params;
int avsr_hotword_step(const avsr_hotword_params* p, void* stream);

/* ------------------------------------------------------------------------------------
 * N-gram LM shallow fusion (avsr_amd/ngram_lm.py compiles the model and states the scoring rule;
 * the reference's counterpart is the "lm" slot of its scorer dict, a host object). A backoff
 * automaton over token ids in the CSR manner of the hot-word tree: node 0 is the empty context,
 * node n > 0 a context of 1 .. order-1 tokens with its backoff weight, its fail link (the node of
 * the context without its oldest token) and its entries [child_off[n], child_off[n+1]) of tok
 * (ascending) / logp / next; the empty context is dense (uni_logp / uni_next [V]; node 0 has no
 * span). start = the state of a fresh hypothesis, the node of (sos).
 *   score(n, v): acc = 0; while n != 0: entry (n, v) exists -> acc + logp, successor next;
 *                else acc += backoff[n], n = fail[n]; at node 0: acc + uni_logp[v], uni_next[v].
 * fp32 sums in that order.
 * avsr_ngram_step, once per search step after the pre-beam and avsr_hotword_step: for row r at
 *   state[r] (a value outside [0, nodes) is read as start) and each column c < P of ids[r] and the
 *   eos column c = P: out[r][c] = score, out_next[r][c] = successor. A blank column (padding of
 *   the hot-word widening) gets 0 and the row's own state. P + 1 <= 64.
 * avsr_ngram_score_seqs, for complete hypotheses: row b of tokens [n][L] (-1 padded), followed by
 *   eos, is scored from start: out[b][j] for j <= len(b) (the last one is eos), 0 beyond. */
enum { AVSR_NGRAM_MAX_ORDER = 6 };
typedef struct {
  int order, nodes, V, start;
  const int* child_off;       /* [nodes + 1] */
  const float* backoff;       /* [nodes] */
  const int* fail;            /* [nodes] */
  const int* tok;             /* [entries]; tok / logp / next all NULL: no entry below the unigram level */
  const float* logp;          /* [entries] */
  const int* next;            /* [entries] */
  const float* uni_logp;      /* [V] */
  const int* uni_next;        /* [V] */
} avsr_ngram_lm;
typedef struct {
  avsr_ngram_lm lm;
  int R, P, blank, eos;
  const int* state;           /* [R] */
  const int* ids;             /* [R][P] */
  float* out;                 /* [R][P + 1] */
  int* out_next;              /* [R][P + 1] */
} avsr_ngram_params;
int avsr_ngram_step(const avsr_ngram_params* p, void* stream);
typedef struct {
  avsr_ngram_lm lm;
  int n, L, eos;
  const int* tokens;          /* [n][L], -1 padded */
  float* out;                 /* [n][L + 1] */
} avsr_ngram_seq_params;
int avsr_ngram_score_seqs(const avsr_ngram_seq_params* p, void* stream);

int avsr_gather_rows(int groups, int n, int64_t row_bytes, const void* src, int64_t src_gstride,
                     int64_t src_rstride, void* dst, int64_t dst_gstride, int64_t dst_rstride,
                     const int* idx, void* stream);

/* Device-side beam bookkeeping (avsr_amd.decode: the whole step lives on the device and is
 * replayed as a HIP graph; the host reads only a done count every few steps and the history at
 * the end). Fixed geometry: U utterances x beam rows = R rows; a finished hypothesis / utterance
 * becomes a dead row (score -inf, never selected: identical to the reference removing it,
 * batch_beam_search.py:262-349, beam_search.py:330-372).
 * avsr_beam_step_prep: at the start of step pos (= *pos): anc[r][pos] = pos*R + r (the
 *   self-attention cache row this step writes for row r) and klen[r] = pos + 1.
 * avsr_beam_kv_put: cache_k[(pos*R + r)*D ..] = qkv[r][D..2D), cache_v from qkv[r][2D..3D).
 * avsr_beam_post: after avsr_beam_select of step pos: new running state per row (token,
 *   score, decoder / CTC score sums in double like the reference's Python floats, CTC prefix
 *   score), the back-pointers and ended-hypothesis records of the step, per-utterance end
 *   detection (e2e_asr_common.py:18-48 over the per-length best ended scores) and stop rules;
 *   src[0..R) = rows to gather the ancestry from, src[R..2R) = r_new rows for r_prev; *pos += 1.
 * Positions per row (a decode session, avsr_amd.decode.DecodeSession: a fixed number of utterance
 * slots, a finished utterance's slot refilled while the others keep stepping, so one replayed step
 * is step 0 of one slot and step 200 of another). upos[U] is the position of each slot and
 * rowpos[R] the same per row, rowpos[r] = upos[r / beam]:
 * avsr_beam_step_prep_rows / avsr_beam_kv_put_rows: the two kernels above with pos = rowpos[r].
 * avsr_beam_post with upos != NULL (`pos` unused): pos = upos[u] everywhere (history index
 *   pos*R + r, forced eos at maxlen[u] - 1, hypothesis length of end detection, best_len); a slot
 *   that was done before the step keeps its position, every other advances by one (also on the
 *   step that finishes it, so a done slot stands one past its last record); rowpos is rewritten.
 *   A done slot's history writes go to its frozen position: the history needs max(maxlen) + 1 rows.
 * avsr_beam_slot_reset: slot u back to the state of a fresh utterance (upos 0, done 0, tok sos,
 *   score 0 for its first row and -inf for the others, sdec = sctc = s_prev = 0, best_len row and
 *   best_end -inf, maxlen / tlen / klen_mem from the arguments, done[U] recounted); touches only
 *   that slot's rows. */
typedef struct {
  int U, beam, P, R, Lmax, steps_cap, eos, end_detect;
  double d_end;
  int* pos;
  const int* maxlen;
  const int* sel_prev; const int* sel_tok; const int* sel_col;
  const float* sel_score; const float* sel_dec; const float* sel_ctc; const float* sel_s;
  int* tok; float* score; double* sdec; double* sctc; float* s_prev;
  int* src;
  int* bp_prev; int* bp_tok; int* end_flag; float* end_score; double* end_dec; double* end_ctc;
  float* best_len;           /* [U][Lmax + 3] */
  float* best_end;           /* [U] */
  int* done;                 /* [U + 1]: per utterance, then the count */
  int* upos;                 /* [U] or NULL: per-slot positions (see above) */
  int* rowpos;               /* [R], with upos */
  /* hot-word biasing (sel_bonus NULL: off): the selected bonus is summed per hypothesis in double
   * like sdec / sctc (shw[R]) and recorded with an ended hypothesis (end_hw, same shape as
   * end_dec); node_out[r] = sel_next[r], the root for a row of a finished utterance: the other
   * buffer of the node ping-pong, which the next step's avsr_hotword_step reads. A hypothesis
   * ended by the step limit keeps the bonus of an unfinished phrase (its eos is not scored). */
  const float* sel_bonus; const int* sel_next;
  double* shw; double* end_hw; int* node_out;
  /* n-gram LM (sel_lm NULL: off) and length bonus (slen NULL: off), like the hot-word sums: the
   * selected unweighted LM score is summed per hypothesis in double (slm[R]) and recorded with an
   * ended hypothesis (end_lm); slen[R] / end_len count the scored tokens (the length bonus scorer
   * gives every token 1). lm_state_out[r] = sel_lm_next[r], lm_start for a row of a finished
   * utterance: the other buffer of the LM state ping-pong. lm_start must be set with sel_lm
   * (avsr_ngram_lm.start, the node of (sos)): a zeroed field means node 0, the EMPTY context, not
   * <s>. A hypothesis ended by the step limit
   * gets the reference's unscored eos: no LM term and no length term for it. */
  const float* sel_lm; const int* sel_lm_next;
  double* slm; double* end_lm; int* lm_state_out;
  double* slen; double* end_len;
  int lm_start;
} avsr_beam_post_params;
typedef struct {
  int U, beam, R, Lmax, slot, sos;
  int maxlen, tlen;          /* the new utterance's step limit and frames (>= 1) */
  int* upos; int* rowpos; int* done;
  int* tok; float* score; double* sdec; double* sctc; float* s_prev;
  float* best_len; float* best_end;
  int* maxlen_arr; int* tlen_arr; int* klen_mem;
} avsr_beam_slot_reset_params;
int avsr_beam_step_prep_rows(int R, int Lmax, const int* rowpos, int* anc, int* klen, void* stream);
int avsr_beam_kv_put_rows(int dtype, int R, int D, const void* qkv, int64_t ldqkv, void* cache_k, void* cache_v,
                          const int* rowpos, void* stream);
int avsr_beam_slot_reset(const avsr_beam_slot_reset_params* p, void* stream);
int avsr_beam_step_prep(int R, int Lmax, const int* pos, int* anc, int* klen, void* stream);
int avsr_beam_kv_put(int dtype, int R, int D, const void* qkv, int64_t ldqkv, void* cache_k, void* cache_v,
                     const int* pos, void* stream);
int avsr_beam_post(const avsr_beam_post_params* p, void* stream);

/* ------------------------------------------------------------------------------------
 * Input front end (the collator's per-clip CPU transforms moved on device).
 * avsr_fbank_stack: log mel filterbank features of 16 kHz waveforms, stacked 4 frames per
 *   video frame and layer-normalised per row, written in the model's audios layout.
 *   Replaces FBanksAndStack.forward src/dataset/avhubert_dataset.py:108-116 (logfbank of
 *   python_speech_features 0.6 at :111: preemphasis 0.97, 400-sample frames every 160,
 *   rectangular window, |rfft_512|^2 / 512, 26 triangular mel filters, eps floor, log;
 *   stacker :91-106; F.layer_norm over 104, eps 1e-5) + collate_pad's 0.0 row padding
 *   (:280-311) + the permute to (B, 104, T) (:351).
 *   wav [B][ldw] f32 (clip b uses n_samples[b] >= 1 samples, e.g. 640 * video frames after
 *   cut_or_pad :22-33); out [B][104][T] f32, rows >= ceil(frames_b / 4) are zero.
 *   bins: the 28 filter edges floor(513 * mel2hz(linspace(0, hz2mel(8000), 28)) / 16000).
 * avsr_video_normalize: uint8 frames [B][T][H][W] -> f32 [B][1][T][crop][crop] =
 *   ((x / 255) cropped at (oy, ox) - mean) / std.  Replaces VideoTransform
 *   (avhubert_dataset.py:225-246: /255, CenterCrop(88) or RandomCrop(88) offsets,
 *   Normalize(0.421, 0.165)) + the collator permute (:350).
 * ------------------------------------------------------------------------------------ */
typedef struct {
  int B, T;                  /* clips, output rows (>= the longest clip's rows) */
  const float* wav; int64_t ldw;
  const int64_t* n_samples;  /* device [B] */
  int bins[28];
  float preemph, ln_eps;
  float* out;
} avsr_fbank_params;
int avsr_fbank_stack(const avsr_fbank_params* p, void* stream);

typedef struct {
  int B, T, H, W, crop, oy, ox;
  const uint8_t* frames;
  float mean, std;
  float* out;
} avsr_video_norm_params;
int avsr_video_normalize(const avsr_video_norm_params* p, void* stream);

/* ------------------------------------------------------------------------------------
 * Train-time augmentation on device (the collator's CPU transforms).
 * avsr_time_mask: zero spans of rows of x [B][L][row_bytes] (any dtype: row_bytes bytes per
 *   time step): rows [spans[b][s][0], spans[b][s][1]) of clip b for s < nspan (empty / negative
 *   spans ignored). Replaces AdaptiveTimeMask.forward's `cloned[t_start:t_end] = 0`
 *   (src/dataset/avhubert_dataset.py:131-151; the span draws stay on the host, :141-149).
 * avsr_add_noise: y[b] = x[b] + s_b * n[b] over the first len_b samples of each clip, with
 *   s_b = 10^((snr0_b - snr_b) / 20), snr0_b = 10 (log10 |x_b|^2 - log10 |n_b|^2) (energies in
 *   fp64 over the clip) — torchaudio.functional.add_noise as AddNoise / AddMultiSpk call it
 *   (avhubert_dataset.py:154-222: :178, :214, :220). y may alias x. ws: 2 * B * 64 doubles.
 * avsr_rgb_to_gray: uint8 RGB [n][3] -> uint8 gray [n], cv2.COLOR_RGB2GRAY fixed point
 *   (R*4899 + G*9617 + B*1868 + 8192) >> 14 (load_video, avhubert_dataset.py:45).
 * ------------------------------------------------------------------------------------ */
typedef struct {
  int B, L, nspan;
  int64_t row_bytes, clip_stride_bytes;     /* bytes per time step, bytes between clips */
  void* x;
  const int* spans;                         /* device [B][nspan][2] */
} avsr_time_mask_params;
int avsr_time_mask(const avsr_time_mask_params* p, void* stream);

typedef struct {
  int B, L;
  const float* x; int64_t ldx;
  const float* noise; int64_t ldn;
  const int* lengths;                       /* device [B] or NULL (all L) */
  const float* snr_db;                      /* device [B] */
  float* y; int64_t ldy;
  double* ws;                               /* >= AVSR_NOISE_WS(B) doubles */
} avsr_add_noise_params;
#define AVSR_NOISE_WS(B) (2 * 64 * (int64_t)(B))
int avsr_add_noise(const avsr_add_noise_params* p, void* stream);

int avsr_rgb_to_gray(const uint8_t* rgb, uint8_t* gray, int64_t n, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* AVSR_HIP_H */
