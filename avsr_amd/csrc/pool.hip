// The stem's BN + PReLU + 3x3 stride-2 max-pool (forward, and the dense part of its backward)
// and the global average pool of the ResNet frontend (declarations and reference call sites in
// include/avsr_hip.h). HBM-bound: 16-byte vector loads/stores over NHWC channel vectors.
#include "norm.h"

namespace {

// =============================================================== stem max-pool
// grid (vector blocks of one image, image): 32-bit in-image indexing, the nine window
// loads issued together (clamped addresses, masked values)
template <typename T>
__global__ __launch_bounds__(256) void stem_pool_fwd_kernel(avsr_stem_pool_params p, FastDiv fwo) {
  constexpr int VE = VecW<T>::VE;
  const int cpv = p.C / VE;
  const int per_img = p.Ho * p.Wo * cpv;
  const int v = blockIdx.x * 256 + threadIdx.x;
  if (v >= per_img) return;
  const int n = blockIdx.y;
  const int cv = v % cpv, c0 = cv * VE;
  const uint32_t opix = (uint32_t)(v / cpv);
  const int oh = (int)fdiv(opix, fwo), ow = (int)(opix - oh * fwo.d);
  float sc[VE], sh[VE], pw[VE];
  chan_load(p.scale, c0, sc); chan_load(p.shift, c0, sh); chan_load(p.prelu, c0, pw);
  const T* base = (const T*)p.h + (int64_t)n * p.H * p.W * p.C + c0;
  float hv[9][VE];
#pragma unroll
  for (int q = 0; q < 9; ++q) {
    const int ih = min(max(2 * oh - 1 + q / 3, 0), p.H - 1), iw = min(max(2 * ow - 1 + q % 3, 0), p.W - 1);
    ldv(base + (ih * p.W + iw) * p.C, hv[q]);
  }
  float best[VE], bh[VE];
  uint8_t idx[VE];
#pragma unroll
  for (int j = 0; j < VE; ++j) { best[j] = -INFINITY; bh[j] = 0.f; idx[j] = 0; }
#pragma unroll
  for (int q = 0; q < 9; ++q) {
    const int ih = 2 * oh - 1 + q / 3, iw = 2 * ow - 1 + q % 3;
    if (ih < 0 || ih >= p.H || iw < 0 || iw >= p.W) continue;
#pragma unroll
    for (int j = 0; j < VE; ++j) {
      const float z = hv[q][j] * sc[j] + sh[j];
      const float y = z > 0.f ? z : z * pw[j];
      if (y > best[j]) { best[j] = y; bh[j] = hv[q][j]; idx[j] = (uint8_t)q; }
    }
  }
  const int64_t ov = (int64_t)n * per_img + v;
  stv((T*)p.y + ov * VE, best);
  if (p.hmax) stv((T*)p.hmax + ov * VE, bh);
  if constexpr (VE == 8) *(uint2*)(p.argmax + ov * VE) = *(const uint2*)idx;
  else *(uint32_t*)(p.argmax + ov * VE) = *(const uint32_t*)idx;
}

// Same outputs for H = 2*Ho, W = 2*Wo: one thread per 2x2 block of pooled outputs and channel
// group. The block's four 3x3 windows cover a 5x5 input patch: each input is loaded and put
// through BN+PReLU once (25 per 4 outputs instead of 36), row by row; every window still
// visits its taps in row-major order with the strict '>' (same maximum, same argmax on ties).
// Grid-stride with the channel group fixed (per-channel coefficients loaded once).
template <typename T>
__global__ __launch_bounds__(256) void stem_pool_fwd2_kernel(avsr_stem_pool_params p, FastDiv fbwo, FastDiv fbho) {
  constexpr int VE = VecW<T>::VE;
  const int cpv = p.C / VE, cshift = 31 - __builtin_clz(cpv);
  const int bho = p.Ho >> 1, bwo = p.Wo >> 1;
  // 32-bit indices with multiply-shift divisions (the launcher checks nv < 2^31)
  const uint32_t nv = (uint32_t)p.nimg * bho * bwo * cpv, stride = gridDim.x * 256u;
  const uint32_t t0 = blockIdx.x * 256u + threadIdx.x;
  const int cv = (int)(t0 & (cpv - 1)), c0 = cv * VE;
  float sc[VE], sh[VE], pw[VE];
  chan_load(p.scale, c0, sc); chan_load(p.shift, c0, sh); chan_load(p.prelu, c0, pw);
  for (uint32_t v = t0; v < nv; v += stride) {
    const uint32_t blk = v >> cshift, q = fdiv(blk, fbwo);
    const int bw = (int)(blk - q * fbwo.d);
    const uint32_t nq = fdiv(q, fbho);
    const int bh = (int)(q - nq * fbho.d);
    const int64_t n = nq;
    const int ih0 = 4 * bh - 1, iw0 = 4 * bw - 1;        // patch origin (may be -1)
    const T* base = (const T*)p.h + n * p.H * p.W * p.C + c0;
    float best[4][VE], bhv[4][VE];
    uint8_t idx[4][VE];
#pragma unroll
    for (int o = 0; o < 4; ++o)
#pragma unroll
      for (int j = 0; j < VE; ++j) { best[o][j] = -INFINITY; bhv[o][j] = 0.f; idx[o][j] = 0; }
#pragma unroll
    for (int r = 0; r < 5; ++r) {
      const int ih = ih0 + r;
      const bool rok = ih >= 0 && ih < p.H;
      float hv[5][VE];
#pragma unroll
      for (int c = 0; c < 5; ++c) {
        const int iw = min(max(iw0 + c, 0), p.W - 1);
        ldv(base + ((int64_t)min(max(ih, 0), p.H - 1) * p.W + iw) * p.C, hv[c]);
      }
      if (!rok) continue;
#pragma unroll
      for (int c = 0; c < 5; ++c) {
        const int iw = iw0 + c;
        if (iw < 0 || iw >= p.W) continue;
#pragma unroll
        for (int o = 0; o < 4; ++o) {
          const int a = o >> 1, b = o & 1;
          const int wr = r - 2 * a, wc = c - 2 * b;       // tap position in window o
          if (wr < 0 || wr > 2 || wc < 0 || wc > 2) continue;
#pragma unroll
          for (int j = 0; j < VE; ++j) {
            const float z = hv[c][j] * sc[j] + sh[j];
            const float y = z > 0.f ? z : z * pw[j];
            if (y > best[o][j]) { best[o][j] = y; bhv[o][j] = hv[c][j]; idx[o][j] = (uint8_t)(wr * 3 + wc); }
          }
        }
      }
    }
#pragma unroll
    for (int o = 0; o < 4; ++o) {
      const int oh = 2 * bh + (o >> 1), ow = 2 * bw + (o & 1);
      const int64_t ov = ((n * p.Ho + oh) * p.Wo + ow) * cpv + cv;
      stv((T*)p.y + ov * VE, best[o]);
      if (p.hmax) stv((T*)p.hmax + ov * VE, bhv[o]);
      if constexpr (VE == 8) *(uint2*)(p.argmax + ov * VE) = *(const uint2*)idx[o];
      else *(uint32_t*)(p.argmax + ov * VE) = *(const uint32_t*)idx[o];
    }
  }
}

// Stem backward, dense part. The BN reductions run over the pooled grid (h at the argmax,
// saved by the forward as hmax; dz is nonzero only where an input pixel is some window's
// argmax, so sum_p dz*xhat = sum_o dzp[o]*xhat(hmax[o])); here dz[p] = sum of dzp[o] over the
// (at most 4) windows o whose argmax is p, and dh = scale*(dz - S0/M - xhat*S1/M).
// Grid-stride over 16-byte vectors with the thread's channel group fixed (the stride is a
// multiple of C/VE), so the per-channel coefficients are formed once per thread.
template <typename T>
__global__ __launch_bounds__(256) void stem_bwd_apply_kernel(avsr_stem_pool_params p, FastDiv fw, FastDiv fhw) {
  constexpr int VE = VecW<T>::VE;
  const int cpv = p.C / VE, cshift = 31 - __builtin_clz(cpv);
  const int64_t nv = (int64_t)p.nimg * p.H * p.W * cpv, stride = (int64_t)gridDim.x * 256;
  const int64_t t0 = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int cv = (int)(t0 % cpv), c0 = cv * VE;
  const float invM = 1.f / (p.m_total > 0 ? (float)p.m_total : (float)p.nimg * p.H * p.W);
  float ka[VE], kb[VE], kc[VE], km[VE];
#pragma unroll
  for (int j = 0; j < VE; ++j) {
    const int c = c0 + j;
    const float s0 = p.sums[c * 3 + 0] * invM, s1 = p.sums[c * 3 + 1] * invM;
    ka[j] = p.scale[c]; kb[j] = -p.scale[c] * s1 * p.invstd[c]; kc[j] = -p.scale[c] * s0; km[j] = p.mean[c];
  }
  // two vectors per iteration: both h loads and all window gathers in flight together
  for (int64_t v = t0; v < nv; v += 2 * stride) {
    const bool two = v + stride < nv;
    float h[2][VE], d[2][VE];
#pragma unroll
    for (int u = 0; u < 2; ++u) {
#pragma unroll
      for (int j = 0; j < VE; ++j) d[u][j] = 0.f;
      if (u == 1 && !two) break;
      const int64_t w = v + u * stride;
      const uint32_t pix = (uint32_t)(w >> cshift);
      const uint32_t n = fdiv(pix, fhw), rem = pix - n * fhw.d;
      const int ih = (int)fdiv(rem, fw), iw = (int)(rem - ih * fw.d);
      ldv((const T*)p.h + w * VE, h[u]);
      // windows (oh, ow) with 2*o-1 <= i <= 2*o+1
      const int oh0 = (ih + 1) / 2 - 1, ow0 = (iw + 1) / 2 - 1;
#pragma unroll
      for (int dh = 0; dh < 2; ++dh) {
        const int oh = oh0 + dh;
        if (oh < 0 || oh >= p.Ho || ih < 2 * oh - 1 || ih > 2 * oh + 1) continue;
#pragma unroll
        for (int dw = 0; dw < 2; ++dw) {
          const int ow = ow0 + dw;
          if (ow < 0 || ow >= p.Wo || iw < 2 * ow - 1 || iw > 2 * ow + 1) continue;
          const int64_t ov = (((int64_t)n * p.Ho + oh) * p.Wo + ow) * cpv + cv;
          const uint8_t want = (uint8_t)((ih - 2 * oh + 1) * 3 + (iw - 2 * ow + 1));
          float g[VE];
          ldv((const T*)p.dz + ov * VE, g);
          uint8_t am[VE];
          if constexpr (VE == 8) *(uint2*)am = *(const uint2*)(p.argmax + ov * VE);
          else *(uint32_t*)am = *(const uint32_t*)(p.argmax + ov * VE);
#pragma unroll
          for (int j = 0; j < VE; ++j) d[u][j] += am[j] == want ? g[j] : 0.f;
        }
      }
    }
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      if (u == 1 && !two) break;
      float o[VE];
#pragma unroll
      for (int j = 0; j < VE; ++j) o[j] = ka[j] * d[u][j] + kb[j] * (h[u][j] - km[j]) + kc[j];
      stv((T*)p.dh + (v + u * stride) * VE, o);
    }
  }
}

// Same result for even H, W (Ho = H/2, Wo = W/2), one thread per 2x2 pixel block (2oh+dy, 2ow+dx)
// and channel group: the block's pixels lie in windows (oh, ow), (oh, ow+1) [dx = 1],
// (oh+1, ow) [dy = 1], (oh+1, ow+1) [both], so the four windows' dz / argmax are loaded once
// for four outputs (2.25 window gathers per pixel otherwise), with no per-pixel divisions and
// every load of the block issued together. Windows are added in the per-pixel kernel's order
// (bit-identical).
template <typename T>
__global__ __launch_bounds__(256) void stem_bwd_apply2_kernel(avsr_stem_pool_params p, FastDiv fwo, FastDiv fho) {
  constexpr int VE = VecW<T>::VE;
  const int cpv = p.C / VE, cshift = 31 - __builtin_clz(cpv);
  // 32-bit indices with multiply-shift divisions (the launcher checks nv < 2^31; the int64
  // divisions they replace were ~1/3 of this HBM-bound pass, 900 -> 737 us at C2). U blocks per
  // iteration with every load issued first (U = 2 needs 198 VGPRs: 2 waves per SIMD instead of 3)
  constexpr int U = 1;
  const uint32_t nv = (uint32_t)p.nimg * p.Ho * p.Wo * cpv, stride = gridDim.x * 256u;
  const uint32_t t0 = blockIdx.x * 256u + threadIdx.x;
  const int cv = (int)(t0 & (cpv - 1)), c0 = cv * VE;
  const float invM = 1.f / (p.m_total > 0 ? (float)p.m_total : (float)p.nimg * p.H * p.W);
  float ka[VE], kb[VE], kc[VE], km[VE];
#pragma unroll
  for (int j = 0; j < VE; ++j) {
    const int c = c0 + j;
    const float s0 = p.sums[c * 3 + 0] * invM, s1 = p.sums[c * 3 + 1] * invM;
    ka[j] = p.scale[c]; kb[j] = -p.scale[c] * s1 * p.invstd[c]; kc[j] = -p.scale[c] * s0; km[j] = p.mean[c];
  }
  for (uint32_t v0 = t0; v0 < nv; v0 += U * stride) {
    float g[U][4][VE], h[U][4][VE];
    uint8_t am[U][4][VE];
    bool wok[U][4], ok[U];
    uint32_t hb[U];                                    // vector index of pixel (2oh, 2ow)
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const uint32_t v = v0 + u * stride;
      ok[u] = v < nv;
      const uint32_t blk = (ok[u] ? v : v0) >> cshift;   // (n, oh, ow)
      const uint32_t q = fdiv(blk, fwo), n = fdiv(q, fho);
      const int ow = (int)(blk - q * fwo.d), oh = (int)(q - n * fho.d);
      // windows w = (oh + a, ow + b), a, b in {0, 1}; out-of-range windows contribute nothing
#pragma unroll
      for (int w = 0; w < 4; ++w) {
        const int wa = w >> 1, wb = w & 1;
        wok[u][w] = oh + wa < p.Ho && ow + wb < p.Wo;
        const uint32_t ov = ((n * p.Ho + min(oh + wa, p.Ho - 1)) * p.Wo + min(ow + wb, p.Wo - 1)) * cpv + cv;
        ldv((const T*)p.dz + (int64_t)ov * VE, g[u][w]);
        if constexpr (VE == 8) *(uint2*)am[u][w] = *(const uint2*)(p.argmax + (int64_t)ov * VE);
        else *(uint32_t*)am[u][w] = *(const uint32_t*)(p.argmax + (int64_t)ov * VE);
      }
      hb[u] = ((n * p.H + 2 * oh) * p.W + 2 * ow) * cpv + cv;
#pragma unroll
      for (int qd = 0; qd < 4; ++qd)
        ldv((const T*)p.h + (int64_t)(hb[u] + ((qd >> 1) * p.W + (qd & 1)) * cpv) * VE, h[u][qd]);
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      if (!ok[u]) break;
#pragma unroll
      for (int qd = 0; qd < 4; ++qd) {
        const int dy = qd >> 1, dx = qd & 1;
        float d[VE];
#pragma unroll
        for (int j = 0; j < VE; ++j) d[j] = 0.f;
        // pixel (2oh+dy, 2ow+dx) sits at window-local position (dy+1, dx+1) of window (oh, ow)
        // and at (dy-1, dx+1), (dy+1, dx-1), (dy-1, dx-1) of the others (rows: 3 per window)
#pragma unroll
        for (int w = 0; w < 4; ++w) {
          const int wa = w >> 1, wb = w & 1;
          if ((wa && !dy) || (wb && !dx)) continue;      // the pixel is not in that window
          const uint8_t want = (uint8_t)((dy - 2 * wa + 1) * 3 + (dx - 2 * wb + 1));
#pragma unroll
          for (int j = 0; j < VE; ++j) d[j] += (wok[u][w] && am[u][w][j] == want) ? g[u][w][j] : 0.f;
        }
        float o[VE];
#pragma unroll
        for (int j = 0; j < VE; ++j) o[j] = ka[j] * d[j] + kb[j] * (h[u][qd][j] - km[j]) + kc[j];
        stv((T*)p.dh + (int64_t)(hb[u] + (dy * p.W + dx) * cpv) * VE, o);
      }
    }
  }
}

// =============================================================== avg pool
template <typename T>
__global__ __launch_bounds__(256) void avgpool_fwd_kernel(int nimg, int P, int C, const T* x, T* y) {
  constexpr int VE = VecW<T>::VE;
  const int cpv = C / VE;
  const int64_t nv = (int64_t)nimg * cpv;
  for (int64_t v = blockIdx.x * 256 + threadIdx.x; v < nv; v += (int64_t)gridDim.x * 256) {
    const int64_t n = v / cpv;
    const int c0 = (int)(v % cpv) * VE;
    float s[VE], t[VE];
#pragma unroll
    for (int j = 0; j < VE; ++j) s[j] = 0.f;
    for (int q = 0; q < P; ++q) {
      ldv(x + ((n * P + q) * C + c0), t);
#pragma unroll
      for (int j = 0; j < VE; ++j) s[j] += t[j];
    }
#pragma unroll
    for (int j = 0; j < VE; ++j) s[j] /= (float)P;
    stv(y + v * VE, s);
  }
}

template <typename T>
__global__ __launch_bounds__(256) void avgpool_bwd_kernel(int nimg, int P, int C, const T* dy, T* dx) {
  constexpr int VE = VecW<T>::VE;
  const int cpv = C / VE;
  const int64_t nv = (int64_t)nimg * P * cpv;
  for (int64_t v = blockIdx.x * 256 + threadIdx.x; v < nv; v += (int64_t)gridDim.x * 256) {
    const int64_t n = v / ((int64_t)P * cpv);
    const int c0 = (int)(v % cpv) * VE;
    float t[VE];
    ldv(dy + (n * C + c0), t);
#pragma unroll
    for (int j = 0; j < VE; ++j) t[j] /= (float)P;
    stv(dx + v * VE, t);
  }
}

}  // namespace

extern "C" int avsr_stem_pool_fwd(const avsr_stem_pool_params* p, void* stream) {
  if (!p) return AVSR_E_ARG;
  return avsr_by_dtype(p->dtype, [&](auto t) -> int {
    using T = decltype(t);
    constexpr int VE = VecW<T>::VE;
    hipStream_t st = (hipStream_t)stream;
    if (p->C % VE) return AVSR_E_SHAPE;
    if (p->nimg > 65535) return AVSR_E_SHAPE;
    if (p->H == 2 * p->Ho && p->W == 2 * p->Wo && !(p->Ho & 1) && !(p->Wo & 1) && avsr_opt(AVSR_OPT_STEM_POOL_2X2) &&
        256 % (p->C / VE) == 0) {
      const int64_t nv2 = (int64_t)p->nimg * (p->Ho / 2) * (p->Wo / 2) * p->C / VE;
      if (nv2 >= (1ll << 31)) return AVSR_E_SHAPE;
      hipLaunchKernelGGL(stem_pool_fwd2_kernel<T>, dim3(bn_grid(nv2)), dim3(256), 0, st, *p, make_fastdiv(p->Wo / 2),
                         make_fastdiv(p->Ho / 2));
    } else {
      const dim3 g((p->Ho * p->Wo * p->C / VE + 255) / 256, p->nimg);
      hipLaunchKernelGGL(stem_pool_fwd_kernel<T>, g, dim3(256), 0, st, *p, make_fastdiv(p->Wo));
    }
    AVSR_CHECK_LAUNCH();
    return 0;
  });
}

extern "C" int avsr_stem_pool_bwd_apply(const avsr_stem_pool_params* p, void* stream) {
  if (!p) return AVSR_E_ARG;
  return avsr_by_dtype(p->dtype, [&](auto t) -> int {
    using T = decltype(t);
    constexpr int VE = VecW<T>::VE;
    hipStream_t st = (hipStream_t)stream;
    if (!p->dz || !p->dh || !p->sums || !p->argmax) return AVSR_E_ARG;
    if (p->C % VE) return AVSR_E_SHAPE;
    if (256 % (p->C / VE)) return AVSR_E_SHAPE;
    if ((int64_t)p->nimg * p->H * p->W >= (1ll << 31)) return AVSR_E_SHAPE;
    if (p->Ho != (p->H + 1) / 2 || p->Wo != (p->W + 1) / 2) return AVSR_E_SHAPE;
    const int64_t nv = (int64_t)p->nimg * p->H * p->W * p->C / VE;
    if (!(p->H & 1) && !(p->W & 1) && avsr_opt(AVSR_OPT_STEM_POOL_2X2)) {     // 2x2-block kernel (same result)
      const int64_t nv2 = (int64_t)p->nimg * p->Ho * p->Wo * p->C / VE;
      if (nv2 >= (1ll << 31) || nv >= (1ll << 31)) return AVSR_E_SHAPE;
      hipLaunchKernelGGL(stem_bwd_apply2_kernel<T>, dim3(bn_grid(nv2)), dim3(256), 0, st, *p, make_fastdiv(p->Wo),
                         make_fastdiv(p->Ho));
    } else {
      hipLaunchKernelGGL(stem_bwd_apply_kernel<T>, dim3(bn_grid(nv)), dim3(256), 0, st, *p, make_fastdiv(p->W),
                         make_fastdiv(p->H * p->W));
    }
    AVSR_CHECK_LAUNCH();
    return 0;
  });
}

extern "C" int avsr_avgpool_fwd(int dtype, int nimg, int P, int C, const void* x, void* y, void* stream) {
  return avsr_by_dtype(dtype, [&](auto t) -> int {
    using T = decltype(t);
    constexpr int VE = VecW<T>::VE;
    if (C % VE) return AVSR_E_SHAPE;
    const int g = avsr_grid((int64_t)nimg * C / VE);
    hipLaunchKernelGGL(avgpool_fwd_kernel<T>, dim3(g), dim3(256), 0, (hipStream_t)stream, nimg, P, C, (const T*)x, (T*)y);
    AVSR_CHECK_LAUNCH();
    return 0;
  });
}

extern "C" int avsr_avgpool_bwd(int dtype, int nimg, int P, int C, const void* dy, void* dx, void* stream) {
  return avsr_by_dtype(dtype, [&](auto t) -> int {
    using T = decltype(t);
    constexpr int VE = VecW<T>::VE;
    if (C % VE) return AVSR_E_SHAPE;
    const int g = avsr_grid((int64_t)nimg * P * C / VE);
    hipLaunchKernelGGL(avgpool_bwd_kernel<T>, dim3(g), dim3(256), 0, (hipStream_t)stream, nimg, P, C, (const T*)dy, (T*)dx);
    AVSR_CHECK_LAUNCH();
    return 0;
  });
}
