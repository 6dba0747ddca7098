// CTC prefix beam search (include/avsr_hip.h avsr_ctc_beam): the first pass of two-pass
// decoding. One workgroup of 320 threads per utterance; thread e = i * (C + 1) + k owns one
// expansion of the frame: k = 0 is "prefix i stays" (blank, a repeated last token, and whatever
// extension of another beam entry spells the same string), k = 1 + j is "prefix i extended by
// candidate j". N * (C + 1) <= 272 expansions, so one per thread. The frame loop is sequential
// and latency-bound (two barriers per frame); the parallelism is over utterances.
//
// Per frame: every thread computes its expansion's (pb, pnb) from the previous beam alone — a
// pure function of LDS state, so no thread waits for another and nothing is accumulated through
// atomics: the stay thread of a prefix GATHERS the one extension that can spell it (the beam
// entry whose (length, hash) is its parent's, extended by its last token), and that extension's
// own thread stands down. The N best are then found by rank counting (a thread counts the
// expansions that beat it, ties by expansion index = creation order) and written to the other
// beam buffer at their rank, so the beam is always sorted and the result does not depend on
// lane timing. A kept extension gets tree node 1 + t * N + rank in the caller's workspace;
// a kept stay keeps its node, whose chain spells the same string. The frame's candidate tokens
// and log-probs are gathered into LDS a chunk of frames at a time (one exposed global latency
// per chunk instead of two dependent ones per frame).
#include <math.h>
#include "common.h"

namespace {

constexpr int CB_NT = 320;        // threads: >= 16 * 17 expansions
constexpr int CB_NMAX = 16, CB_CMAX = 16, CB_LCAP = 511;
constexpr int CB_SKIP = -2;       // a candidate that is not a CTC label here (never equals a last token)

AVSR_DEV float lae(float a, float b) {
  const float m = fmaxf(a, b);
  if (m == -INFINITY) return -INFINITY;
  return m + log1pf(expf(fminf(a, b) - m));
}

// hash of the string l + c from the hash of l (murmur3's 64-bit finaliser over a multiply-add)
AVSR_DEV unsigned long long hash_ext(unsigned long long h, int c) {
  unsigned long long x = h * 0x9E3779B97F4A7C15ull + (unsigned long long)(c + 1);
  x ^= x >> 33; x *= 0xFF51AFD7ED558CCDull;
  x ^= x >> 33; x *= 0xC4CEB9FE1A85EC53ull;
  return x ^ (x >> 33);
}

struct Beam {
  float pb[CB_NMAX], pnb[CB_NMAX], tot[CB_NMAX];
  int len[CB_NMAX], last[CB_NMAX], node[CB_NMAX];
  unsigned long long hash[CB_NMAX], phash[CB_NMAX];   // of the string, and of the string without its last token
};

__global__ __launch_bounds__(CB_NT) void ctc_beam_kernel(avsr_ctc_beam_params p) {
  const int u = blockIdx.x, tid = threadIdx.x;
  const int N = p.N, C = p.C, C1 = p.C + 1, Lcap = p.Lcap;
  const int T = min(max(p.tlen[u], 0), p.Tm);
  const int i = tid / C1, k = tid - i * C1;          // beam entry and expansion kind of this thread
  const float* LP = p.logp + (int64_t)u * p.Tm * p.ldp;
  const int* CAND = p.cand + (int64_t)u * p.Tm * C;
  const int nodes = p.Tm * N + 1;
  int2* tree = (int2*)p.ws + (int64_t)u * nodes;
  int* otok = p.tokens + (int64_t)u * N * Lcap;

  __shared__ Beam beam[2];
  __shared__ __attribute__((aligned(16))) float sc[CB_NT];   // score per expansion, NaN = no entry
  __shared__ int ctok[CB_NT];                                  // chunk: token per (frame, k), k = 0 blank
  __shared__ float clp[CB_NT];                                 //        its log-prob
  __shared__ int nb_s;

  if (tid == 0) {
    Beam& b = beam[0];
    b.pb[0] = 0.f; b.pnb[0] = -INFINITY; b.tot[0] = 0.f;
    b.len[0] = 0; b.last[0] = -1; b.node[0] = 0;
    b.hash[0] = 0x243F6A8885A308D3ull; b.phash[0] = 0;
    nb_s = T > 0 ? 1 : 0;
  }
  const int F = CB_NT / C1;          // frames per chunk (>= 18)
  const int EQ = (N * C1 + 3) >> 2;  // float4 groups of expansions
  int t0 = -F;
  __syncthreads();
  int nb = T > 0 ? 1 : 0;

  for (int t = 0; t < T; ++t) {
    if (t - t0 >= F) {               // gather the next chunk of frames (thread = (frame i, column k))
      t0 = t;
      if (i < F && t0 + i < T) {
        const int tt = t0 + i;
        int c = p.blank;
        if (k > 0) {
          c = CAND[(int64_t)tt * C + (k - 1)];
          if (c < 0 || c >= p.V || c == p.blank || c == p.eos) c = CB_SKIP;
        }
        ctok[tid] = c;
        clp[tid] = c >= 0 ? LP[(int64_t)tt * p.ldp + c] : -INFINITY;
      }
      __syncthreads();
    }
    const Beam& b = beam[t & 1];
    Beam& nx = beam[(t + 1) & 1];
    const int* ct = ctok + (t - t0) * C1 + 1;        // the frame's C candidates
    const float* cl = clp + (t - t0) * C1 + 1;       // (cl[-1] = blank's log-prob)
    // ---- this thread's expansion
    bool valid = false;
    float npb = -INFINITY, npnb = -INFINITY;
    int nlen = 0, nlast = -1, nnode = 0;
    unsigned long long nh = 0, nph = 0;
    if (i < nb) {
      const float pb = b.pb[i], pnb = b.pnb[i], tot = b.tot[i];
      const int len = b.len[i], last = b.last[i];
      const unsigned long long h = b.hash[i];
      if (k == 0) {                                  // the prefix stays
        valid = true;
        nlen = len; nlast = last; nnode = b.node[i]; nh = h; nph = b.phash[i];
        npb = tot + cl[-1];
        if (last >= 0) {
          for (int j = 0; j < C; ++j)
            if (ct[j] == last) npnb = lae(npnb, pnb + cl[j]);
          for (int i2 = 0; i2 < nb; ++i2) {          // the beam entry that is this string without its last token
            if (b.len[i2] != len - 1 || b.hash[i2] != nph) continue;
            const float base = b.last[i2] == last ? b.pb[i2] : b.tot[i2];
            for (int j = 0; j < C; ++j)
              if (ct[j] == last) npnb = lae(npnb, base + cl[j]);
          }
        }
      } else {                                       // the prefix extended by candidate k - 1
        const int j = k - 1, c = ct[j];
        bool ok = c >= 0 && len + 1 <= Lcap;
        for (int j2 = 0; ok && j2 < j; ++j2) ok = ct[j2] != c;       // a repeated candidate: its first column owns it
        if (ok) {
          nh = hash_ext(h, c);
          for (int i2 = 0; ok && i2 < nb; ++i2) ok = !(b.len[i2] == len + 1 && b.hash[i2] == nh);   // in the beam: its stay thread gathers this
        }
        if (ok) {
          valid = true;
          nlen = len + 1; nlast = c; nph = h; nnode = b.node[i];     // nnode: the parent's node for now
          const float base = c == last ? pb : tot;
          npnb = base + cl[j];
          for (int j2 = j + 1; j2 < C; ++j2)
            if (ct[j2] == c) npnb = lae(npnb, base + cl[j2]);
        }
      }
    }
    const float s = lae(npb, npnb);
    sc[tid] = valid ? s : __builtin_nanf("");
    const int nvalid = __syncthreads_count(valid);
    // ---- rank among the frame's entries; the N best become the beam, in rank order
    if (valid) {
      int rank = 0;
      for (int q = 0; q < EQ; ++q) {
        const f32x4 v = *(const f32x4*)(sc + 4 * q);
#pragma unroll
        for (int r = 0; r < 4; ++r) rank += (v[r] > s) || (v[r] == s && 4 * q + r < tid);
      }
      if (rank < N) {
        if (k > 0) {
          const int node = 1 + t * N + rank;         // < nodes
          tree[node] = make_int2(nnode, nlast);
          nnode = node;
        }
        nx.pb[rank] = npb; nx.pnb[rank] = npnb; nx.tot[rank] = s;
        nx.len[rank] = nlen; nx.last[rank] = nlast; nx.node[rank] = nnode;
        nx.hash[rank] = nh; nx.phash[rank] = nph;
      }
    }
    nb = min(nvalid, N);
    __syncthreads();
  }

  // ---- outputs: the final beam is sorted; fills first, then one lane per hypothesis walks its chain
  const Beam& b = beam[T & 1];
  for (int idx = tid; idx < N * Lcap; idx += CB_NT) {
    const int r = idx / Lcap, pos = idx - r * Lcap;
    if (r >= nb || pos >= b.len[r]) otok[idx] = -1;
  }
  if (tid < N) {
    const bool live = tid < nb;
    p.len[u * N + tid] = live ? b.len[tid] : 0;
    p.score[u * N + tid] = live ? b.tot[tid] : -INFINITY;
    if (live) {
      int node = b.node[tid];
      for (int pos = b.len[tid] - 1; pos >= 0 && node > 0 && node < nodes; --pos) {
        const int2 e = tree[node];
        otok[tid * Lcap + pos] = e.y;
        node = e.x;
      }
    }
  }
  if (tid == 0) p.n_out[u] = nb;
}

}  // namespace

extern "C" int avsr_ctc_beam(const avsr_ctc_beam_params* p, void* stream) {
  if (!p || p->U < 0 || p->Tm < 0 || p->V <= 0 || p->ldp < p->V || p->blank < 0 || p->blank >= p->V) return AVSR_E_ARG;
  if (p->N < 1 || p->N > CB_NMAX || p->C < 1 || p->C > CB_CMAX || p->Lcap < 0 || p->Lcap > CB_LCAP) return AVSR_E_SHAPE;
  if (p->U == 0) return 0;
  if (!p->tlen || !p->ws || !p->n_out || !p->len || !p->score || (p->Lcap > 0 && !p->tokens)) return AVSR_E_ARG;
  if (p->Tm > 0 && (!p->logp || !p->cand)) return AVSR_E_ARG;
  if ((uintptr_t)p->ws & 7) return AVSR_E_ALIGN;
  hipLaunchKernelGGL(ctc_beam_kernel, dim3(p->U), dim3(CB_NT), 0, (hipStream_t)stream, *p);
  AVSR_CHECK_LAUNCH();
  return 0;
}
