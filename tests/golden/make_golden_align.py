"""Golden vectors for CTC forced alignment, produced by running the REFERENCE (quanpn90/avsr,
read-only at /root/reference) on CPU, fp32, in this container. Never run on the GPU box; only the
.npz output is committed: tests/golden/avsr_align.npz

CTC.forced_align_batch(hs_pad (T, B, V) logits, ys_pad, ilens) (src/nets/backend/ctc.py:246-328)
on ctc_lo(hs) of the tiny recipe (oracle/weights.py TINY_CONFIG, gen_tensor weights, seed 0,
dropouts 0, eval). Hidden states: the reference's own encoder outputs stored in avsr_tiny.N.npz
(dec_enc_0 / dec_enc_1, T = 25 / 19), padded into one batch.
  batch 1: the labels of oracle.weights.make_inputs on the full utterances
  batch 2: rows cut to T = 7 / 6 / 12 / 19 with (9, 9, 9, 9) (tight, repeats), (1..6) (tight, no
           blank), (7, 7, 7, 3, 3) and (11,)
Stored per batch k: hs{k} (B, T, D), ys_pad{k} (B, L) padded with -1, ilens{k}, ali{k} (B, T) int64
(the returned arrays, padded with -1 beyond ilens) and score{k} (B,) fp64, each path's
log-probability under the fp64 log-softmax of the logits.

Asserted before writing: a plain fp32 and a plain fp64 Viterbi (tests/align_ref.py) of the same
log-probs give the stored paths, and 8 draws of N(0, 1e-3) noise on the log-probs leave every
path unchanged (100 x the 1e-5 the fp32 log-softmax test allows, tests/test_gpu_decode.py:72: the
engine's fp32 logits cannot flip a decision).
Printed for the record, not stored: what the reference's single-utterance CTC.forced_align
(ctc.py:181-244) returns where there is slack — its s - 1 = -1 wrap-around.

usage: PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_align.py   (a few seconds)
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, "/root/reference")
sys.dont_write_bytecode = True
if not hasattr(np, "bool"):          # ctc.py:290 uses the alias numpy 1.24 removed
    np.bool = bool

from oracle.weights import NO_DROPOUT, TINY_CONFIG, gen_tensor, make_inputs  # noqa: E402
from tests.align_ref import viterbi  # noqa: E402
from tests.golden.parts import load_parts  # noqa: E402

CUTS2 = ((0, 7, (9, 9, 9, 9)), (1, 6, (1, 2, 3, 4, 5, 6)), (0, 12, (7, 7, 7, 3, 3)), (1, 19, (11,)))
NOISE, DRAWS = 1e-3, 8


def _pad_labels(labels):
    out = np.full((len(labels), max(len(l) for l in labels)), -1, dtype=np.int64)
    for b, l in enumerate(labels):
        out[b, :len(l)] = l
    return out


def main():
    torch.manual_seed(0)
    torch.set_num_threads(8)
    from src.avhubert_avsr.avhubert_avsr_model import AVHubertAVSR
    from src.avhubert_avsr.configuration_avhubert_avsr import AVHubertAVSRConfig

    model = AVHubertAVSR(AVHubertAVSRConfig(**TINY_CONFIG, **NO_DROPOUT))
    sd = model.state_dict()
    model.load_state_dict({k: torch.from_numpy(gen_tensor(k, v.shape, seed=0)) for k, v in sd.items()}, strict=True)
    model.eval()
    ctc = model.avsr.ctc
    g = load_parts("avsr_tiny")
    enc = [g["dec_enc_0"], g["dec_enc_1"]]
    assert enc[0].shape[0] == 25 and enc[1].shape[0] >= 19
    labels1 = make_inputs()[3]
    batches = [[(enc[0][:25], labels1[0]), (enc[1][:19], labels1[1])],
               [(enc[c][:T], y) for c, T, y in CUTS2]]
    rng = np.random.Generator(np.random.PCG64(7))
    out = {}
    for k, batch in enumerate(batches, start=1):
        B, T = len(batch), max(len(h) for h, _ in batch)
        hs = np.zeros((B, T, enc[0].shape[1]), dtype=np.float32)
        for b, (h, _) in enumerate(batch):
            hs[b, :len(h)] = h
        ilens = np.array([len(h) for h, _ in batch], dtype=np.int64)
        ys_pad = _pad_labels([y for _, y in batch])
        with torch.no_grad():
            logits = ctc.ctc_lo(torch.from_numpy(hs))                      # (B, T, V)
            alis = ctc.forced_align_batch(logits.transpose(0, 1), torch.from_numpy(ys_pad), torch.from_numpy(ilens))
        lp32 = torch.log_softmax(logits, -1).numpy()
        lp64 = torch.log_softmax(logits.double(), -1).numpy()
        ali = np.full((B, T), -1, dtype=np.int64)
        score = np.zeros(B, dtype=np.float64)
        zero = np.zeros(T, dtype=np.float32)
        for b, (h, y) in enumerate(batch):
            Tb = int(ilens[b])
            a = np.asarray(alis[b])
            assert a.shape == (Tb,) and a.dtype == np.int64, (a.shape, a.dtype)
            a32, _, f32 = viterbi(lp32[b], zero, y, Tb, dtype=np.float32)
            a64, s64, f64 = viterbi(lp64[b], zero, y, Tb, dtype=np.float64)
            assert f32 and f64 and np.array_equal(a32, a) and np.array_equal(a64, a), (k, b)
            for _ in range(DRAWS):
                noisy = lp64[b] + rng.normal(0.0, NOISE, size=lp64[b].shape)
                an, _, fn = viterbi(noisy, zero, y, Tb, dtype=np.float64)
                assert fn and np.array_equal(an, a), (k, b, "a path flips under noise: choose other rows or labels")
            ali[b, :Tb] = a
            score[b] = lp64[b][np.arange(Tb), a].sum()
            assert abs(score[b] - float(s64)) < 1e-9
            print(f"batch {k} utt {b}: T = {Tb}, y = {tuple(y)}, score {score[b]:.6f}\n  forced_align_batch: {a.tolist()}")
            with torch.no_grad():
                single = ctc.forced_align(torch.from_numpy(hs[b:b + 1, :Tb]), np.array(y, dtype=np.int64))
            single = [int(t) for t in single]
            print(f"  forced_align (single, not stored): {single}" + ("" if single == a.tolist() else "   <- wrap-around"))
        out.update({f"hs{k}": hs, f"ys_pad{k}": ys_pad, f"ilens{k}": ilens, f"ali{k}": ali, f"score{k}": score})
    path = os.path.join(HERE, "avsr_align.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
