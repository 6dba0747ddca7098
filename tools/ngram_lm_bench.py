"""What n-gram LM shallow fusion costs in decode throughput, in one process, medians of --reps
interleaved pairs (the manner of tools/decode_stream_bench.py and tools/hotword_bench.py):
  joint     decode_batch of 8 utterances of 100 frames (4 s, the C4 length) at beam 5:
            no_lm (launches what the parent launches) against lm (an order-4 table of about 1e6
            seeded entries, lm_weight 0.3, length_bonus 0.5)
  rescore   the two-pass decoder at 10 hypotheses over the same utterances: no_lm against lm
Also the host time to compile the table (NgramLM.from_table's numpy part, from arrays) and to
upload it. Same model as bench.decode_throughput: full size, random weights (torch.manual_seed(0),
odim 5049), fp32, ctc_weight 0.1, so every joint search runs to maxlen = T steps. The table is
random (numpy RandomState(9)): 5048 unigrams, then per level contexts drawn from the
entries of the level below, so every n-gram's prefix is listed. Random-weight searches do not follow
the table, so the figure is the cost of carrying the LM (one more launch per step, mostly backed
off to the unigram level), not of a model that likes its n-grams.

python tools/ngram_lm_bench.py [--reps 3] [--entries 1000000] [--out profiles/ngram_lm_bench.json]"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from avsr_amd.avhubert_avsr_model import AVHubertAVSR, get_beam_search_decoder, get_rescoring_decoder  # noqa: E402
from avsr_amd.configuration_avhubert_avsr import AVHubertAVSRConfig  # noqa: E402
from avsr_amd.ngram_lm import NgramLM  # noqa: E402

TOKENS = ["<blank>"] + [f"u{i}" for i in range(1, 5048)] + ["<eos>"]
V = len(TOKENS)
EOS = V - 1
UTTS, FRAMES, BEAM, NBEST, ORDER, W_LM, W_LEN = 8, 100, 5, 10, 4, 0.3, 0.5


def random_grams(entries, seed=9):
    """{k: (tokens [n, k], logp, backoff)} of about `entries` n-grams: the unigrams, then a third of
    the rest per level, each level's n-grams extending n-grams of the level below by a random token"""
    rng = np.random.RandomState(seed)
    uni = np.arange(1, V, dtype=np.int64).reshape(-1, 1)           # tokens 1 .. V-2 and eos
    grams = {1: (uni, rng.uniform(-9.0, -6.0, len(uni)), rng.uniform(-1.0, -0.1, len(uni)))}
    prev = np.concatenate([uni[:-1], [[EOS]]])                      # contexts: a token, or <s> (the shared id)
    per_level = (entries - len(uni)) // (ORDER - 1)
    for k in range(2, ORDER + 1):
        ctx = prev[rng.randint(0, len(prev), per_level)]
        ctx = ctx[~np.any(ctx[:, 1:] == EOS, axis=1)] if k > 2 else ctx      # </s> only ever comes last
        t = np.unique(np.concatenate([ctx, rng.randint(1, V, (len(ctx), 1))], axis=1), axis=0)
        grams[k] = (t, rng.uniform(-4.0, -0.5, len(t)), rng.uniform(-1.0, -0.1, len(t)) if k < ORDER else np.zeros(len(t)))
        prev = t[t[:, -1] != EOS]
    return grams


def timed(fn, dev):
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize(dev)
    return time.perf_counter() - t0, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--entries", type=int, default=1000000)
    ap.add_argument("--out", default="profiles/ngram_lm_bench.json")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("ngram_lm_bench needs an MI355X: timings come from the device only")
    dev = torch.device("cuda:0")
    grams = random_grams(args.entries)
    t0 = time.perf_counter()
    lm = NgramLM(ORDER, grams, EOS, EOS, V, -10.0)
    compile_s = time.perf_counter() - t0
    g = torch.Generator().manual_seed(5)
    xs = [(torch.randn(FRAMES, 1024, generator=g) * 0.5).to(dev) for _ in range(UTTS)]
    torch.manual_seed(0)
    model = AVHubertAVSR(AVHubertAVSRConfig(odim=V)).eval()
    model.setup_engine(dev, torch.float32)
    runs = {
        "joint_no_lm": get_beam_search_decoder(model.avsr, TOKENS, 0.1, BEAM),
        "joint_lm": get_beam_search_decoder(model.avsr, TOKENS, 0.1, BEAM, lm=lm, lm_weight=W_LM, length_bonus=W_LEN),
        "rescore_no_lm": get_rescoring_decoder(model.avsr, TOKENS, 0.1, NBEST),
        "rescore_lm": get_rescoring_decoder(model.avsr, TOKENS, 0.1, NBEST, lm=lm, lm_weight=W_LM, length_bonus=W_LEN),
    }
    upload_s, _ = timed(lambda: runs["joint_lm"]._lm_dev.get(lm, dev), dev)
    times, results = {k: [] for k in runs}, {}
    for k, bs in runs.items():
        bs.decode_batch(xs)                     # warm-up
    for _ in range(args.reps):
        for k, bs in runs.items():
            t, out = timed(lambda: bs.decode_batch(xs), dev)
            times[k].append(t)
            results[k] = out
    rec = {"tool": "ngram_lm_bench", "utterances": UTTS, "frames_per_utt": FRAMES, "beam": BEAM, "rescore_nbest": NBEST,
           "dtype": "fp32", "ctc_weight": 0.1, "reps": args.reps, "lm_order": ORDER, "lm_weight": W_LM,
           "length_bonus": W_LEN, "lm_entries": int(sum(len(t) for t, _, _ in grams.values())), "lm_nodes": lm.nodes,
           "lm_compile_s": round(compile_s, 3), "lm_upload_s": round(upload_s, 4), "configs": {}}
    med = {k: statistics.median(ts) for k, ts in times.items()}
    for k, ts in times.items():
        rec["configs"][k] = {"seconds": [round(t, 4) for t in ts], "median_s": round(med[k], 4),
                             "utt_per_s": round(UTTS / med[k], 2)}
    rec["joint_lm_over_no_lm_utt_per_s"] = round(med["joint_no_lm"] / med["joint_lm"], 4)
    rec["rescore_lm_over_no_lm_utt_per_s"] = round(med["rescore_no_lm"] / med["rescore_lm"], 4)
    lms = [float(h.scores["lm"]) for nbest in results["joint_lm"] for h in nbest]
    rec["joint_lm_hyps"], rec["joint_lm_mean_lm_score"] = len(lms), round(sum(lms) / max(1, len(lms)), 3)
    print(json.dumps(rec), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(rec, f, indent=1)


if __name__ == "__main__":
    main()
