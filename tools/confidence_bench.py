"""What token confidences cost next to the search that produced the hypotheses: for 8 utterances
of 1 / 4 / 15 s (25 / 100 / 375 frames), in one process,
  decode       decoder.decode_batch at beam 5 (the joint search, ctc_weight 0.1)
  confidence   confidence_batch over the top hypothesis of every utterance (ctc_weight 0.1, 3
               alternatives): CTC head, ONE avsr_ctc_neighbors launch, row top-k, one
               teacher-forced decoder pass per utterance, one host read
  confidence_short   the same over the first max(1, T // 9) tokens of each hypothesis
timed as --reps interleaved rounds (decode, confidence, confidence_short): host clock around a
call that ends in a device synchronise; medians reported, every round kept. kernel_ms is
avsr_ctc_neighbors alone (its three launches, with lz) on the same logits and labels, device
events, median of 5.

Same model as bench.decode_throughput and tools/hotword_bench.py: full size, random weights
(torch.manual_seed(0), odim 5049), fp32. That model never emits eos, so every search runs to
maxlen = T and its hypotheses have ONE TOKEN PER FRAME (L = T; those with an adjacent repeat
have no CTC path and come back None): L * V * T recurrence steps grow with T^2 there, nine times
the L ~ T / 9 of speech at 25 frames / s, which `confidence_short` stands for.

python tools/confidence_bench.py [--reps 3] [--out profiles/confidence_bench.json]"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from avsr_amd import confidence, ops, rescore  # noqa: E402
from avsr_amd.align import strip_sos_eos  # noqa: E402
from avsr_amd.avhubert_avsr_model import AVHubertAVSR, get_beam_search_decoder  # noqa: E402
from avsr_amd.configuration_avhubert_avsr import AVHubertAVSRConfig  # noqa: E402

TOKENS = ["<blank>"] + [f"u{i}" for i in range(1, 5048)] + ["<eos>"]
UTTS, BEAM, W, ALTS = 8, 5, 0.1, 3
FRAMES = {"1s": 25, "4s": 100, "15s": 375}


def timed(dev, fn):
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize(dev)
    return time.perf_counter() - t0, out


def kernel_ms(e2e, xs, ys):
    """avsr_ctc_neighbors alone on the logits and labels confidence_batch gives it"""
    eng = e2e.engine()
    dev = eng.device
    _, cl, Ts, Tm = rescore.ctc_logits(eng, xs)
    Lmax = max(1, max(len(y) for y in ys))
    lab = torch.full((len(ys), Lmax), -1, dtype=torch.int32)
    for u, y in enumerate(ys):
        lab[u, :len(y)] = torch.tensor(y, dtype=torch.int32)
    lab, llen, ilen = lab.to(dev), torch.tensor([len(y) for y in ys], dtype=torch.int32).to(dev), \
        torch.tensor(Ts, dtype=torch.int32).to(dev)
    lse = ops.row_lse(cl, eng.V, torch.empty(len(xs) * Tm, device=dev, dtype=torch.float32))
    B = len(xs)
    bufs = dict(sub=torch.empty(B, Lmax, eng.Vp, device=dev), dele=torch.empty(B, Lmax, device=dev),
                base=torch.empty(B, device=dev), feasible=torch.empty(B, device=dev, dtype=torch.int32),
                lz=torch.empty(B, Lmax, device=dev),
                ws=torch.empty(ops.ctc_neighbors_ws(B, Tm, Lmax), device=dev, dtype=torch.uint8))
    ms = []
    for i in range(6):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        ops.ctc_neighbors(cl, B, Tm, eng.V, lab, llen, ilen, lse, blank=e2e.blank, eos=e2e.eos, **bufs)
        b.record()
        b.synchronize()
        if i:
            ms.append(a.elapsed_time(b))
    return statistics.median(ms), Lmax


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default="profiles/confidence_bench.json")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("confidence_bench needs an MI355X: timings come from the device only")
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    model = AVHubertAVSR(AVHubertAVSRConfig(odim=5049)).eval()
    model.setup_engine(dev, torch.float32)
    e2e = model.avsr
    bs = get_beam_search_decoder(e2e, TOKENS, ctc_weight=W, beam_size=BEAM)
    rec = {"tool": "confidence_bench", "utterances": UTTS, "beam": BEAM, "dtype": "fp32", "ctc_weight": W,
           "alternatives": ALTS, "reps": args.reps, "lengths": {}}
    for name, T in FRAMES.items():
        g = torch.Generator().manual_seed(5)
        xs = [(torch.randn(T, 1024, generator=g) * 0.5).to(dev) for _ in range(UTTS)]
        top = [strip_sos_eos(nbest[0].yseq.tolist(), e2e.sos, e2e.eos) for nbest in bs.decode_batch(xs)]   # warm-up too
        short = [y[:max(1, T // 9)] for y in top]
        runs = {"decode": lambda: bs.decode_batch(xs),
                "confidence": lambda: confidence.confidence_batch(e2e, xs, top, ctc_weight=W, alternatives=ALTS),
                "confidence_short": lambda: confidence.confidence_batch(e2e, xs, short, ctc_weight=W, alternatives=ALTS)}
        scored = {k: sum(c is not None for c in runs[k]()) for k in ("confidence", "confidence_short")}   # warm-up
        times = {k: [] for k in runs}
        for _ in range(args.reps):
            for k, fn in runs.items():
                times[k].append(timed(dev, fn)[0])
        med = {k: statistics.median(ts) for k, ts in times.items()}
        r = {"frames": T, "configs": {k: {"seconds": [round(t, 5) for t in ts], "median_s": round(med[k], 5)}
                                      for k, ts in times.items()}}
        for k, ys in (("confidence", top), ("confidence_short", short)):
            ms, Lmax = kernel_ms(e2e, xs, ys)
            r["configs"][k].update(tokens_max=Lmax, utterances_scored=scored[k], kernel_ms=round(ms, 4),
                                   over_decode=round(med[k] / med["decode"], 4))
        rec["lengths"][name] = r
    print(json.dumps(rec), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(rec, f, indent=1)


if __name__ == "__main__":
    main()
