"""What keyword spotting costs next to the CTC prefix beam search on the same log-probs: for 8
utterances of 1 / 4 / 15 s (25 / 100 / 375 frames) and 16 / 256 / 4096 keywords of 1 to 8 tokens
(drawn with a fixed seed), in one process,
  kws_ms          avsr_ctc_kws alone (score / start / end), one launch for all keywords x utterances
  kws_trace_ms    the same with the trace / tstart outputs
  ctc_beam_ms     avsr_ctc_beam (N = 10, 10 candidates per frame) on the same logp, per length
each the median of 5 launches timed one by one with device events after a warm-up launch, and
  spot_batch_s    ONE wall-clock call of kws.spot_batch (CTC head per utterance, log-softmax +
                  argmax, the launch, the host read and the host loop over U x K results), host
                  clock around a call that ends in a device synchronise, after one warm-up call.

Same model as tools/confidence_bench.py: full size, random weights (torch.manual_seed(0), odim
5049), fp32. Random keywords on random posteriors: the timings do not depend on the values, and
nothing here says anything about detection accuracy.

python tools/kws_bench.py [--out profiles/kws_bench.json]"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from avsr_amd import kws, ops, rescore  # noqa: E402
from avsr_amd.avhubert_avsr_model import AVHubertAVSR  # noqa: E402
from avsr_amd.configuration_avhubert_avsr import AVHubertAVSRConfig  # noqa: E402

UTTS, BEAM, REPS = 8, 10, 5
FRAMES = {"1s": 25, "4s": 100, "15s": 375}
KEYWORDS = (16, 256, 4096)


def event_ms(fn):
    """median of REPS device-event timings of fn(), after one warm-up call"""
    ms = []
    for i in range(REPS + 1):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        if i:
            ms.append(a.elapsed_time(b))
    return statistics.median(ms), ms


def draw_keywords(K, V, eos, seed):
    rng = np.random.Generator(np.random.PCG64(seed))
    return [rng.integers(1, eos, size=int(rng.integers(1, 9))).tolist() for _ in range(K)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/kws_bench.json")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("kws_bench needs an MI355X: timings come from the device only")
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    model = AVHubertAVSR(AVHubertAVSRConfig(odim=5049)).eval()
    model.setup_engine(dev, torch.float32)
    e2e = model.avsr
    eng = e2e.engine()
    V = eng.V
    rec = {"tool": "kws_bench", "utterances": UTTS, "dtype": "fp32", "keyword_tokens": "1..8", "reps": REPS,
           "ctc_beam": {"N": BEAM, "C": BEAM}, "lengths": {}}
    for name, T in FRAMES.items():
        g = torch.Generator().manual_seed(5)
        xs = [(torch.randn(T, 1024, generator=g) * 0.5).to(dev) for _ in range(UTTS)]
        _, cl, Ts, Tm = rescore.ctc_logits(eng, xs)
        logp = torch.empty(UTTS, Tm, V, device=dev, dtype=torch.float32)
        cand = torch.empty(UTTS, Tm, BEAM, device=dev, dtype=torch.int32)
        ops.log_softmax_topk(cl, V, logp.view(UTTS * Tm, V), BEAM, cand.view(UTTS * Tm, BEAM))
        top = cand[:, :, 0].contiguous()
        tlen = torch.tensor(Ts, dtype=torch.int32).to(dev)
        ws = torch.empty(ops.ctc_beam_ws(UTTS, Tm, BEAM) // 8, device=dev, dtype=torch.int64)
        beam_ms, beam_all = event_ms(lambda: ops.ctc_beam(logp, tlen, cand, BEAM, blank=e2e.blank, eos=e2e.eos, ws=ws))
        r = {"frames": T, "ctc_beam_ms": round(beam_ms, 4), "ctc_beam_all_ms": [round(m, 4) for m in beam_all],
             "keywords": {}}
        for K in KEYWORDS:
            kw = draw_keywords(K, V, e2e.eos, seed=K)
            Lmax = max(len(y) for y in kw)
            lab = torch.full((K, Lmax), -1, dtype=torch.int32)
            for k, y in enumerate(kw):
                lab[k, :len(y)] = torch.tensor(y, dtype=torch.int32)
            lab, llen = lab.to(dev), torch.tensor([len(y) for y in kw], dtype=torch.int32).to(dev)
            out = dict(score=torch.empty(UTTS, K, device=dev), start=torch.empty(UTTS, K, device=dev, dtype=torch.int32),
                       end=torch.empty(UTTS, K, device=dev, dtype=torch.int32))
            tr = dict(trace_out=torch.empty(UTTS, K, Tm, device=dev),
                      tstart_out=torch.empty(UTTS, K, Tm, device=dev, dtype=torch.int32))
            ms, ms_all = event_ms(lambda: ops.ctc_kws(logp, tlen, top, lab, llen, blank=e2e.blank, **out))
            ms_t, ms_t_all = event_ms(lambda: ops.ctc_kws(logp, tlen, top, lab, llen, blank=e2e.blank, **out, **tr))
            del tr
            kws.spot_batch(e2e, xs, kw)                                   # warm-up
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            hits = kws.spot_batch(e2e, xs, kw)
            torch.cuda.synchronize(dev)
            wall = time.perf_counter() - t0
            r["keywords"][str(K)] = {
                "kws_ms": round(ms, 4), "kws_all_ms": [round(m, 4) for m in ms_all],
                "kws_trace_ms": round(ms_t, 4), "kws_trace_all_ms": [round(m, 4) for m in ms_t_all],
                "pairs": UTTS * K, "ns_per_pair_frame": round(ms * 1e6 / (UTTS * K * T), 3),
                "kws_over_ctc_beam": round(ms / beam_ms, 4), "spot_batch_s": round(wall, 5),
                "hits": sum(len(h) for h in hits)}
        rec["lengths"][name] = r
    print(json.dumps(rec), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(rec, f, indent=1)


if __name__ == "__main__":
    main()
