"""Streaming decode session (decode.DecodeSession, continuous batching) beside decode_batch over
consecutive groups of 8, in one process.

Same model as bench.decode_throughput: full size, random weights (torch.manual_seed(0), odim 5049),
fp32, ctc_weight 0.1, so every search runs to maxlen = T steps. Three workloads:
  mixed    64 utterances, T uniform in [25, 375] from torch.Generator().manual_seed(5) in draw order, beam 5
  uniform  16 x 375 frames, beam 5
  short    64 x 25 frames, beam 1
A side: decode_batch over consecutive groups of 8 (each call builds its state and captures its
graphs; a group steps until its longest utterance is done: sum over groups of max T replays, known
before running). B side: one session of 8 slots per pass over the workload, what
decode_stream(xs, slots=8, max_frames=max T) runs, its step count read from the session. Both
sides are warmed up on the workload, then timed in interleaved pairs (batch, stream) x --reps
(host clock around a pass that ends in a device synchronise); medians reported, every round kept.

python tools/decode_stream_bench.py [--reps 3] [--out profiles/decode_stream_bench.json] [--only mixed]"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from avsr_amd import stream_slots  # noqa: E402

TOKENS = ["<blank>"] + [f"u{i}" for i in range(1, 5048)] + ["<eos>"]
GROUP = SLOTS = 8


def workloads():
    g = torch.Generator().manual_seed(5)
    mixed = [int(t) for t in torch.randint(25, 376, (64,), generator=g)]
    return {"mixed": (mixed, 5), "uniform": ([375] * 16, 5), "short": ([25] * 64, 1)}


def timed(fn, dev):
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize(dev)
    return time.perf_counter() - t0, out


def plain(results):
    return [[h.asdict() for h in nbest] for nbest in results]


def run_workload(model, dev, name, Ts, beam, reps):
    from avsr_amd.avhubert_avsr_model import get_beam_search_decoder
    bs = get_beam_search_decoder(model.avsr, TOKENS, ctc_weight=0.1, beam_size=beam)
    g = torch.Generator().manual_seed(5)
    xs = [(torch.randn(T, 1024, generator=g) * 0.5).to(dev) for T in Ts]
    n = len(xs)
    batch_replays = sum(max(Ts[s:s + GROUP]) for s in range(0, n, GROUP))
    stream_replays = []

    def batch():
        out = []
        for s in range(0, n, GROUP):
            out += bs.decode_batch(xs[s:s + GROUP])
        return out

    def stream():
        with bs.stream(slots=SLOTS, max_frames=max(Ts)) as session:
            out = stream_slots.in_input_order(session.run(xs), n)
            stream_replays.append(session.replays)
        return out

    batch()
    stream()
    tb, ts, equal = [], [], True
    for _ in range(reps):
        dt, a = timed(batch, dev)
        tb.append(dt)
        dt, b = timed(stream, dev)
        ts.append(dt)
        equal = equal and plain(a) == plain(b)
    mb, ms = statistics.median(tb), statistics.median(ts)
    rec = {"workload": name, "utterances": n, "beam": beam, "frames_min": min(Ts), "frames_max": max(Ts),
           "frames_sum": sum(Ts), "dtype": "fp32", "ctc_weight": 0.1, "reps": reps,
           "batch": {"call": f"decode_batch over groups of {GROUP}", "seconds": [round(t, 4) for t in tb],
                     "median_s": round(mb, 4), "utt_per_s": round(n / mb, 2), "step_replays": batch_replays},
           "stream": {"call": f"decode_stream(slots={SLOTS}, max_frames={max(Ts)})", "seconds": [round(t, 4) for t in ts],
                      "median_s": round(ms, 4), "utt_per_s": round(n / ms, 2), "step_replays": stream_replays[-1]},
           "stream_over_batch_utt_per_s": round(mb / ms, 3),
           "stream_over_batch_step_replays": round(stream_replays[-1] / batch_replays, 3),
           "all_results_equal": equal}
    print(json.dumps(rec), flush=True)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default="profiles/decode_stream_bench.json")
    ap.add_argument("--only", default=None, choices=list(workloads()))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("decode_stream_bench needs an MI355X: timings come from the device only")
    dev = torch.device("cuda:0")
    from avsr_amd.avhubert_avsr_model import AVHubertAVSR
    from avsr_amd.configuration_avhubert_avsr import AVHubertAVSRConfig
    torch.manual_seed(0)
    model = AVHubertAVSR(AVHubertAVSRConfig(odim=5049)).eval()
    model.setup_engine(dev, torch.float32)
    result = {"tool": "decode_stream_bench", "workloads": []}
    for name, (Ts, beam) in workloads().items():
        if args.only in (None, name):
            result["workloads"].append(run_workload(model, dev, name, Ts, beam, args.reps))
    mixed = [w for w in result["workloads"] if w["workload"] == "mixed"]
    if mixed and not mixed[0]["stream"]["step_replays"] < mixed[0]["batch"]["step_replays"]:
        raise SystemExit("mixed workload: the stream must take fewer step replays than the batches")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
