"""Two-pass decoding (avsr_amd/rescore.py) beside the joint beam search, in one process.

Same model, seed and inputs as bench.decode_throughput: the full-size model with random weights
(torch.manual_seed(0), odim 5049), fp32, 8 utterances of T = 25 / 100 / 375 frames drawn from
torch.Generator().manual_seed(5). Per length, decode_batch of the two-pass search at
(N, C) = (10, 10) and of get_beam_search_decoder at beams 1 / 3 / 5 (ctc_weight 0.1 everywhere)
are warmed up on the timed shapes, then timed alternately (--reps rounds, host clock around a call
that ends in a device synchronise); the JSON holds every round and the median. With random weights
the joint search runs to maxlen = T steps and the CTC n-best are about T tokens long, so both
modes do the most work an utterance of that length can ask of them.

Also the avsr_ctc_beam kernel alone at U = 8, T = 375, V = 5049, (N, C) = (10, 10) on
log_softmax(3 * randn): median of 50 launches timed one by one with events, and the mean of 200
back to back (tools/align_kbench.py's pattern).

python tools/rescore_bench.py [--reps 5] [--out profiles/rescore_bench.json]
python tools/rescore_bench.py --profile 25     (the two-pass decode alone, to run under a tracer)"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from avsr_amd import ops  # noqa: E402

TOKENS = ["<blank>"] + [f"u{i}" for i in range(1, 5048)] + ["<eos>"]
U, N, C = 8, 10, 10


def timed(fn, dev):
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize(dev)
    return time.perf_counter() - t0, out


def build_model(dev):
    from avsr_amd.avhubert_avsr_model import AVHubertAVSR
    from avsr_amd.configuration_avhubert_avsr import AVHubertAVSRConfig
    torch.manual_seed(0)
    model = AVHubertAVSR(AVHubertAVSRConfig(odim=5049)).eval()
    model.setup_engine(dev, torch.float32)
    return model


def two_pass_only(dev, T, calls):
    """--profile T: the two-pass decode_batch alone, `calls` times after one warm-up, for a
    kernel trace taken in a run of its own (rocprofv3 --kernel-trace --stats -- python ...)"""
    from avsr_amd.avhubert_avsr_model import get_rescoring_decoder
    model = build_model(dev)
    g = torch.Generator().manual_seed(5)
    xs = [(torch.randn(T, 1024, generator=g) * 0.5).to(dev) for _ in range(U)]
    s = get_rescoring_decoder(model.avsr, TOKENS, ctc_weight=0.1, beam_size=N, token_beam=C)
    s.decode_batch(xs)
    ts = [timed(lambda: s.decode_batch(xs), dev)[0] for _ in range(calls)]
    print(json.dumps({"profile_frames": T, "calls": calls + 1, "seconds": [round(t, 5) for t in ts]}), flush=True)


def decode_modes(dev, reps):
    from avsr_amd.avhubert_avsr_model import get_beam_search_decoder, get_rescoring_decoder
    model = build_model(dev)
    out = []
    for T in (25, 100, 375):
        g = torch.Generator().manual_seed(5)
        xs = [(torch.randn(T, 1024, generator=g) * 0.5).to(dev) for _ in range(U)]
        modes = {f"two_pass_N{N}_C{C}": get_rescoring_decoder(model.avsr, TOKENS, ctc_weight=0.1, beam_size=N, token_beam=C)}
        for beam in (1, 3, 5):
            modes[f"joint_beam{beam}"] = get_beam_search_decoder(model.avsr, TOKENS, ctc_weight=0.1, beam_size=beam)
        last = {}
        for name, s in modes.items():          # warm-up on the timed shapes
            s.decode_batch(xs[:2])
            last[name] = s.decode_batch(xs)
        torch.cuda.synchronize(dev)
        times = {name: [] for name in modes}
        for _ in range(reps):                  # alternating: one round times every mode once
            for name, s in modes.items():
                dt, last[name] = timed(lambda: s.decode_batch(xs), dev)
                times[name].append(dt)
        rec = {"frames_per_utt": T, "utterances": U, "dtype": "fp32", "ctc_weight": 0.1, "reps": reps, "modes": {}}
        for name, ts in times.items():
            lens = [len(nb[0].yseq) - 2 for nb in last[name] if nb]
            rec["modes"][name] = {"seconds": [round(t, 5) for t in ts], "median_s": round(statistics.median(ts), 5),
                                  "utt_per_s": round(U / statistics.median(ts), 2),
                                  "best_len_mean": round(sum(lens) / max(1, len(lens)), 1),
                                  "nbest_mean": round(sum(len(nb) for nb in last[name]) / U, 1)}
        out.append(rec)
        print(json.dumps(rec), flush=True)
    del model
    torch.cuda.empty_cache()
    return out


def kernel_alone(dev):
    T, V = 375, 5049
    logits = torch.zeros(U * T, 5056, device=dev)
    logits[:, :V] = (torch.randn(U * T, V, generator=torch.Generator().manual_seed(0)) * 3).to(dev)
    logp = torch.empty(U, T, V, device=dev)
    cand = torch.empty(U, T, C, device=dev, dtype=torch.int32)
    ops.log_softmax_topk(logits, V, logp.view(U * T, V), C, cand.view(U * T, C))
    tlen = torch.full((U,), T, dtype=torch.int32).to(dev)
    ws = torch.empty(ops.ctc_beam_ws(U, T, N) // 8, device=dev, dtype=torch.int64)

    def fn():
        return ops.ctc_beam(logp, tlen, cand, N, blank=0, eos=V - 1, ws=ws)

    for _ in range(10):
        res = fn()
    torch.cuda.synchronize(dev)
    one = []
    for _ in range(50):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize(dev)
        one.append(a.elapsed_time(b) * 1e3)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(200):
        fn()
    b.record()
    torch.cuda.synchronize(dev)
    rec = {"kernel": "avsr_ctc_beam", "U": U, "T": T, "V": V, "N": N, "C": C,
           "median_us": round(statistics.median(one), 1), "min_us": round(min(one), 1), "max_us": round(max(one), 1),
           "back_to_back_us": round(a.elapsed_time(b) * 1e3 / 200, 1),
           "us_per_frame": round(statistics.median(one) / T, 3), "best_len": int(res[2][0, 0])}
    print(json.dumps(rec), flush=True)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--kernel-only", action="store_true")
    ap.add_argument("--profile", type=int, default=0, metavar="T", help="only the two-pass decode at T frames, 4 calls")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("rescore_bench needs an MI355X: timings come from the device only")
    dev = torch.device("cuda:0")
    if args.profile:
        return two_pass_only(dev, args.profile, 3)
    result = {"tool": "rescore_bench", "kernel_alone": kernel_alone(dev)}
    if not args.kernel_only:
        result["decode"] = decode_modes(dev, args.reps)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
