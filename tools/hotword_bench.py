"""What hot-word biasing costs in decode throughput: decode_batch of 8 utterances of 4 s (100
frames) at beam 5, in one process, three configurations timed in interleaved rounds:
  parent    the package of the parent commit (--parent DIR: a checkout of it with its library
            built, loaded beside this one under the name avsr_amd_parent); left out without --parent
  no_list   this tree, no phrase list: launches exactly what the parent launches
  hotwords  this tree, 100 random 3-token phrases (torch.Generator().manual_seed(7)), bonus 1.0

Same model as bench.decode_throughput and tools/decode_stream_bench.py: full size, random weights
(torch.manual_seed(0), odim 5049), fp32, ctc_weight 0.1, so every search runs to maxlen = T steps.
Each configuration is warmed up, then timed --reps times in rounds (parent, no_list, hotwords): host
clock around a call that ends in a device synchronise; medians reported, every round kept.

python tools/hotword_bench.py [--parent DIR] [--reps 3] [--out profiles/hotword_bench.json]"""
import argparse
import importlib.util
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

TOKENS = ["<blank>"] + [f"u{i}" for i in range(1, 5048)] + ["<eos>"]
UTTS, FRAMES, BEAM, PHRASES, BONUS = 8, 100, 5, 100, 1.0


def load_package(root, name):
    """the avsr_amd package under `root` as module `name` (its imports are all relative, its
    library is the one beside it)"""
    pkg = os.path.join(root, "avsr_amd")
    spec = importlib.util.spec_from_file_location(name, os.path.join(pkg, "__init__.py"), submodule_search_locations=[pkg])
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return name


def searcher(pkg, dev):
    m = importlib.import_module(pkg + ".avhubert_avsr_model")
    cfg = importlib.import_module(pkg + ".configuration_avhubert_avsr")
    torch.manual_seed(0)
    model = m.AVHubertAVSR(cfg.AVHubertAVSRConfig(odim=5049)).eval()
    model.setup_engine(dev, torch.float32)
    return model, m.get_beam_search_decoder(model.avsr, TOKENS, ctc_weight=0.1, beam_size=BEAM)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", default=None)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default="profiles/hotword_bench.json")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("hotword_bench needs an MI355X: timings come from the device only")
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(5)
    xs = [(torch.randn(FRAMES, 1024, generator=g) * 0.5).to(dev) for _ in range(UTTS)]
    g = torch.Generator().manual_seed(7)
    phrases = (torch.randint(1, len(TOKENS) - 1, (PHRASES, 3), generator=g)).tolist()
    keep = []                                   # the models stay alive with their searches
    runs = {}
    if args.parent:
        model, bs = searcher(load_package(args.parent, "avsr_amd_parent"), dev)
        keep.append(model)
        runs["parent"] = bs
    model, runs["no_list"] = searcher("avsr_amd", dev)
    model2, runs["hotwords"] = searcher("avsr_amd", dev)
    runs["hotwords"].set_hotwords(phrases, BONUS)
    keep += [model, model2]
    times, results = {k: [] for k in runs}, {}
    for k, bs in runs.items():
        bs.decode_batch(xs)                     # warm-up
    for _ in range(args.reps):
        for k, bs in runs.items():
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            out = bs.decode_batch(xs)
            torch.cuda.synchronize(dev)
            times[k].append(time.perf_counter() - t0)
            results[k] = [[h.asdict() for h in nbest] for nbest in out]
    rec = {"tool": "hotword_bench", "utterances": UTTS, "frames_per_utt": FRAMES, "beam": BEAM, "dtype": "fp32",
           "ctc_weight": 0.1, "reps": args.reps, "phrases": PHRASES, "phrase_tokens": 3, "bonus": BONUS, "configs": {}}
    for k, ts in times.items():
        med = statistics.median(ts)
        rec["configs"][k] = {"seconds": [round(t, 4) for t in ts], "median_s": round(med, 4),
                             "utt_per_s": round(UTTS / med, 2)}
    med = {k: statistics.median(ts) for k, ts in times.items()}
    if "parent" in med:
        rec["no_list_over_parent_utt_per_s"] = round(med["parent"] / med["no_list"], 4)
        rec["no_list_results_equal_parent"] = results["no_list"] == results["parent"]
    rec["hotwords_over_no_list_utt_per_s"] = round(med["no_list"] / med["hotwords"], 4)
    rec["hotword_nonzero_scores"] = sum(h["scores"]["hotword"] != 0.0 for nbest in results["hotwords"] for h in nbest)
    print(json.dumps(rec), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(rec, f, indent=1)


if __name__ == "__main__":
    main()
