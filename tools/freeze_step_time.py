"""Step time of the C2 train step with parameters frozen (requires_grad=False): bench.py's own loop
(16 x 15 s clips, bf16, FusedAdamW with the engine's overlap settings, gradient clear on the side
stream, no host syncs inside a block) for the all-trainable video-on step and the freeze sets
R (the video ResNet) and E (the whole encoder), alternating block by block in one process so that
clocks and allocator state are shared. Every variant is warmed up before anything is timed and
again for a few steps after each switch; a block is timed like bench.py's run: device-synchronised
wall time over its steps.

usage: python tools/freeze_step_time.py [--steps 10] [--rounds 3] [--warmup 3] [--out FILE]
writes profiles/freeze_step_times.json (or FILE) and prints it."""
import argparse
import gc
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from avsr_amd import engine as E  # noqa: E402
from avsr_amd.avhubert_avsr_model import AVHubertAVSR  # noqa: E402
from avsr_amd.configuration_avhubert_avsr import AVHubertAVSRConfig  # noqa: E402
from avsr_amd.optim import FusedAdamW  # noqa: E402
from bench import synthetic_batch  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SETS = {"all": [], "R": ["encoder.feature_extractor_video.resnet"], "E": ["encoder"]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10, help="timed steps per block")
    ap.add_argument("--rounds", type=int, default=3, help="blocks per variant")
    ap.add_argument("--warmup", type=int, default=3, help="untimed steps after each switch")
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--seq", type=int, default=375)
    ap.add_argument("--labels", type=int, default=40)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "freeze_step_times.json"))
    args = ap.parse_args()

    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    E.prioritize_step_stream(dev)
    torch.manual_seed(0)
    cfg = AVHubertAVSRConfig(odim=5049)
    model = AVHubertAVSR(cfg).train()
    model.setup_engine(dev, torch.bfloat16)
    eng = model.avsr.engine()
    arena = eng.arena
    opt = FusedAdamW(arena, lr=1e-4, weight_decay=0.005, max_grad_norm=1.0, overlap=E.OPT_OVERLAP)
    opt.overlap_blocks = E.OPT_OVERLAP_BLOCKS
    opt.clear_in_update = E.OPT_CLEAR_IN_UPDATE
    if E.EARLY_NORM:
        eng.pre_video_grads = opt.early_sumsq
    v, a, lens, lab = synthetic_batch(args.batch, args.seq, args.labels)
    v, a = v.to(dev), a.to(dev)
    d_ctc = torch.full((1,), cfg.mtlalpha, device=dev)
    d_att = torch.full((1,), 1.0 - cfg.mtlalpha, device=dev)
    eng.force_modality = (None,)                # the video-on step, as bench.py --force-modality none
    gc.collect()
    gc.freeze()
    seed = [1]

    def select(name):
        model.requires_grad_(True)
        for sub in SETS[name]:
            model.avsr.get_submodule(sub).requires_grad_(False)

    def step():
        eng.zero_grad_async()
        seed[0] += 1
        _, ctx = eng.forward(v, a, lens, lab, train=True, need_grad=True, seed=seed[0])
        eng.backward(ctx, d_ctc, d_att)
        opt.step()

    arena.zero_grad()
    for name in SETS:                           # every variant's allocation pattern before any timing
        select(name)
        for _ in range(max(2, args.warmup)):
            step()
    torch.cuda.synchronize()
    blocks = {name: [] for name in SETS}
    for _ in range(args.rounds):
        for name in SETS:
            select(name)
            for _ in range(args.warmup):
                step()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                step()
            torch.cuda.synchronize()
            blocks[name].append((time.perf_counter() - t0) * 1e3 / args.steps)
    opt.sync()
    torch.cuda.synchronize()
    frames = args.batch * args.seq
    res = {"tool": "tools/freeze_step_time.py", "device": torch.cuda.get_device_name(dev),
           "workload": f"C2: {args.batch} x {args.seq} frames, L={args.labels}, bf16, video on, "
                       "FusedAdamW(overlap) + clip, bench.py's loop",
           "steps_per_block": args.steps, "rounds": args.rounds, "warmup_after_switch": args.warmup,
           "variants": {name: {"frozen": SETS[name], "ms_per_step_blocks": [round(x, 3) for x in ms],
                               "ms_per_step": round(statistics.median(ms), 3),
                               "frames_per_s": round(frames / (statistics.median(ms) * 1e-3), 1)}
                        for name, ms in blocks.items()}}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
