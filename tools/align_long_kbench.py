"""the long-form CTC alignment kernel in isolation: (1) one recording of T = 30000
frames (20 min), L = 5000 labels, V = 5049 logits (ldx 5056), fp32 and bf16, through
avsr_ctc_align_long: median of 5 launches timed one by one with events after warm-up; (2) the shape
of tools/align_kbench.py (B = 8, T = 375, L ~ 60) through avsr_ctc_align and avsr_ctc_align_long in
the same process: median of 50 launches each; (3) the shape of (1) through avsr_ctc_align_gaps with
filler = row maximum - lse and gap_penalty = -1, once with the flags at both ends and once with all
flags set, timed as (1), as a ratio to avsr_ctc_align_long in the same process; it asserts that
gap_penalty = -inf reproduces ctc_align_long's ali and score. Writes (1) and (2) to
profiles/align_long_kbench.txt and everything to profiles/align_gaps_kbench.txt; --parent FILE
appends the lines of FILE (this tool's output on the parent commit, same box and session) to the
latter under "parent commit:".
python tools/align_long_kbench.py [--parent FILE]"""
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from avsr_amd import ops  # noqa: E402

dev = torch.device("cuda")
V, Vp = 5049, 5056
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def timed(fn, warm, reps):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) * 1e3)
    return out


def setup(B, T, lens, dtype, seed):
    rng = np.random.Generator(np.random.PCG64(seed))
    lab = torch.full((B, max(lens)), -1, dtype=torch.int32)
    for b, n in enumerate(lens):
        lab[b, :n] = torch.from_numpy(rng.integers(1, V - 1, size=n).astype(np.int32))
    x = torch.empty(B * T, Vp, device=dev, dtype=dtype)
    g = torch.Generator(device=dev).manual_seed(seed)
    for r in range(0, B * T, 3000):             # in pieces: no second full-size fp32 buffer
        x[r:r + 3000] = (torch.randn(min(3000, B * T - r), Vp, generator=g, device=dev) * 3).to(dtype)
    lse = torch.empty(B * T, device=dev)
    ops.row_lse(x, V, lse)
    return dict(x=x, lse=lse, lab=lab.to(dev), llen=torch.tensor(lens, dtype=torch.int32).to(dev),
                ilen=torch.full((B,), T, dtype=torch.int32).to(dev), ali=torch.empty(B, T, dtype=torch.int32, device=dev),
                score=torch.empty(B, device=dev), feas=torch.empty(B, dtype=torch.int32, device=dev))


def run(op, ws, s, B, T):
    op(s["x"], B, T, V, s["lab"], s["llen"], s["ilen"], s["lse"], ali=s["ali"], score=s["score"], feasible=s["feas"],
       ws=ws)


# (1) a 20-minute recording
B, T, Lr = 1, 30000, 5000
ws = torch.empty(ops.ctc_align_long_ws(B, T, Lr), dtype=torch.uint8, device=dev)
for dtype in (torch.float32, torch.bfloat16):
    s = setup(B, T, [Lr], dtype, 0)
    one = timed(lambda: run(ops.ctc_align_long, ws, s, B, T), 1, 5)
    assert s["feas"].tolist() == [1]
    med = statistics.median(one)
    say(f"ctc_align_long {str(dtype)[6:]} B=1 T={T} L={Lr} V={V}: median {med / 1e3:.2f} ms = {med / T:.3f} us/frame "
        f"(min {min(one) / 1e3:.2f}, max {max(one) / 1e3:.2f} ms, 5 launches), workspace {ws.numel() / 1e6:.0f} MB")
    del s
del ws

# (2) the clip shape of tools/align_kbench.py through both kernels
B, T = 8, 375
LENS = [60, 55, 64, 58, 61, 52, 63, 60]
ws_old = torch.empty(ops.ctc_align_ws(B, T, max(LENS)), dtype=torch.uint8, device=dev)
ws_new = torch.empty(ops.ctc_align_long_ws(B, T, max(LENS)), dtype=torch.uint8, device=dev)
for dtype in (torch.float32, torch.bfloat16):
    s = setup(B, T, LENS, dtype, 0)
    old = timed(lambda: run(ops.ctc_align, ws_old, s, B, T), 20, 50)
    ali_old, score_old = s["ali"].clone(), s["score"].clone()
    new = timed(lambda: run(ops.ctc_align_long, ws_new, s, B, T), 20, 50)
    assert s["feas"].tolist() == [1] * B and torch.equal(s["ali"], ali_old) and torch.equal(s["score"], score_old)
    mo, mn = statistics.median(old), statistics.median(new)
    say(f"{str(dtype)[6:]} B={B} T={T} L~60 V={V}: ctc_align median {mo:.1f} us (min {min(old):.1f}), "
        f"ctc_align_long median {mn:.1f} us (min {min(new):.1f}), long / old = {mn / mo:.2f}")

n_long = len(lines)

# (3) the recording of (1) with gap states
B, T, Lr = 1, 30000, 5000
ws = torch.empty(ops.ctc_align_long_ws(B, T, Lr), dtype=torch.uint8, device=dev)
for dtype in (torch.float32, torch.bfloat16):
    s = setup(B, T, [Lr], dtype, 0)
    filler = s["x"][:, :V].amax(1).float() - s["lse"]
    plain = timed(lambda: run(ops.ctc_align_long, ws, s, B, T), 1, 5)
    ali0, score0 = s["ali"].clone(), s["score"].clone()
    mp = statistics.median(plain)
    say(f"ctc_align_long {str(dtype)[6:]} B=1 T={T} L={Lr} V={V} (again, for the ratios): median {mp / 1e3:.2f} ms")
    for name, gap in (("ends", torch.zeros(B, Lr + 1, dtype=torch.uint8)),
                      ("all", torch.ones(B, Lr + 1, dtype=torch.uint8))):
        gap[:, 0] = gap[:, Lr] = 1
        gap = gap.to(dev)

        def gaps(pen):
            ops.ctc_align_gaps(s["x"], B, T, V, s["lab"], s["llen"], s["ilen"], s["lse"], gap, filler, pen,
                               ali=s["ali"], score=s["score"], feasible=s["feas"], ws=ws)

        gaps(-float("inf"))
        assert s["feas"].tolist() == [1] and torch.equal(s["ali"], ali0) and torch.equal(s["score"], score0)
        one = timed(lambda: gaps(-1.0), 1, 5)
        assert s["feas"].tolist() == [1]
        med = statistics.median(one)
        say(f"ctc_align_gaps {str(dtype)[6:]} flags={name} gap_penalty=-1: median {med / 1e3:.2f} ms = "
            f"{med / T:.3f} us/frame "
            f"(min {min(one) / 1e3:.2f}, max {max(one) / 1e3:.2f} ms, 5 launches), gaps / long = {med / mp:.3f}, "
            f"{int((s['ali'] == ops.CTC_ALIGN_GAP).sum())} gap frames; -inf equals ctc_align_long")
    del s, filler
del ws

if "--parent" in sys.argv:
    with open(sys.argv[sys.argv.index("--parent") + 1]) as f:
        parent = [ln.rstrip("\n") for ln in f if ln.strip()]
else:
    parent = []

os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
with open(os.path.join(ROOT, "profiles", "align_long_kbench.txt"), "w") as f:
    f.write("\n".join(lines[:n_long]) + "\n")
with open(os.path.join(ROOT, "profiles", "align_gaps_kbench.txt"), "w") as f:
    f.write("\n".join(lines + (["parent commit:"] + parent if parent else [])) + "\n")
