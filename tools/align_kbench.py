"""the CTC forced-alignment kernel in isolation: B = 8 utterances of T = 375 frames
(15 s), ~60 labels each, V = 5049 logits (ldx 5056), fp32 and bf16; median of 50 launches timed
one by one with events after warm-up, and the mean of 200 back-to-back launches.
python tools/align_kbench.py"""
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from avsr_amd import ops  # noqa: E402

dev = torch.device("cuda")
B, T, V, Vp = 8, 375, 5049, 5056
LENS = [60, 55, 64, 58, 61, 52, 63, 60]
rng = np.random.Generator(np.random.PCG64(0))
lab = torch.full((B, max(LENS)), -1, dtype=torch.int32)
for b, n in enumerate(LENS):
    lab[b, :n] = torch.from_numpy(rng.integers(1, V - 1, size=n).astype(np.int32))
lab, llen = lab.to(dev), torch.tensor(LENS, dtype=torch.int32).to(dev)
ilen = torch.full((B,), T, dtype=torch.int32).to(dev)
x32 = (torch.randn(B * T, Vp, generator=torch.Generator().manual_seed(0)) * 3).to(dev)
ws = torch.empty(ops.ctc_align_ws(B, T, lab.shape[1]), dtype=torch.uint8, device=dev)
ali = torch.empty(B, T, dtype=torch.int32, device=dev)
score, feas = torch.empty(B, device=dev), torch.empty(B, dtype=torch.int32, device=dev)
for dtype in (torch.float32, torch.bfloat16):
    x = x32.to(dtype)
    lse = torch.empty(B * T, device=dev)
    ops.row_lse(x, V, lse)

    def fn():
        ops.ctc_align(x, B, T, V, lab, llen, ilen, lse, ali=ali, score=score, feasible=feas, ws=ws)

    for _ in range(20):
        fn()
    torch.cuda.synchronize()
    assert feas.tolist() == [1] * B
    one = []
    for _ in range(50):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        one.append(a.elapsed_time(b) * 1e3)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(200):
        fn()
    b.record()
    torch.cuda.synchronize()
    print(f"ctc_align {str(dtype)[6:]} B={B} T={T} L~60 V={V}: median {statistics.median(one):.1f} us "
          f"(min {min(one):.1f}, max {max(one):.1f}, 50 launches), back-to-back {a.elapsed_time(b) * 1e3 / 200:.1f} us",
          flush=True)
