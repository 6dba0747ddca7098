"""Frozen parameters (requires_grad=False) under data parallelism, world_size 2 over gloo.

CPU: GradReducer with `written` ranges — a bucket that meets no written range is not exchanged
(it keeps its per-rank sentinel values and costs no all_reduce call), everything else equals a
plain all-reduce, also when the backward stopped early and finish() has to send the rest.

GPU (two ranks on cuda:0, like test_gpu_dp.py): the tiny model with the ResNet frozen on both
ranks, 2 steps of ArenaDDP + ArenaAdamW — the replicas stay identical and the frozen slice of the
parameter arena does not move."""
import os
import socket

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from avsr_amd import parallel


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _spawn(worker, world=2, timeout=120):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = dict(q.get(timeout=timeout) for _ in range(world))
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    return res


N = 100003                      # odd: the last tail bucket is short
STEP = 10000                    # elements per bucket
SEG = (1000, 90000)             # "decay segment": buckets (80000, 90000), ..., (1000, 10000)
# ranges with a gradient: the buckets (30000, 40000) ... (1000, 10000) lie wholly outside them, and
# so does the tail bucket (90000, 100000); (40000, 50000) is met by 5 elements only
WRITTEN = [(0, 500), (49995, 90000), (100000, N)]


def _count_calls():
    calls = []
    real = dist.all_reduce

    def counted(t, *a, **k):
        calls.append(t.numel())
        return real(t, *a, **k)
    dist.all_reduce = counted
    return calls, real


def _worker(rank, world, port, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      LOCAL_RANK=str(rank))
    res = {}
    try:
        parallel.init_from_env(backend="gloo")
        base = torch.arange(N, dtype=torch.float32) * (rank + 1)         # per-rank values = sentinels
        want = torch.arange(N, dtype=torch.float32) * sum(range(1, world + 1))
        calls, real = _count_calls()
        try:
            full = base.clone()
            red = parallel.GradReducer(full, bucket_bytes=4 * STEP, segment=SEG)
            red.allreduce(average=False)
            n_all = len(calls)
            res["plain"] = bool(torch.equal(full, want)) and n_all == len(red.buckets) + len(red.tail)

            def sent(a, b):
                return any(s < b and a < e for s, e in WRITTEN)
            every = red.buckets + red.tail
            n_skip = sum(not sent(a, b) for a, b in every)
            expect = base.clone()
            for a, b in every:
                if sent(a, b):
                    expect[a:b] = want[a:b]
            res["n_skip"] = n_skip
            # watermarks all the way down, then finish()
            del calls[:]
            g = base.clone()
            red = parallel.GradReducer(g, bucket_bytes=4 * STEP, segment=SEG)
            red.written = WRITTEN
            red.begin()
            for off in (85000, 60000, 60000, 20000, 1000):
                red.ready(off)
            red.finish(average=False)
            res["marks"] = bool(torch.equal(g, expect))
            res["marks_calls"] = (len(calls), n_all - n_skip, red.skipped)
            # the backward stopped early: ready() never called below 60000; finish() sends the rest
            del calls[:]
            g = base.clone()
            red = parallel.GradReducer(g, bucket_bytes=4 * STEP, segment=SEG)
            red.written = WRITTEN
            red.begin()
            red.ready(60000)
            res["early_before_finish"] = len(calls)
            red.finish(average=False)
            res["early"] = bool(torch.equal(g, expect))
            res["early_calls"] = (len(calls), n_all - n_skip, red.skipped)
            # written=None is the old behaviour
            del calls[:]
            g = base.clone()
            red = parallel.GradReducer(g, bucket_bytes=4 * STEP, segment=SEG)
            red.begin()
            red.ready(60000)
            red.finish(average=False)
            res["none"] = bool(torch.equal(g, want)) and len(calls) == n_all and red.skipped == 0
        finally:
            dist.all_reduce = real
    except Exception:  # pragma: no cover - reported to the parent
        import traceback
        res["error"] = traceback.format_exc()
    finally:
        q.put((rank, res))
        if dist.is_initialized():
            dist.destroy_process_group()


def test_grad_reducer_skips_unwritten_buckets_world2():
    res = _spawn(_worker)
    for rank in range(2):
        r = res[rank]
        assert "error" not in r, r.get("error")
        assert r["plain"], r
        assert r["n_skip"] == 5, r                      # 4 decay buckets + 1 tail bucket
        assert r["marks"], r
        assert r["marks_calls"][0] == r["marks_calls"][1] and r["marks_calls"][2] == r["n_skip"], r
        assert r["early_before_finish"] == 3, r         # (80000, 90000), (70000, 80000), (60000, 70000)
        assert r["early"], r
        assert r["early_calls"][0] == r["early_calls"][1] and r["early_calls"][2] == r["n_skip"], r
        assert r["none"], r


def test_written_ranges_are_the_complement_of_the_dead_ones():
    """Arena.written_ranges (CPU layout arena): None with nothing frozen; with a module frozen in
    every backward since the clear, everything but its (alignment-padded) ranges"""
    from avsr_amd.arena import Arena
    root = torch.nn.Sequential(torch.nn.Linear(100, 70), torch.nn.Linear(70, 30), torch.nn.LayerNorm(30))
    ar = Arena(root, "cpu", torch.float32)
    assert ar.snapshot().all and ar.written_ranges() is None
    ar.begin_backward(ar.snapshot())
    assert ar.written_ranges() is None and not ar.dead_names()
    ar.zero_grad()
    root[1].requires_grad_(False)
    snap = ar.snapshot()
    assert snap.frozen == {"1.weight", "1.bias"} and snap.any and not snap.all
    assert ar.snapshot() is snap                        # cached per flag vector
    ar.begin_backward(snap)
    dead = ar.dead_ranges()
    m = ar.meta
    assert [s for s, _ in dead] == sorted([m["1.weight"]["off"], m["1.bias"]["off"]])
    wr = ar.written_ranges()
    covered = sorted(dead + wr)
    assert covered[0][0] == 0 and covered[-1][1] == ar.total
    assert all(a[1] == b[0] for a, b in zip(covered, covered[1:]))
    # a micro-step in which the module trains: it has a gradient at the optimizer step
    root[1].requires_grad_(True)
    ar.begin_backward(ar.snapshot())
    assert ar.written_ranges() is None
    # .grad follows the flags: None while frozen, the arena view again afterwards
    root[1].requires_grad_(False)
    ar.attach_grads()
    assert root[1].weight.grad is None and root[0].weight.grad is not None
    root[1].requires_grad_(True)
    ar.grad.fill_(3.0)
    ar.attach_grads()
    assert root[1].weight.grad is not None and float(root[1].weight.grad.abs().max()) == 0.0
    assert float(root[0].weight.grad.min()) == 3.0


# ---------------------------------------------------------------------------------- GPU
def _gpu_worker(rank, world, port, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      LOCAL_RANK="0", HSA_ENABLE_IPC_MODE_LEGACY="0")
    res = {}
    try:
        import sys
        sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
        torch.cuda.set_device(0)
        from avsr_amd.avhubert_avsr_model import AVHubertAVSR
        from avsr_amd.configuration_avhubert_avsr import AVHubertAVSRConfig
        from avsr_amd.optim import ArenaAdamW
        from oracle.weights import NO_DROPOUT, TINY_CONFIG
        from tests.oracle_util import golden_batch, golden_state, load_golden
        dist.init_process_group("gloo", rank=rank, world_size=world)
        g = load_golden()
        state = {k: torch.from_numpy(v) for k, v in golden_state(g).items()}
        batch = {k: torch.from_numpy(v) for k, v in golden_batch(g).items()}
        m = AVHubertAVSR(AVHubertAVSRConfig(**TINY_CONFIG, **NO_DROPOUT)).train()
        m.load_state_dict(state, strict=True)
        m.setup_engine("cuda:0", torch.float32)
        m.avsr.encoder.feature_extractor_video.resnet.requires_grad_(False)
        eng = m.avsr.engine()
        ar = eng.arena
        ddp = parallel.ArenaDDP(m, bucket_bytes=1 << 18, average=True, use_stream=True)
        opt = ArenaAdamW(ar, lr=1e-3, weight_decay=0.01)
        rn = ar.ranges_of("encoder.feature_extractor_video.resnet.")
        before = ar.data.clone()
        shard = {k: v[rank:rank + 1].contiguous() for k, v in batch.items()}
        skipped = []
        for _ in range(2):
            opt.zero_grad()
            m(**shard).loss.backward()
            skipped.append(ddp.reducer.skipped)
            opt.clip_grad_norm_(1.0)
            opt.step()
        torch.cuda.synchronize()
        res["skipped"] = skipped
        res["frozen_same"] = all(bool(torch.equal(ar.data[a:b], before[a:b])) for a, b in rn)
        res["moved"] = bool((ar.data != before).any())
        both = [torch.empty_like(ar.data) for _ in range(world)]
        dist.all_gather(both, ar.data)
        res["ranks_equal"] = bool(torch.equal(both[0], both[1]))
        res["finite"] = bool(torch.isfinite(ar.data).all())
    except Exception:  # pragma: no cover - reported to the parent
        import traceback
        res["error"] = traceback.format_exc()
    finally:
        q.put((rank, res))
        if dist.is_initialized():
            dist.destroy_process_group()


@pytest.mark.gpu
def test_dp_world2_frozen_resnet_two_steps():
    res = _spawn(_gpu_worker, timeout=240)
    for rank in range(2):
        r = res[rank]
        assert "error" not in r, r.get("error")
        assert r["finite"] and r["moved"], r
        assert r["frozen_same"], r
        assert r["ranks_equal"], r
        assert all(s > 0 for s in r["skipped"]), r       # whole buckets lie inside the frozen ResNet
