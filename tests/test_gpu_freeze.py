"""requires_grad=False on parameters of AVHubertAVSR (and feature_grad_mult = 0): the backward
gives a gradient to exactly the trainable parameters, prunes what lies below the lowest trainable
unit, and the optimizers leave frozen ranges alone — tiny configuration, golden batch.

Freeze sets: R the video ResNet; F both feature extractors (= feature_grad_mult 0); P = F + fusion
LayerNorm + post_extract_proj + pos-conv + encoder layer 0; E the whole encoder; D the decoder;
C the CTC head."""
import numpy as np
import pytest
import torch
from torch.utils.data import SequentialSampler
from transformers import TrainerCallback, TrainingArguments

from avsr_amd import ops
from avsr_amd.avhubert_avsr_model import AVHubertAVSR
from avsr_amd.configuration_avhubert_avsr import AVHubertAVSRConfig
from avsr_amd.optim import FusedAdamW
from avsr_amd.trainer import AVSRTrainer
from oracle.weights import NO_DROPOUT, TINY_CONFIG
from tests.oracle_util import golden_batch, golden_state, load_golden

pytestmark = pytest.mark.gpu

# the bounds of tests/test_gpu_model_parity.py
TOL = {torch.float32: dict(enc=2e-4, loss=1e-4, grad=2e-3, bn=1e-4),
       torch.bfloat16: dict(enc=6e-2, loss=3e-2, grad=8e-2, bn=5e-2)}

E_ = "encoder."
SETS = {
    "R": [E_ + "feature_extractor_video.resnet"],
    "F": [E_ + "feature_extractor_audio", E_ + "feature_extractor_video"],
    "P": [E_ + "feature_extractor_audio", E_ + "feature_extractor_video", E_ + "layer_norm", E_ + "post_extract_proj",
          E_ + "encoder.pos_conv_embed", E_ + "encoder.layers.0"],
    "E": ["encoder"],
    "D": ["decoder"],
    "C": ["ctc"],
}


@pytest.fixture(scope="module")
def g():
    return load_golden()


def _freeze(m, name, flag=False):
    for sub in SETS[name] if name else []:
        m.avsr.get_submodule(sub).requires_grad_(flag)


def _model(g, dtype, extra=None, dropout=False):
    kw = {**TINY_CONFIG, **({} if dropout else NO_DROPOUT), **(extra or {})}
    m = AVHubertAVSR(AVHubertAVSRConfig(**kw)).train()
    m.load_state_dict({k: torch.from_numpy(v) for k, v in golden_state(g).items()}, strict=True)
    m.setup_engine(torch.device("cuda:0"), dtype)
    return m


def _frozen_names(m):
    """arena names (without the 'avsr.' prefix) of the parameters with requires_grad False"""
    ar = m.avsr.engine().arena
    return {n for n in ar.grad_views if not ar.params[n].requires_grad}


def _slices(ar, names):
    return [(ar.meta[n]["off"], ar.meta[n]["off"] + ar.meta[n]["numel"]) for n in sorted(names)]


def _batch(g):
    return {k: torch.from_numpy(v) for k, v in golden_batch(g).items()}


# ------------------------------------------------------------------ 1. reference parity
def _check_parity(g, m, dtype, frozen_prefixes):
    out = m(**_batch(g))
    loss = torch.stack([out.loss, out.loss_ctc, out.loss_att, out.acc]).detach().cpu().numpy()
    t = TOL[dtype]
    for i in range(3):
        assert abs(loss[i] - g["loss"][i]) / abs(g["loss"][i]) < t["loss"], (i, loss, g["loss"])
    out.loss.backward()
    params = dict(m.named_parameters())
    bad, n_frozen, n_live = [], 0, 0
    for k, n in zip(g["grad_keys"], g["grad_norm"]):
        if k.startswith(frozen_prefixes):
            assert params[k].grad is None, k
            n_frozen += 1
            continue
        gr = params[k].grad
        assert gr is not None and torch.isfinite(gr).all(), k
        n_live += 1
        got = gr.double().norm().item()
        if abs(got - n) > t["grad"] * abs(n) + t["grad"] * 1e-3:
            bad.append((k, got, float(n)))
    assert not bad, bad[:10]
    assert n_frozen > 0 and n_live > 0


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("fs", list(SETS))
def test_reference_parity_of_what_still_trains(g, fs, dtype):
    m = _model(g, dtype)
    _freeze(m, fs)
    _check_parity(g, m, dtype, tuple("avsr." + s + "." for s in SETS[fs]))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_feature_grad_mult_zero_is_set_F(g, dtype):
    m = _model(g, dtype, extra={"feature_grad_mult": 0.0})
    assert all(p.requires_grad for n, p in m.named_parameters() if "feature_extractor" in n)
    _check_parity(g, m, dtype, tuple("avsr." + s + "." for s in SETS["F"]))


def test_nothing_trainable_is_a_forward_without_graph(g):
    m = _model(g, torch.float32)
    m.requires_grad_(False)
    out = m(**_batch(g))
    assert not out.loss.requires_grad
    assert abs(float(out.loss) - g["loss"][0]) / abs(g["loss"][0]) < TOL[torch.float32]["loss"]


def _grads_of(m, batch):
    m.zero_grad()
    out = m(**batch)
    out.loss.backward()
    torch.cuda.synchronize()
    return out.loss.detach().clone(), m.avsr.engine().arena.grad.clone()


@pytest.mark.parametrize("subs", [("encoder.feature_extractor_audio", "encoder.feature_extractor_video"),
                                  ("encoder.feature_extractor_audio", "encoder.feature_extractor_video",
                                   "encoder.layer_norm"),
                                  ("encoder.feature_extractor_audio", "encoder.feature_extractor_video",
                                   "encoder.layer_norm", "encoder.encoder.pos_conv_embed")],
                         ids=["F", "F+ln", "F+ln+posconv"])
def test_modality_fuse_add(g, subs):
    """modality_fuse='add' has no post_extract_proj: the cut falls on the fusion LayerNorm, the
    pos-conv or encoder layer 0; what still trains gets the unfrozen run's gradient bit for bit"""
    from tests.oracle_util import CFGVAR, cfgvar_state, load_cfgvar
    gv = load_cfgvar()

    def model():
        m = AVHubertAVSR(AVHubertAVSRConfig(**{**TINY_CONFIG, **NO_DROPOUT, **CFGVAR["add"]})).train()
        m.load_state_dict({k: torch.from_numpy(v) for k, v in cfgvar_state(gv, "add").items()}, strict=True)
        m.setup_engine("cuda", torch.bfloat16)
        return m
    batch = _batch(g)
    loss0, g0 = _grads_of(model(), batch)
    m = model()
    assert not any("post_extract_proj" in k for k, _ in m.named_parameters())
    for sub in subs:
        m.avsr.get_submodule(sub).requires_grad_(False)
    loss1, g1 = _grads_of(m, batch)
    assert torch.equal(loss0, loss1)
    ar = m.avsr.engine().arena
    frozen = _frozen_names(m)
    live = set(ar.grad_views) - frozen
    bad = [n for n, (s, e) in zip(sorted(live), _slices(ar, live)) if not torch.equal(g0[s:e], g1[s:e])]
    assert not bad, bad[:10]
    assert all(ar.params[n].grad is None for n in frozen) and all(ar.params[n].grad is not None for n in live)


def test_encoder_call_form_follows_the_flags(g):
    """model.avsr.encoder(input_features=, video=) in train mode (surface._EncoderStep): with the
    ResNet frozen its parameters get no gradient and the rest the unfrozen run's, bit for bit; with
    the whole encoder frozen the output carries no graph"""
    batch = _batch(g)
    T = batch["videos"].shape[2]
    wout = torch.randn(T, TINY_CONFIG["hidden_size"], generator=torch.Generator().manual_seed(3)).cuda()

    def run(fs):
        m = _model(g, torch.float32)
        _freeze(m, fs)
        m.avsr.engine().force_modality = None
        np.random.seed(11)                       # the modality draw of the call (numpy's global RNG)
        m.zero_grad()
        out = m.avsr.encoder(input_features=batch["audios"], video=batch["videos"]).last_hidden_state
        if out.requires_grad:
            (out * wout).sum().backward()
        torch.cuda.synchronize()
        return m, out, m.avsr.engine().arena.grad.clone()

    m0, out0, g0 = run(None)
    m1, out1, g1 = run("R")
    assert out0.requires_grad and out1.requires_grad and torch.equal(out0, out1)
    ar = m1.avsr.engine().arena
    frozen = _frozen_names(m1)
    live = {n for n in ar.grad_views if n.startswith("encoder.")} - frozen
    assert frozen and all(ar.params[n].grad is None for n in frozen)
    bad = [n for n, (s, e) in zip(sorted(live), _slices(ar, live)) if not torch.equal(g0[s:e], g1[s:e])]
    assert not bad, bad[:10]
    assert any(float(g1[s:e].abs().max()) > 0 for s, e in _slices(ar, live))
    m2, out2, _ = run("E")
    assert not out2.requires_grad and torch.equal(out2, out0)


def test_flags_changed_between_forward_and_backward(g):
    """the backward follows the forward's snapshot, whatever the flags say by then"""
    batch = _batch(g)
    m = _model(g, torch.float32)
    _, g0 = _grads_of(m, batch)
    m.zero_grad()
    _freeze(m, "D")
    out = m(**batch)
    _freeze(m, "D", True)                        # thawed before the backward: still no gradient
    out.loss.backward()
    torch.cuda.synchronize()
    ar = m.avsr.engine().arena
    dn = [n for n in ar.grad_views if n.startswith("decoder.")]
    assert all(ar.params[n].grad is None for n in dn)
    assert ar.dead_names() == frozenset(dn)
    live = set(ar.grad_views) - set(dn)
    bad = [n for n, (s, e) in zip(sorted(live), _slices(ar, live)) if not torch.equal(g0[s:e], ar.grad[s:e])]
    assert not bad, bad[:10]
    # gradient accumulation: a second micro-step in which D trains gives it a gradient
    _, g2 = _grads_of_more(m, batch)
    assert not ar.dead_names()
    assert all(torch.equal(g2[s:e], g0[s:e]) for s, e in _slices(ar, dn))


def _grads_of_more(m, batch):
    """a further micro-step without a gradient clear"""
    out = m(**batch)
    out.loss.backward()
    torch.cuda.synchronize()
    return out.loss.detach().clone(), m.avsr.engine().arena.grad.clone()


# ------------------------------------------------- 2./3. the bench loop (engine + FusedAdamW)
def _loop(g, fs, *, steps, overlap=False, max_norm=1.0, extra=None, check_sumsq=False):
    """bench.py's loop on the tiny model, bf16, dropouts on, fixed seeds: returns per-step
    gradient arenas and the final state"""
    torch.manual_seed(0)
    m = _model(g, torch.bfloat16, extra=extra, dropout=True)
    _freeze(m, fs)
    eng = m.avsr.engine()
    ar = eng.arena
    b = golden_batch(g)
    v, a = torch.from_numpy(b["videos"]).cuda(), torch.from_numpy(b["audios"]).cuda()
    lens, lab = torch.from_numpy(b["video_lengths"]), torch.from_numpy(b["labels"])
    mtl = eng.cfg.mtlalpha
    d_ctc = torch.full((1,), mtl, device="cuda")
    d_att = torch.full((1,), 1.0 - mtl, device="cuda")
    opt = FusedAdamW(ar, lr=1e-3, weight_decay=0.01, max_grad_norm=max_norm, overlap=overlap)
    eng.pre_video_grads = opt.early_sumsq
    eng.force_modality = (None,)
    torch.manual_seed(1)                  # LayerDrop draws (CPU generator)
    opt.sync()
    torch.cuda.synchronize()
    init = dict(data=ar.data.clone(), shadow=ar.shadow.clone(), exp_avg=ar.exp_avg.clone(),
                exp_avg_sq=ar.exp_avg_sq.clone())
    grads, losses = [], []
    frozen = _frozen_names(m)
    live = set(ar.grad_views) - frozen
    ar.zero_grad()
    for i in range(steps):
        eng.zero_grad_async()
        out4, ctx = eng.forward(v, a, lens, lab, train=True, need_grad=True, seed=100 + i)
        eng.backward(ctx, d_ctc, d_att)
        grads.append(ar.grad.clone())
        if max_norm:
            ss = opt.grad_sumsq()
            if check_sumsq:
                want = sum(float(grads[-1][s:e].double().pow(2).sum()) for s, e in _slices(ar, live))
                print(f"grad_sumsq[{fs}] step {i}: {float(ss):.9g} fp64 {want:.9g}")
                assert abs(float(ss) - want) <= 1e-5 * want, (float(ss), want)
        opt.step(sumsq_ready=bool(max_norm))
        losses.append(out4.clone())
    opt.sync()
    torch.cuda.synchronize()
    final = dict(data=ar.data.clone(), shadow=ar.shadow.clone(), exp_avg=ar.exp_avg.clone(),
                 exp_avg_sq=ar.exp_avg_sq.clone())
    return dict(m=m, ar=ar, opt=opt, grads=grads, losses=losses, init=init, final=final, frozen=frozen, live=live,
                bn=eng.bn_flat.clone())


_BASE = {}


def _base(g):
    """the all-trainable one-step run without clipping, shared by the cases below"""
    if "r" not in _BASE:
        r = _loop(g, None, steps=1, max_norm=0.0)
        _BASE["r"] = {k: r[k] for k in ("grads", "final", "bn", "losses")}
    return _BASE["r"]


@pytest.mark.parametrize("fs", list(SETS))
def test_same_gradients_and_update_as_the_unfrozen_run(g, fs):
    """one step, dropouts on, clipping off: gradient, parameters and moments of every trainable
    parameter are bit-identical to the all-trainable run of the same seed (no kernel variant
    changes with the pruning); BatchNorm statistics of a frozen ResNet move as they did"""
    base = _base(g)
    r = _loop(g, fs, steps=1, max_norm=0.0)
    ar = r["ar"]
    assert torch.equal(r["losses"][0], base["losses"][0])
    bad = [n for n, (s, e) in zip(sorted(r["live"]), _slices(ar, r["live"]))
           if not torch.equal(r["grads"][0][s:e], base["grads"][0][s:e])]
    assert not bad, bad[:10]
    for key in ("data", "shadow", "exp_avg", "exp_avg_sq"):
        bad = [n for n, (s, e) in zip(sorted(r["live"]), _slices(ar, r["live"]))
               if not torch.equal(r["final"][key][s:e], base["final"][key][s:e])]
        assert not bad, (key, bad[:10])
    assert torch.equal(r["bn"], base["bn"])
    assert not torch.equal(r["bn"], torch.zeros_like(r["bn"]))


def _assert_frozen_unmoved(r):
    ar = r["ar"]
    assert r["frozen"]
    for key in ("data", "shadow", "exp_avg", "exp_avg_sq"):
        bad = [n for n, (s, e) in zip(sorted(r["frozen"]), _slices(ar, r["frozen"]))
               if not torch.equal(r["final"][key][s:e], r["init"][key][s:e])]
        assert not bad, (key, bad[:10])
    moved = [n for n, (s, e) in zip(sorted(r["live"]), _slices(ar, r["live"]))
             if not torch.equal(r["final"]["data"][s:e], r["init"]["data"][s:e])]
    assert len(moved) > len(r["live"]) // 2


@pytest.mark.parametrize("fs", list(SETS))
def test_frozen_parameters_do_not_move(g, fs):
    """3 steps of FusedAdamW, serial and overlapped: the frozen slices of the parameters, the bf16
    shadow and both moments keep their initial bits; the clip norm is the norm of the gradients
    that exist; both runs agree bit for bit"""
    ser = _loop(g, fs, steps=3, check_sumsq=True)
    _assert_frozen_unmoved(ser)
    ovl = _loop(g, fs, steps=3, overlap=True)
    _assert_frozen_unmoved(ovl)
    for i in range(3):
        assert torch.equal(ser["losses"][i], ovl["losses"][i]), i
        for s, e in _slices(ser["ar"], ser["live"]):
            assert torch.equal(ser["grads"][i][s:e], ovl["grads"][i][s:e]), i
    for key in ("data", "shadow", "exp_avg", "exp_avg_sq"):
        assert torch.equal(ser["final"][key], ovl["final"][key]), key
    assert ser["opt"].param_skips == ovl["opt"].param_skips
    ar = ser["ar"]
    sk = ser["opt"].param_skips
    assert all(sk[k] == (3 if n in ser["frozen"] else 0) for k, n in enumerate(ar.order))


def test_frozen_parameters_do_not_move_with_layerdrop(g):
    """LayerDrop composes: a layer both frozen and dropped is skipped once (its parameters' own
    count = the layer's count minus the steps that skipped it while its layer ran)"""
    ser = _loop(g, "P", steps=3, extra={"layerdrop": 0.5})
    _assert_frozen_unmoved(ser)
    ovl = _loop(g, "P", steps=3, overlap=True, extra={"layerdrop": 0.5})
    _assert_frozen_unmoved(ovl)
    for key in ("data", "shadow", "exp_avg", "exp_avg_sq"):
        assert torch.equal(ser["final"][key], ovl["final"][key]), key
    assert ser["opt"].layer_steps == ovl["opt"].layer_steps
    assert ser["opt"].param_skips == ovl["opt"].param_skips
    # layer 0 lies below the cut: no backward touches it, so its layer count stands still and its
    # parameters' skip count with it
    ar, opt = ser["ar"], ser["opt"]
    assert opt.layer_steps[0] == 0
    k0 = [k for k, n in enumerate(ar.order) if n.startswith("encoder.encoder.layers.0.")]
    assert k0 and all(opt.param_skips[k] == 0 for k in k0)


# ------------------------------------------------------------------ 4. staged unfreezing
def test_staged_unfreezing_equals_torch_adamw(g):
    """D frozen for 2 steps, trainable for 2 more (overlapped update, which clears only what it
    reads): parameters follow torch.optim.AdamW fed the engine's gradients (None where frozen),
    D's first update uses step 1, nothing the frozen steps left in D's gradient range leaks into
    its first gradient, and the optimizer state survives a state_dict round trip"""
    m = _model(g, torch.float32)
    eng = m.avsr.engine()
    ar = eng.arena
    b = golden_batch(g)
    v, a = torch.from_numpy(b["videos"]).cuda(), torch.from_numpy(b["audios"]).cuda()
    lens, lab = torch.from_numpy(b["video_lengths"]), torch.from_numpy(b["labels"])
    mtl = eng.cfg.mtlalpha
    d_ctc = torch.full((1,), mtl, device="cuda")
    d_att = torch.full((1,), 1.0 - mtl, device="cuda")
    eng.force_modality = (None,)
    opt = FusedAdamW(ar, lr=1e-3, weight_decay=0.005, max_grad_norm=1.0, overlap=True)
    d0, d1 = ar.segments["decay"]
    n0, n1 = ar.segments["no_decay"]
    names = list(ar.grad_views)
    sl = {n: (ar.meta[n]["off"], ar.meta[n]["off"] + ar.meta[n]["numel"]) for n in names}
    tp = {n: torch.nn.Parameter(ar.data[s:e].clone()) for n, (s, e) in sl.items()}
    ref = torch.optim.AdamW([{"params": [tp[n] for n in names if sl[n][0] < d1], "weight_decay": 0.005},
                             {"params": [tp[n] for n in names if sl[n][0] >= n0], "weight_decay": 0.0}],
                            lr=1e-3, betas=(0.9, 0.999), eps=1e-8, foreach=False)
    dnames = [n for n in names if n.startswith("decoder.")]
    _freeze(m, "D")
    ar.zero_grad()

    def step(model, optim):
        e = model.avsr.engine()
        e.zero_grad_async()
        out4, ctx = e.forward(v, a, lens, lab, train=True, need_grad=True, seed=7)
        e.backward(ctx, d_ctc, d_att)
        gr = e.arena.grad.clone()
        optim.step()
        optim.sync()
        return gr

    for i in range(4):
        if i == 2:
            _freeze(m, "D", True)
            after2 = ar.data.clone()
        frozen = _frozen_names(m)
        gr = step(m, opt)
        if i == 2:
            g3 = gr
        live = [n for n in names if n not in frozen]
        norm = torch.sqrt(sum(gr[s:e].double().pow(2).sum() for s, e in (sl[n] for n in live))).item()
        coef = min(1.0, 1.0 / (norm + 1e-6))
        for n in names:
            s, e = sl[n]
            tp[n].grad = None if n in frozen else gr[s:e] * coef
        ref.step()
        err = torch.stack([(ar.data[s:e] - tp[n].detach()).abs().max() for n, (s, e) in sl.items()]).max().item()
        print(f"staged step {i + 1}: max |engine - torch.optim.AdamW| = {err:.3g}")
        assert err < 2e-6, (i, err)
        kd = [k for k, n in enumerate(ar.order) if n.startswith("decoder.")]
        assert all(opt.param_skips[k] == min(i + 1, 2) for k in kd)
        if i == 2:      # D's first update ran at its own step 1 (the others at step 3)
            steps_d = {st for s0, e0 in ((d0, d1), (n0, n1)) for ps, pe, st in opt._pieces(s0, e0)
                       if any(ps <= sl[n][0] < pe for n in dnames)}
            assert steps_d == {1}, steps_d
            assert int(ref.state[tp[dnames[0]]]["step"]) == 1
            sd = opt.state_dict()
            after3 = ar.data.clone()
    assert "param_skips" in sd
    # the first real gradient of D equals that of a model that starts with D trainable
    m2 = _model(g, torch.float32)
    m2.avsr.engine().force_modality = (None,)
    ar2 = m2.avsr.engine().arena
    ar2.data.copy_(after2)
    ar2.sync_shadow()
    opt2 = FusedAdamW(ar2, lr=1e-3, weight_decay=0.005, max_grad_norm=1.0, overlap=True)
    ar2.zero_grad()
    gfresh = step(m2, opt2)
    bad = [n for n in dnames if not torch.equal(g3[sl[n][0]:sl[n][1]], gfresh[sl[n][0]:sl[n][1]])]
    assert not bad, bad[:10]
    assert any(float(g3[sl[n][0]:sl[n][1]].abs().max()) > 0 for n in dnames)
    # state_dict -> load_state_dict on a fresh optimizer after step 3, then step 4
    m3 = _model(g, torch.float32)
    m3.avsr.engine().force_modality = (None,)
    ar3 = m3.avsr.engine().arena
    ar3.data.copy_(after3)
    ar3.sync_shadow()
    opt3 = FusedAdamW(ar3, lr=1e-3, weight_decay=0.005, max_grad_norm=1.0, overlap=True)
    opt3.load_state_dict(sd)
    assert opt3.param_skips == sd["param_skips"].tolist() and opt3.step_count == 3
    ar3.zero_grad()
    step(m3, opt3)
    torch.cuda.synchronize()
    assert torch.equal(ar3.data, ar.data)
    assert torch.equal(ar3.exp_avg, ar.exp_avg) and torch.equal(ar3.exp_avg_sq, ar.exp_avg_sq)
    old = {k: v for k, v in sd.items() if k != "param_skips"}       # a state saved before this feature
    opt3.load_state_dict(old)
    assert opt3.param_skips is None and opt3.step_count == 3


# ------------------------------------------------------------------ 5. pruning happens
class _Calls:
    """host-side call log of avsr_amd.ops entry points during a backward"""
    NAMES = ("conv_bwd_data", "conv_bwd_data_bnr", "conv_bwd_weight", "bn_act_bwd_reduce", "bn_bwd_finalize",
             "bn_bwd_apply", "bn_act_bwd", "stem_pool_bwd", "stem_pool_bwd_reduce", "stem_pool_bwd_apply",
             "stem_wgrad_unpack", "avgpool_bwd", "attn_bwd", "layernorm_bwd", "gemm", "wgrad_group")

    def __init__(self, monkeypatch):
        self.log = []
        self.on = False
        for name in self.NAMES:
            monkeypatch.setattr(ops, name, self._wrap(name, getattr(ops, name)))

    def _wrap(self, name, fn):
        def wrapped(*a, **k):
            if self.on:
                self.log.append((name, a, k))
            return fn(*a, **k)
        return wrapped

    def of(self, *names):
        return [(a, k) for n, a, k in self.log if n in names]


def _backward_calls(g, monkeypatch, fs):
    calls = _Calls(monkeypatch)
    m = _model(g, torch.bfloat16)
    _freeze(m, fs)
    eng = m.avsr.engine()
    n_enc_bwd = []
    real = eng.encoder_bwd
    eng.encoder_bwd = lambda *a, **k: (n_enc_bwd.append(1), real(*a, **k))[1]
    batch = _batch(g)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = m(**batch)
    calls.on = True
    out.loss.backward()
    calls.on = False
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    return calls, m, len(n_enc_bwd), peak


def _in_ranges(t, buf, ranges):
    off = (t.data_ptr() - buf.data_ptr()) // buf.element_size()
    return t.data_ptr() >= buf.data_ptr() and any(s <= off < e for s, e in ranges)


def test_pruning_happens(g, monkeypatch):
    T = golden_batch(g)["videos"].shape[2]
    resnet_ops = ("conv_bwd_data_bnr", "bn_act_bwd_reduce", "bn_bwd_finalize", "bn_bwd_apply", "bn_act_bwd",
                  "stem_pool_bwd", "stem_pool_bwd_reduce", "stem_pool_bwd_apply", "stem_wgrad_unpack", "avgpool_bwd")

    def resnet_convs(c):
        return [a for a, k in c.of("conv_bwd_data", "conv_bwd_weight") if a[0].groups == 1]

    def enc_attn(c):
        return [k for a, k in c.of("attn_bwd") if k["Lq"] == T and k["Lk"] == T]

    def enc_norms(c, m):
        ar = m.avsr.engine().arena
        rs = ar.ranges_of("encoder.")
        return [a for a, k in c.of("layernorm_bwd") if _in_ranges(a[2], ar.data, rs)]

    def dec_wgrads(c, m):
        ar = m.avsr.engine().arena
        rs = ar.ranges_of("decoder.")
        return ([a for a, k in c.of("gemm") if a[2].dtype == torch.float32 and _in_ranges(a[2], ar.grad, rs)]
                + [p for a, k in c.of("wgrad_group") for p in a[0] if _in_ranges(p[2], ar.grad, rs)])

    # all trainable: every one of these happens (so their absence below means something)
    c, m, n_enc, peak_all = _backward_calls(g, monkeypatch, None)
    assert c.of(*resnet_ops) and resnet_convs(c) and enc_attn(c) and enc_norms(c, m) and dec_wgrads(c, m)
    assert n_enc == 1
    # R: nothing of the ResNet backward
    c, m, n_enc, _ = _backward_calls(g, monkeypatch, "R")
    assert not c.of(*resnet_ops) and not resnet_convs(c)
    assert n_enc == 1 and enc_attn(c)
    # E: no encoder backward at all, and less memory held between forward and backward
    c, m, n_enc, peak_e = _backward_calls(g, monkeypatch, "E")
    assert n_enc == 0
    assert not enc_attn(c) and not enc_norms(c, m) and not c.of(*resnet_ops) and not resnet_convs(c)
    assert dec_wgrads(c, m)
    print(f"peak memory of forward + backward: all trainable {peak_all}, encoder frozen {peak_e}")
    assert peak_e < peak_all, (peak_e, peak_all)
    # D above a training encoder: the data-gradient chain runs, the decoder's weight-gradients do not
    c, m, n_enc, _ = _backward_calls(g, monkeypatch, "D")
    assert not dec_wgrads(c, m)
    assert n_enc == 1 and enc_attn(c) and resnet_convs(c)


# ------------------------------------------------------------------ 6. HF Trainer
LABELS2 = [[12, 5, 9, 40], [77, 301, 17]]


def _samples(g):
    """4 samples (2 micro-batches of 2): the golden batch, then the same clips with other labels"""
    b = golden_batch(g)
    out = []
    for labels in (None, LABELS2):
        for i in range(2):
            lab = b["labels"][i][b["labels"][i] != -1] if labels is None else np.array(labels[i])
            out.append({"videos": b["videos"][i], "audios": b["audios"][i], "labels": lab,
                        "video_lengths": b["video_lengths"][i], "audio_lengths": b["audio_lengths"][i]})
    return out


def collate(samples):
    L = max(len(s["labels"]) for s in samples)
    lab = torch.full((len(samples), L), -1, dtype=torch.int64)
    for i, s in enumerate(samples):
        lab[i, :len(s["labels"])] = torch.as_tensor(s["labels"])
    return {"videos": torch.from_numpy(np.stack([s["videos"] for s in samples])),
            "audios": torch.from_numpy(np.stack([s["audios"] for s in samples])),
            "labels": lab,
            "video_lengths": torch.tensor([int(s["video_lengths"]) for s in samples]),
            "audio_lengths": torch.tensor([int(s["audio_lengths"]) for s in samples]),
            "label_lengths": torch.tensor([len(s["labels"]) for s in samples])}


class SeqTrainer(AVSRTrainer):
    def _get_train_sampler(self, *a, **k):
        return SequentialSampler(self.train_dataset)


class StopAfter(TrainerCallback):
    def __init__(self, n):
        self.n = n

    def on_step_end(self, args, state, control, **kw):
        if state.global_step >= self.n:
            control.should_save = True
            control.should_training_stop = True
        return control


class FreezeEncoderUntil(TrainerCallback):
    """the usual recipe: the encoder is frozen for the first n updates"""

    def __init__(self, model, n):
        self.model, self.n = model, n

    def on_step_begin(self, args, state, control, **kw):
        self.model.avsr.encoder.requires_grad_(state.global_step >= self.n)


class Capture(TrainerCallback):
    def __init__(self, model):
        self.model, self.before, self.after = model, [], []

    def on_pre_optimizer_step(self, args, state, control, **kw):
        self.before.append(self.model.avsr.engine().arena.data.clone())

    def on_optimizer_step(self, args, state, control, **kw):
        self.after.append(self.model.avsr.engine().arena.data.clone())


def _args(out, steps, **kw):
    a = dict(output_dir=str(out), per_device_train_batch_size=2, gradient_accumulation_steps=2, max_steps=steps,
             learning_rate=1e-3, weight_decay=0.005, warmup_steps=0, max_grad_norm=1.0, report_to="none",
             remove_unused_columns=False, dataloader_num_workers=0, logging_steps=1, seed=0, save_strategy="no",
             dataloader_drop_last=True)
    a.update(kw)
    return TrainingArguments(**a)


def _tmodel(g):
    m = AVHubertAVSR(AVHubertAVSRConfig(**TINY_CONFIG, **NO_DROPOUT))
    m.load_state_dict({k: torch.from_numpy(v) for k, v in golden_state(g).items()}, strict=True)
    return m


def test_trainer_callback_unfreezes_the_encoder(g, tmp_path):
    ds = _samples(g) * 2                  # 2 optimizer steps of GA 2 x batch 2
    m1 = _tmodel(g)
    cap1 = Capture(m1)
    SeqTrainer(model=m1, args=_args(tmp_path / "a", 2), data_collator=collate, train_dataset=ds,
               callbacks=[FreezeEncoderUntil(m1, 1), cap1]).train()
    ar = m1.avsr.engine().arena
    enc = [(s, e) for s, e in _slices(ar, [n for n in ar.grad_views if n.startswith("encoder.")])]
    dec = [(s, e) for s, e in _slices(ar, [n for n in ar.grad_views if n.startswith("decoder.")])]
    assert len(cap1.after) == 2
    assert all(torch.equal(cap1.after[0][s:e], cap1.before[0][s:e]) for s, e in enc)     # step 1: frozen
    assert sum(not torch.equal(cap1.after[0][s:e], cap1.before[0][s:e]) for s, e in dec) > len(dec) // 2
    assert sum(not torch.equal(cap1.after[1][s:e], cap1.before[1][s:e]) for s, e in enc) > len(enc) // 2
    # stop after step 1 with a checkpoint, resume for step 2: the straight run, bit for bit
    m2 = _tmodel(g)
    SeqTrainer(model=m2, args=_args(tmp_path / "b", 2, save_strategy="steps", save_steps=1), data_collator=collate,
               train_dataset=ds, callbacks=[FreezeEncoderUntil(m2, 1), StopAfter(1)]).train()
    m3 = _tmodel(g)
    cap3 = Capture(m3)
    tr3 = SeqTrainer(model=m3, args=_args(tmp_path / "b", 2, save_strategy="no"), data_collator=collate,
                     train_dataset=ds, callbacks=[FreezeEncoderUntil(m3, 1), cap3])
    tr3.train(resume_from_checkpoint=str(tmp_path / "b" / "checkpoint-1"))
    assert len(cap3.after) == 1 and tr3.state.global_step == 2
    a1, a3 = m1.avsr.engine().arena, m3.avsr.engine().arena
    assert torch.equal(cap3.before[0], cap1.before[1])
    assert torch.equal(a1.exp_avg, a3.exp_avg) and torch.equal(a1.exp_avg_sq, a3.exp_avg_sq)
    assert torch.equal(a1.data, a3.data)
    assert m1.avsr.engine().arena is a1 and tr3.optimizer is not None
