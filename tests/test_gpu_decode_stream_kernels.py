"""The per-row-position forms of the beam-search step kernels (a decode session's rows stand at
different steps) against the existing shared-position forms, with torch.equal: each slot's rows
of a per-row launch equal a scalar-form launch at that slot's position. Geometry: 2 slots x beam 3
= 6 rows, D = 64, V = 32, P = 4, 12 positions; slot positions [0, 5] and [7, 0]."""
import numpy as np
import pytest
import torch

from avsr_amd import ops
from avsr_amd.decode import BatchBeamSearch, D_END

pytestmark = pytest.mark.gpu

S, BEAM, D, V, P, TCAP = 2, 3, 64, 32, 4, 12
R = S * BEAM
UPOS = [[0, 5], [7, 0]]
INF = float("inf")


def _i32(x, dev):
    return torch.as_tensor(np.asarray(x), dtype=torch.int32).to(dev)


def _rowpos(upos, dev):
    return _i32([upos[r // BEAM] for r in range(R)], dev)


def _slot_rows(u):
    return slice(u * BEAM, (u + 1) * BEAM)


@pytest.mark.parametrize("upos", UPOS)
def test_beam_step_prep_per_row(dev, upos):
    g = torch.Generator().manual_seed(1)
    anc0 = torch.randint(0, 1000, (R, TCAP), generator=g, dtype=torch.int32).to(dev)
    anc, klen = anc0.clone(), torch.full((R,), -1, dtype=torch.int32, device=dev)
    ops.beam_step_prep(R, _rowpos(upos, dev), anc, klen, per_row=True)
    for u in range(S):
        a, k = anc0.clone(), torch.full((R,), -1, dtype=torch.int32, device=dev)
        ops.beam_step_prep(R, _i32([upos[u]], dev), a, k)
        assert torch.equal(anc[_slot_rows(u)], a[_slot_rows(u)]) and torch.equal(klen[_slot_rows(u)], k[_slot_rows(u)])
        assert anc[u * BEAM, upos[u]].item() == upos[u] * R + u * BEAM


def _merged_cache(init, upos, launch):
    """the cache a per-row launch must leave: `init` with, per slot, the rows pos*R + r of a
    scalar launch at that slot's position (`launch(pos tensor, cache k, cache v)`)"""
    want = [c.clone() for c in init]
    outs = []
    for u in range(S):
        c = [t.clone() for t in init]
        outs.append(launch(_i32([upos[u]], init[0].device), *c))
        rows = [upos[u] * R + r for r in range(u * BEAM, (u + 1) * BEAM)]
        for w, t in zip(want, c):
            w[rows] = t[rows]
    return want, outs


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("upos", UPOS)
def test_beam_kv_put_per_row(dev, upos, dtype):
    g = torch.Generator().manual_seed(2)
    qkv = torch.randn(R, 3 * D, generator=g).to(dtype).to(dev)
    init = [torch.randn(TCAP * R, D, generator=g).to(dtype).to(dev) for _ in range(2)]
    want, _ = _merged_cache(init, upos, lambda pos, kc, vc: ops.beam_kv_put(qkv, kc, vc, pos, R, D))
    kc, vc = init[0].clone(), init[1].clone()
    ops.beam_kv_put(qkv, kc, vc, _rowpos(upos, dev), R, D, per_row=True)
    assert torch.equal(kc, want[0]) and torch.equal(vc, want[1])
    assert not torch.equal(kc, init[0])


@pytest.mark.parametrize("upos", UPOS)
def test_embed_per_row_position(dev, upos):
    g = torch.Generator().manual_seed(3)
    tok = _i32(torch.randint(0, V, (R,), generator=g), dev)
    table, pe = torch.randn(V, D, generator=g).to(dev), torch.randn(TCAP, D, generator=g).to(dev)
    y = torch.empty(R, D, device=dev)
    ops.embed_fwd(tok, table, pe, 8.0, y, 1, pe_row=_rowpos(upos, dev), per_row=True)
    for u in range(S):
        yu = torch.empty(R, D, device=dev)
        ops.embed_fwd(tok, table, pe, 8.0, yu, 1, pe_row=_i32([upos[u]], dev))
        assert torch.equal(y[_slot_rows(u)], yu[_slot_rows(u)])
    y0 = torch.empty(R, D, device=dev)
    ops.embed_fwd(tok, table, pe, 8.0, y0, 1, pe_row=_i32([upos[0]], dev))
    assert not torch.equal(y[_slot_rows(1)], y0[_slot_rows(1)])      # (the positions do differ)


@pytest.mark.parametrize("fold", [False, True])
@pytest.mark.parametrize("upos", UPOS)
def test_few_row_gemm_kv_append_per_row(dev, upos, fold):
    """N = 3 * 64, K = 64, 6 rows: C (the Q third) and the appended cache rows equal two
    scalar-form launches, with and without the LayerNorm prologue"""
    g = torch.Generator().manual_seed(4)
    x = torch.randn(R, D, generator=g).to(dev)
    W, b = (torch.randn(3 * D, D, generator=g) / 8).to(dev), torch.randn(3 * D, generator=g).to(dev)
    kw = {}
    if fold:
        W, b, c1 = ops.fold_layernorm(W, b, torch.rand(D, generator=g).to(dev) + 0.5, torch.randn(D, generator=g).to(dev))
        kw = dict(ln=(c1, 1e-12))
    init = [torch.randn(TCAP * R, D, generator=g).to(dev) for _ in range(2)]
    want, outs = _merged_cache(init, upos, lambda pos, kc, vc: ops.linear_fwd(x, W, b, kv=(kc, vc, pos, R), **kw).clone())
    kc, vc = init[0].clone(), init[1].clone()
    C = ops.linear_fwd(x, W, b, kv=(kc, vc, _rowpos(upos, dev), R, True), **kw)
    assert torch.equal(kc, want[0]) and torch.equal(vc, want[1])
    for u in range(S):
        assert torch.equal(C[_slot_rows(u), :D], outs[u][_slot_rows(u), :D])


# ---------------------------------------------------------------------------- ctc_prefix
V_CTC = 300


@pytest.mark.parametrize("lens", [[0, 0, 0, 3, 3, 3], [3, 3, 3, 0, 0, 0]])
@pytest.mark.parametrize("T,Pc", [(40, 4), (245, 64)], ids=["lds", "fallback"])
def test_ctc_prefix_per_row_length(dev, T, Pc, lens):
    """both prefix kernels (245 frames x (64 + 3) floats exceed 64 KiB of LDS: the fallback): rows of
    length 0 equal the scalar launch with r_prev = None, rows of length 3 the scalar launch with
    the given r_prev, for psi and r_new; two utterances of unequal length"""
    assert (T * (Pc + 3) * 4 > 65536) == (T == 245)
    g = torch.Generator().manual_seed(5)
    eos = V_CTC - 1
    tlen = [T, T - 7]
    logp = torch.log_softmax(torch.randn(S, T, V_CTC, generator=g) * 3, -1).to(dev)
    ids = torch.stack([torch.randperm(V_CTC - 22, generator=g)[:Pc] + 20 for _ in range(R)]).to(torch.int32)
    last = torch.randint(20, V_CTC - 2, (R,), generator=g, dtype=torch.int32)
    ids[1, 0], ids[4, 0] = last[1], last[4]          # a repeated label
    ids[2, 1], ids[5, 1] = eos, eos
    ids[0, 2], ids[3, 2] = 0, 0                      # blank among the scored ids
    ids, last = ids.to(dev), last.to(dev)
    r_prev = (torch.log_softmax(torch.randn(R, T, 2, generator=g), -1) - 3.0).to(dev)
    kw = dict(n=R, out_len=0, blank=0, eos=eos, uidx=_i32([r // BEAM for r in range(R)], dev), tlen=_i32(tlen, dev))

    def launch(rp, out_len_dev, per_row=False):
        r_new, psi = torch.zeros(R, Pc, T, 2, device=dev), torch.zeros(R, Pc + 1, device=dev)
        ops.ctc_prefix(logp, rp, last, ids, r_new, psi, out_len_dev=out_len_dev, per_row=per_row, **kw)
        return psi, r_new
    psi, r_new = launch(r_prev, _i32(lens, dev), per_row=True)
    ref = {0: launch(None, _i32([0], dev)), 3: launch(r_prev, _i32([3], dev))}
    assert not torch.equal(ref[0][0], ref[3][0])
    for h in range(R):
        Tu = tlen[h // BEAM]
        want_psi, want_r = ref[lens[h]]
        assert torch.equal(psi[h], want_psi[h]), h
        assert torch.equal(r_new[h, :, :Tu], want_r[h, :, :Tu]), h


@pytest.mark.parametrize("T,Pc", [(40, 4), (245, 64)], ids=["lds", "fallback"])
def test_ctc_prefix_per_row_length_of_a_single_row(dev, T, Pc):
    """one row (a session of one slot at beam 1): its length tensor has one element in either
    form, so the form is what the caller states. Per row, length 0 ignores r_prev (the first
    step); shared, the same tensor with the same r_prev is a later step of length 0"""
    g = torch.Generator().manual_seed(8)
    logp = torch.log_softmax(torch.randn(T, V_CTC, generator=g) * 3, -1).to(dev)
    ids = (torch.randperm(V_CTC - 22, generator=g)[:Pc] + 20).to(torch.int32).view(1, Pc).to(dev)
    last = _i32([V_CTC - 1], dev)
    r_prev = (torch.log_softmax(torch.randn(1, T, 2, generator=g), -1) - 3.0).to(dev)
    zero = _i32([0], dev)

    def launch(rp, per_row):
        r_new, psi = torch.zeros(1, Pc, T, 2, device=dev), torch.zeros(1, Pc + 1, device=dev)
        ops.ctc_prefix(logp, rp, last, ids, r_new, psi, n=1, out_len=0, blank=0, eos=V_CTC - 1, out_len_dev=zero,
                       per_row=per_row)
        return psi, r_new
    first, rows, shared = launch(None, False), launch(r_prev, True), launch(r_prev, False)
    assert torch.equal(rows[0], first[0]) and torch.equal(rows[1], first[1])
    assert not torch.equal(shared[0], first[0])


# ---------------------------------------------------------------------------- beam_post
HIST = ("bp_prev", "bp_tok", "end_flag", "end_score", "end_dec", "end_ctc")
ROWS = ("tok", "score", "sdec", "sctc", "s_prev")
EOS = V - 1


def _post_state(g, nslot, dev):
    """a mid-search state of nslot slots (host tensors): finite scores and sums, some best_len
    entries set, a history of recognisable values"""
    n = nslot * BEAM
    f64 = torch.float64
    st = dict(tok=torch.randint(1, EOS, (n,), generator=g, dtype=torch.int32), score=-torch.rand(n, generator=g) * 9,
              sdec=-torch.rand(n, generator=g, dtype=f64) * 9, sctc=-torch.rand(n, generator=g, dtype=f64) * 9,
              s_prev=-torch.rand(n, generator=g) * 9, src=torch.full((2 * n,), -7, dtype=torch.int32),
              bp_prev=torch.full((TCAP, n), -3, dtype=torch.int32), bp_tok=torch.full((TCAP, n), -4, dtype=torch.int32),
              end_flag=torch.full((TCAP, n), -5, dtype=torch.int32), end_score=torch.full((TCAP, n), 0.25),
              end_dec=torch.full((TCAP, n), 0.5, dtype=f64), end_ctc=torch.full((TCAP, n), 0.75, dtype=f64),
              best_len=torch.full((nslot, TCAP + 3), -INF), best_end=torch.full((nslot,), -INF))
    return st


def _sel(g, toks):
    """a selection per slot: parents within the slot, descending scores"""
    sel = dict(prev=torch.cat([torch.randint(0, BEAM, (BEAM,), generator=g, dtype=torch.int32) + u * BEAM
                               for u in range(S)]),
               tok=torch.tensor(toks, dtype=torch.int32), col=torch.randint(0, P, (R,), generator=g, dtype=torch.int32),
               score=torch.cat([-torch.sort(torch.rand(BEAM, generator=g) * 5).values - 1 for _ in range(S)]),
               dec=-torch.rand(R, generator=g), ctc=-torch.rand(R, generator=g), s=-torch.rand(R, generator=g) * 20)
    return sel


def _post_launch(dev, nslot, st, sel, maxlen, done, end_detect, **pos):
    d = {k: v.clone().to(dev) for k, v in st.items()}
    d["done"] = _i32(done + [sum(done)], dev)
    pos = {k: _i32(v, dev) for k, v in pos.items()}
    ops.beam_post(U=nslot, beam=BEAM, P=P, R=nslot * BEAM, Lmax=TCAP, steps_cap=TCAP - 1, eos=EOS, end_detect=end_detect,
                  d_end=float(D_END), maxlen=_i32(maxlen, dev), **{"sel_" + k: v.to(dev) for k, v in sel.items()},
                  **d, **pos)
    d.update(pos)
    return {k: v.cpu() for k, v in d.items()}


POST_CASES = {
    # upos, maxlen, done before, tokens picked (EOS = the eos), best_len entries [(slot, len, score)]
    "both_advance": ([4, 0], [9, 9], [0, 0], [3, 4, 5, 6, 7, 8], []),
    "done_slot_keeps_its_position": ([4, 0], [9, 9], [1, 0], [3, 4, 5, 6, 7, 8], []),
    "other_slot_done": ([4, 0], [9, 9], [0, 1], [3, 4, 5, 6, 7, 8], []),
    "forced_eos_slot0": ([4, 0], [5, 9], [0, 0], [3, 4, 5, 6, 7, 8], []),
    "forced_eos_slot1_at_step0": ([4, 0], [9, 1], [0, 0], [3, 4, 5, 6, 7, 8], []),
    "eos_picks": ([4, 0], [9, 9], [0, 0], [EOS, 4, EOS, 6, EOS, 8], []),
    "no_live_row": ([4, 0], [9, 9], [0, 0], [EOS, EOS, EOS, 6, 7, 8], []),
    "end_detection_slot0": ([4, 0], [9, 9], [0, 0], [3, 4, 5, 6, 7, 8], [(0, 2, -30.0), (0, 3, -31.0), (0, 4, -32.0),
                                                                        (0, 5, -1.0)]),
    "swapped": ([0, 4], [9, 5], [0, 0], [3, EOS, 5, 6, 7, 8], []),
}


@pytest.mark.parametrize("end_detect", [1, 0])
@pytest.mark.parametrize("case", POST_CASES, ids=list(POST_CASES))
def test_beam_post_per_slot(dev, case, end_detect):
    """one step of two slots at different positions against the scalar kernel run on each slot's
    rows alone (U = 1, its rows renumbered from 0): state, history records, src, done, best_len
    and best_end equal; a slot done before the step keeps upos, every other advances; the forced
    eos at maxlen - 1 fires per slot"""
    upos, maxlen, done, toks, bl = POST_CASES[case]
    g = torch.Generator().manual_seed(6)
    st, sel = _post_state(g, S, dev), _sel(g, toks)
    for u, ln, sc in bl:
        st["best_len"][u, ln] = sc
        st["best_end"][u] = max(st["best_end"][u].item(), sc)
    for u in range(S):
        if done[u]:
            st["score"][_slot_rows(u)] = -INF
    got = _post_launch(dev, S, st, sel, maxlen, done, end_detect, upos=upos, rowpos=[-1] * R)
    for u in range(S):
        rows, off = _slot_rows(u), u * BEAM
        one = {k: (v[:, rows] if k in HIST else v[u:u + 1] if k in ("best_len", "best_end") else
                   torch.full((2 * BEAM,), -7, dtype=torch.int32) if k == "src" else v[rows]) for k, v in st.items()}
        s1 = {k: v[rows] - (off if k == "prev" else 0) for k, v in sel.items()}
        ref = _post_launch(dev, 1, one, s1, [maxlen[u]], [done[u]], end_detect, pos=[upos[u]])
        for k in ROWS:
            assert torch.equal(got[k][rows], ref[k]), (u, k)
        assert torch.equal(got["src"][rows], ref["src"][:BEAM] + off)
        assert torch.equal(got["src"][R:][rows], ref["src"][BEAM:] + off * P)
        for k in HIST:
            want = ref[k].clone()
            if k == "bp_prev":
                want[upos[u]] += off
            assert torch.equal(got[k][:, rows], want), (u, k)
        assert torch.equal(got["best_len"][u], ref["best_len"][0]) and torch.equal(got["best_end"][u], ref["best_end"][0])
        assert got["done"][u] == ref["done"][0]
        assert got["upos"][u].item() == (upos[u] if done[u] else upos[u] + 1)
        if not done[u]:
            assert ref["pos"].item() == upos[u] + 1
            forced = upos[u] == maxlen[u] - 1
            assert (got["end_flag"][upos[u], rows] == 2).all().item() == forced
            if forced:
                assert got["done"][u] == 1
    assert got["done"][S] == got["done"][:S].sum()
    assert got["rowpos"].tolist() == [got["upos"][r // BEAM].item() for r in range(R)]
    if case == "end_detection_slot0":
        assert got["done"].tolist() == ([1, 0, 1] if end_detect else [0, 0, 0])
    if case == "no_live_row":
        assert got["done"].tolist() == [1, 0, 1]


# ---------------------------------------------------------------------------- beam_slot_reset
def test_beam_slot_reset(dev):
    """after garbage in every array, slot 1 holds what `_new_state` gives a fresh utterance and
    slot 0 is bit-unchanged"""
    bs = BatchBeamSearch(None, beam_size=BEAM, vocab_size=V, weights={"decoder": 0.7, "ctc": 0.3}, sos=EOS, eos=EOS)
    Ts, maxlens = [7, 9], [6, 9]
    fresh = bs._new_state(dev, torch.float32, Ts, maxlens, torch.zeros(S, 9, V, device=dev), None, D, 0)
    Lmax = fresh["Lmax"]
    g = torch.Generator().manual_seed(7)
    keys = ("tok", "score", "sdec", "sctc", "s_prev", "best_len", "best_end", "maxlen", "tlen", "klen_mem")
    junk = {}
    for k in keys:
        t = fresh[k]
        junk[k] = (torch.randint(1, 50, t.shape, generator=g, dtype=torch.int32) if t.dtype == torch.int32 else
                   torch.randn(t.shape, generator=g, dtype=t.dtype) * 100).to(dev)
    junk.update(upos=_i32([5, 3], dev), rowpos=_i32([5, 5, 5, 3, 3, 3], dev), done=_i32([1, 1, 2], dev))
    st = {k: v.clone() for k, v in junk.items()}
    ops.beam_slot_reset(U=S, beam=BEAM, Lmax=Lmax, slot=1, sos=EOS, maxlen=maxlens[1], tlen=Ts[1], upos=st["upos"],
                        rowpos=st["rowpos"], done=st["done"], tok=st["tok"], score=st["score"], sdec=st["sdec"],
                        sctc=st["sctc"], s_prev=st["s_prev"], best_len=st["best_len"], best_end=st["best_end"],
                        maxlen_arr=st["maxlen"], tlen_arr=st["tlen"], klen_mem=st["klen_mem"])
    per_row = ("tok", "score", "sdec", "sctc", "s_prev", "klen_mem")
    for k in keys:
        sl = (lambda u: _slot_rows(u)) if k in per_row else (lambda u: slice(u, u + 1))
        assert torch.equal(st[k][sl(1)], fresh[k][sl(1)]), k
        assert torch.equal(st[k][sl(0)], junk[k][sl(0)]), k
    assert st["upos"].tolist() == [5, 0] and st["rowpos"].tolist() == [5, 5, 5, 0, 0, 0]
    assert st["done"].tolist() == [1, 0, 1]
    assert st["score"][_slot_rows(1)].tolist() == [0.0, -INF, -INF] and st["tok"][_slot_rows(1)].tolist() == [EOS] * BEAM
