"""The device-side beam-search kernels (decode_softmax.hip, dec_attn.hip, ctc_prefix.hip,
beam.hip), one by one, against the plain references of tests/decode_ref.py (fp64 / exact integer logic written from include/avsr_hip.h) and the CPU
oracle's CTC prefix scorer: both CTC prefix kernels with the batched fields, beam selection with
true ties, the bookkeeping state machine, the one-query attention's kmap / bf16 / partial-group /
key-split paths, top-k ties, and the exact data movers."""
import numpy as np
import pytest
import torch

from avsr_amd import ops
from oracle import decode_oracle as DO
from tests import decode_ref as R

pytestmark = pytest.mark.gpu

LOGZERO = R.LOGZERO
INF = float("inf")


def _i32(x, dev):
    return torch.as_tensor(np.asarray(x), dtype=torch.int32).to(dev)


def _f32(x, dev):
    return torch.as_tensor(np.asarray(x), dtype=torch.float32).to(dev)


# ============================================================================ 1. ctc_prefix
V_CTC, N_CTC = 300, 3
CTC_SHAPES = [(244, 64), (245, 64), (40, 4)]     # LDS kernel at 65392 B, fallback at 65660 B, small


def _ctc_inputs(T, P, first, seed, n=N_CTC, U=1):
    """logp (U, T, V), previous tokens, states, ids with a repeated label, eos and blank among them"""
    g = torch.Generator().manual_seed(seed)
    V, eos = V_CTC, V_CTC - 1
    logp = torch.log_softmax(torch.randn(U, T, V, generator=g) * 3, -1)
    if first:
        yseqs = [[eos] for _ in range(n)]
        states = [None] * n
    else:
        yseqs = [[eos, 5 + h, 7] for h in range(n)]
        states = [(torch.log_softmax(torch.randn(T, 2, generator=g), -1) - 3.0, -2.5 - 0.25 * h) for h in range(n)]
    ids = torch.stack([torch.randperm(V - 22, generator=g)[:P] + 20 for _ in range(n)])   # (20 .. V-3: none planted)
    ids[1 % n, 0] = yseqs[1 % n][-1]  # repeated-label path
    ids[2 % n, 1] = eos
    ids[0, 2] = 0                     # blank among the scored ids
    return logp, yseqs, states, ids, eos


def _ctc_oracle(logp, yseqs, states, ids, eos, dtype=torch.float64):
    st = [None if s is None else (s[0].to(dtype), s[1]) for s in states]
    _, r, psi = DO.ctc_prefix_scores(logp.to(dtype), yseqs, st, ids, 0, eos)
    return psi, r.permute(2, 3, 0, 1)            # psi (n, V), r (n, P, T, 2)


def _ctc_launch(dev, logp, yseqs, states, ids, eos, out_len=None, **kw):
    n, P = ids.shape
    T = logp.shape[-2]
    first = states[0] is None
    r_prev = None if first else torch.stack([s[0] for s in states]).to(dev).contiguous()
    last = _i32([y[-1] for y in yseqs], dev)
    r_new = torch.full((n, P, T, 2), float("nan"), device=dev)
    psi = torch.full((n, P + 1), float("nan"), device=dev)
    ops.ctc_prefix(logp.to(dev).contiguous(), r_prev, last, ids.to(dev, torch.int32).contiguous(), r_new, psi, n=n,
                   out_len=len(yseqs[0]) - 1 if out_len is None else out_len, blank=0, eos=eos, **kw)
    return psi.cpu(), r_new.cpu()


def _ctc_check(psi, r_new, ids, eos, ref_psi, ref_r, ref32_psi, ref32_r, T=None):
    """the existing test's tolerance (psi 1e-5 |want| + 1e-4; r rtol 1e-5, atol 1e-4 above -1e9),
    or three times the error of the same oracle evaluated in fp32 where that is larger. Returns
    (kernel psi error, fp32-oracle psi error, kernel r error, fp32-oracle r error, the largest
    kernel error as a share of the existing test's tolerance)."""
    n, P = ids.shape
    T = ref_r.shape[2] if T is None else T
    want = torch.cat([ref_psi.gather(1, ids), ref_psi[:, eos:eos + 1]], 1)
    w32 = torch.cat([ref32_psi.gather(1, ids), ref32_psi[:, eos:eos + 1]], 1).double()
    e32 = float((w32 - want).abs().max())
    err = (psi.double() - want).abs()
    tol = torch.clamp(1e-5 * want.abs() + 1e-4, min=3 * e32)
    share = float((err / (1e-5 * want.abs() + 1e-4)).max())
    assert bool((err <= tol).all()), ("psi", float(err.max()), e32)
    rr, ok = ref_r[:, :, :T], ref_r[:, :, :T] > -1e9
    e32r = float((ref32_r[:, :, :T].double() - rr)[ok].abs().max())
    errr = (r_new[:, :, :T].double() - rr)[ok].abs()
    tolr = torch.clamp(1e-5 * rr[ok].abs() + 1e-4, min=3 * e32r)
    assert bool((errr <= tolr).all()), ("r_new", float(errr.max()), e32r)
    share = max(share, float((errr / (1e-5 * rr[ok].abs() + 1e-4)).max()))
    return float(err.max()), e32, float(errr.max()), e32r, share


@pytest.mark.parametrize("first", [True, False])
@pytest.mark.parametrize("T,P", CTC_SHAPES)
def test_ctc_prefix_both_kernels_match_oracle(dev, T, P, first):
    """avsr_ctc_prefix at the LDS kernel's last size (T * (P + 3) * 4 = 65392 B), the fallback
    kernel's first (65660 B) and a small one, first and later step, against the oracle's fp64
    CTCPrefixScoreTH restatement.
    Measured on an MI355X, largest |kernel - fp64| with the same oracle evaluated in fp32 on the
    CPU (e32) in brackets:
      (244, 64) LDS       first step psi 5.9e-4 (1.0e-4), r 1.7e-3 (1.5e-3); later psi 3.4e-7 (3.8e-7), r 3.4e-6 (3.8e-6)
      (245, 64) fallback  first step psi 5.8e-4 (8.9e-5), r 1.7e-3 (1.6e-3); later psi 9.2e-7 (3.7e-7), r 3.3e-6 (3.3e-6)
      (40, 4)   LDS       first step psi 9.5e-7 (9.5e-7), r 8.5e-5 (5.6e-5); later psi 2.8e-7 (2.8e-7), r 2.8e-6 (2.8e-6)
    The first-step values reach -2.3e3 (the eos score: 244 frames of blank log-probs, one fp32
    ulp 2.4e-4), so these are a few ulp and inside the existing tolerance (at most 0.08 of it); the fp32-oracle
    allowance is there for inputs where they would not be."""
    logp, yseqs, states, ids, eos = _ctc_inputs(T, P, first, seed=5)
    ref_psi, ref_r = _ctc_oracle(logp[0], yseqs, states, ids, eos)
    r32_psi, r32_r = _ctc_oracle(logp[0], yseqs, states, ids, eos, torch.float32)
    psi, r_new = _ctc_launch(dev, logp[0], yseqs, states, ids, eos)
    figs = _ctc_check(psi, r_new, ids, eos, ref_psi, ref_r, r32_psi, r32_r)
    print(f"ctc_prefix T={T} P={P} first={first}: psi err {figs[0]:.3g} (fp32 oracle {figs[1]:.3g}), "
          f"r err {figs[2]:.3g} (fp32 oracle {figs[3]:.3g}), {figs[4]:.2f} of the project tolerance")


@pytest.mark.parametrize("first", [True, False])
@pytest.mark.parametrize("T,P", CTC_SHAPES)
def test_ctc_prefix_batched_rows_match_their_utterance(dev, T, P, first):
    """U = 3 utterances in one (U, T, V) buffer, tlen = [T, 100, 17], hypotheses routed by uidx:
    every row equals the oracle on its own utterance truncated to tlen (out_len 0 or 2 < tlen);
    out_len read from the device (with a wrong host value) gives the same bits"""
    U = 3
    tlen = [T, min(100, T), 17]
    uidx = [0, 1, 2, 1, 0]
    n = len(uidx)
    logp, yseqs, states, ids, eos = _ctc_inputs(T, P, first, seed=7, n=n, U=U)
    kw = dict(uidx=_i32(uidx, dev), tlen=_i32(tlen, dev))
    psi, r_new = _ctc_launch(dev, logp, yseqs, states, ids, eos, **kw)
    for h in range(n):
        Tu = tlen[uidx[h]]
        lp = logp[uidx[h], :Tu]
        st = [None if states[h] is None else (states[h][0][:Tu], states[h][1])]
        ref_psi, ref_r = _ctc_oracle(lp, yseqs[h:h + 1], st, ids[h:h + 1], eos)
        r32_psi, r32_r = _ctc_oracle(lp, yseqs[h:h + 1], st, ids[h:h + 1], eos, torch.float32)
        _ctc_check(psi[h:h + 1], r_new[h:h + 1], ids[h:h + 1], eos, ref_psi, ref_r, r32_psi, r32_r, T=Tu)
    true_len = len(yseqs[0]) - 1
    psi_d, r_d = _ctc_launch(dev, logp, yseqs, states, ids, eos, out_len=5 - true_len,
                             out_len_dev=_i32([true_len], dev), **kw)
    for h in range(n):
        Tu = tlen[uidx[h]]
        assert torch.equal(psi_d[h], psi[h]) and torch.equal(r_d[h, :, :Tu], r_new[h, :, :Tu])


@pytest.mark.parametrize("first", [True, False])
@pytest.mark.parametrize("T", [244, 245])
def test_ctc_prefix_independent_of_the_other_ids(dev, T, first):
    """permuting the ids of a launch permutes psi and r_new bit for bit (the full-vocabulary
    scoring of ctc_weight = 1 relies on it), on both kernels"""
    P = 64
    logp, yseqs, states, ids, eos = _ctc_inputs(T, P, first, seed=9)
    psi, r_new = _ctc_launch(dev, logp[0], yseqs, states, ids, eos)
    perm = torch.randperm(P, generator=torch.Generator().manual_seed(T))
    assert not torch.equal(perm, torch.arange(P))
    psi_p, r_p = _ctc_launch(dev, logp[0], yseqs, states, ids[:, perm], eos)
    assert torch.equal(psi_p[:, :P], psi[:, perm]) and torch.equal(psi_p[:, P], psi[:, P])
    assert torch.equal(r_p, r_new[:, perm])


# ============================================================================ 2. beam_select
def _quant(g, shape, lo, hi):
    """multiples of 1/4 in [lo, hi): every product with 0 / 0.5 / 1 and every sum is exact in fp32"""
    return (torch.randint(int(lo * 4), int(hi * 4), shape, generator=g).float() / 4).numpy()


def _select_inputs(seed, n, V, P, dead=(), eos_in_ids=(), blank_in_ids=(), spread=2.0):
    g = torch.Generator().manual_seed(seed)
    eos = V - 1
    dec = _quant(g, (n, V), -spread, 0.25)
    ids = np.stack([(torch.randperm(V - 2, generator=g)[:P] + 1).numpy() for _ in range(n)]).astype(np.int32)
    for h in eos_in_ids:
        ids[h, (h + 1) % P] = eos
    for h in blank_in_ids:
        ids[h, h % P] = 0
    psi = _quant(g, (n, P + 1), -spread - 1, 0.0)
    s_prev = _quant(g, (n,), -3, 0.0)
    score = _quant(g, (n,), -3, 0.0)
    for h in dead:
        score[h] = -INF
    return dict(dec=dec, ids=ids, psi=psi, s_prev=s_prev, score=score, eos=eos, V=V, P=P, n=n)


def _select_launch(dev, c, beam, w_dec, w_ctc, seg=None, rows=None):
    lo, hi = (0, c["n"]) if rows is None else rows
    nseg = 1 if seg is None else len(seg) - 1
    out = {**{k: torch.full((nseg * beam,), -77, dtype=torch.int32, device=dev) for k in ("prev", "tok", "col")},
           **{k: torch.full((nseg * beam,), float("nan"), device=dev) for k in ("score", "dec", "ctc", "s")}}
    dec = torch.zeros(hi - lo, c["V"] + 3)           # ld > V
    dec[:, :c["V"]] = torch.from_numpy(c["dec"][lo:hi])
    ops.beam_select(dec.to(dev), c["V"], _i32(c["ids"][lo:hi], dev), _f32(c["psi"][lo:hi], dev),
                    _f32(c["s_prev"][lo:hi], dev), _f32(c["score"][lo:hi], dev), out, n=hi - lo, beam=beam, blank=0,
                    eos=c["eos"], w_dec=w_dec, w_ctc=w_ctc, seg=None if seg is None else _i32(seg, dev))
    return {k: v.cpu().tolist() for k, v in out.items()}


def _select_ref(c, beam, w_dec, w_ctc, seg=None):
    return R.beam_select_ref(c["dec"], c["ids"], c["psi"], c["s_prev"], c["score"], beam=beam, blank=0, eos=c["eos"],
                             w_dec=w_dec, w_ctc=w_ctc, seg=seg)


def _assert_select_equal(got, want):
    for k in ("prev", "tok", "col", "score", "dec", "ctc", "s"):
        assert got[k] == want[k], (k, got[k], want[k])


WEIGHTS = [(0.5, 0.5), (1.0, 0.0), (0.0, 1.0)]


@pytest.mark.parametrize("w_dec,w_ctc", WEIGHTS)
@pytest.mark.parametrize("beam", [1, 3, 5, 10, 16])
def test_beam_select_matches_full_matrix(dev, beam, w_dec, w_ctc):
    """all seven outputs equal the top `beam` of the full weighted matrix (value descending, flat
    index ascending) on quantised inputs with many exact ties: the candidate-only fast path
    (beams 1-10, nrow * (P + 1) <= 256), the full rows x V scan (beam 16: 16 * 25 > 256; w_ctc = 0
    always, psi zeroed as the search does), w_dec = 0, eos inside and outside the pre-beam ids"""
    P, ties = int(1.5 * beam), 0
    for V in (50, 5049) if beam in (3, 16) else (50,):
        for seed, spread in ((beam, 2.0), (beam + 100, 0.5)):     # the narrow spread: ties everywhere
            c = _select_inputs(seed, beam, V, P, eos_in_ids=range(0, beam, 2), spread=spread)
            if beam >= 3:                        # rows 0 and 1 alike: each of their entries ties across the rows
                for k in ("dec", "ids", "psi", "s_prev", "score"):
                    c[k][1] = c[k][0]
            if w_ctc == 0.0:
                c["psi"][:] = 0.0
            got, want = _select_launch(dev, c, beam, w_dec, w_ctc), _select_ref(c, beam, w_dec, w_ctc)
            _assert_select_equal(got, want)
            ties += len(set(want["score"])) < beam
    assert beam < 3 or ties > 0                  # the cases do hold ties among the selected


@pytest.mark.parametrize("w_dec,w_ctc", WEIGHTS)
@pytest.mark.parametrize("beam", [1, 3, 5])
def test_beam_select_first_step_and_unscored_pick(dev, beam, w_dec, w_ctc):
    """first-step geometry (one live row, the rest dead: the dead rows are never picked), and at
    w_ctc = 0 a row whose best token is outside its ids: col = P - 1, out_s = LOGZERO"""
    P, V = int(1.5 * beam), 50
    c = _select_inputs(40 + beam, beam, V, P, dead=range(1, beam))
    if w_ctc == 0.0:
        c["psi"][:] = 0.0
        c["dec"][0, 7] = 0.5                     # the single best token ...
        c["ids"][0][c["ids"][0] == 7] = 8        # ... is not among the ids
        if (c["ids"][0] == 8).sum() > 1:
            c["ids"][0][np.nonzero(c["ids"][0] == 8)[0][1:]] = 9
    got, want = _select_launch(dev, c, beam, w_dec, w_ctc), _select_ref(c, beam, w_dec, w_ctc)
    _assert_select_equal(got, want)
    assert set(got["prev"]) == {0}
    if w_ctc == 0.0:
        assert got["tok"][0] == 7 and got["col"][0] == P - 1 and got["s"][0] == np.float32(LOGZERO)


def test_beam_select_blank_in_prebeam_takes_full_scan(dev):
    """one live row, P = 2, ids = (blank, a), beam 3: only a and eos are finite candidates, the
    blank's LOGZERO entry fails the bound check and the third pick comes from the full scan, where
    every unscored token rounds to the same fp32 score (w_ctc * LOGZERO absorbs the rest): the two
    finite picks are exact, of the third the score and its consistency with its own (row, token)"""
    beam, P, V = 3, 2, 50
    c = _select_inputs(77, 1, V, P, blank_in_ids=[0])
    got, want = _select_launch(dev, c, beam, 0.5, 0.5), _select_ref(c, beam, 0.5, 0.5)
    assert sorted(got["score"]) == sorted(want["score"])
    for k in ("prev", "tok", "col", "score", "dec", "ctc", "s"):
        assert got[k][:2] == want[k][:2], k
    assert set(got["tok"][:2]) == {int(c["ids"][0, 1]), c["eos"]}
    tok = got["tok"][2]
    assert got["prev"][2] == 0 and tok not in got["tok"][:2] and 0 <= tok < V
    assert got["score"][2] == float(np.float32(0.5) * np.float32(LOGZERO))
    hit = np.nonzero(c["ids"][0] == tok)[0]
    assert got["col"][2] == (int(hit[0]) if len(hit) else P - 1)
    assert got["dec"][2] == float(c["dec"][0, tok]) and got["s"][2] == float(np.float32(LOGZERO))
    assert got["ctc"][2] == float(np.float32(LOGZERO) - np.float32(c["s_prev"][0]))


@pytest.mark.parametrize("w_dec,w_ctc", WEIGHTS)
def test_beam_select_segments(dev, w_dec, w_ctc):
    """nseg = 3: a full segment, an all-dead one (the documented filler: out_prev = seg[u],
    tok = eos, col = P - 1, score = -inf, zeros) and a single live row; every segment equals the
    reference and, bit for bit, a launch over its rows alone with out_prev offset by seg[u]"""
    beam, P, V = 3, 4, 50
    seg = [0, 3, 6, 7]
    c = _select_inputs(91, 7, V, P, dead=(1, 3, 4, 5), eos_in_ids=(0, 6), spread=0.5)
    if w_ctc == 0.0:
        c["psi"][:] = 0.0
    got, want = _select_launch(dev, c, beam, w_dec, w_ctc, seg=seg), _select_ref(c, beam, w_dec, w_ctc, seg=seg)
    _assert_select_equal(got, want)
    assert got["prev"][3:6] == [3, 3, 3] and got["tok"][3:6] == [c["eos"]] * 3 and got["col"][3:6] == [P - 1] * 3
    assert got["score"][3:6] == [-INF] * 3 and got["dec"][3:6] == got["ctc"][3:6] == got["s"][3:6] == [0.0] * 3
    for u in range(3):
        alone = _select_launch(dev, c, beam, w_dec, w_ctc, rows=(seg[u], seg[u + 1]))
        alone["prev"] = [p + seg[u] for p in alone["prev"]]
        for k in alone:
            assert got[k][u * beam:(u + 1) * beam] == alone[k], (u, k)


# ============================================================================ 3. beam_post
def _post_script(U, beam, maxlen, eos, steps, seed, P, V=40):
    """scripted selections [steps] of dicts prev/tok/col/score/dec/ctc/s [R]. Utterances by
    u % 3: 0 runs to its maxlen (one row's token is already eos at the forced step), 1 keeps one
    early eos far above three later ones at consecutive lengths (end detection at step 6 when
    maxlen allows), 2 picks eos on every row at step 3 (no live row left)."""
    g = torch.Generator().manual_seed(seed)
    R_ = U * beam
    f = lambda t: [float(x) for x in t.float()]
    out = []
    for i in range(steps):
        prev = torch.arange(R_) // beam * beam + torch.randint(0, beam, (R_,), generator=g)
        tok = torch.randint(1, V - 1, (R_,), generator=g)
        score = -(3.0 * i + 0.25 * (torch.arange(R_) % beam)) - torch.rand(R_, generator=g).float()
        for u in range(U):
            r0, kind = u * beam, u % 3
            if kind == 0 and i == maxlen[u] - 1:
                tok[r0] = eos
            if kind == 1 and beam > 1:
                if i == 1:
                    tok[r0 + 1], score[r0 + 1] = eos, -1.0
                if i in (2, 3, 4):
                    tok[r0 + beam - 1], score[r0 + beam - 1] = eos, -12.0 - i
            if kind == 2 and i == 3:
                tok[r0:r0 + beam] = eos
        out.append(dict(prev=prev.tolist(), tok=tok.tolist(), col=torch.randint(0, P, (R_,), generator=g).tolist(),
                        score=f(score), dec=f(-torch.rand(R_, generator=g) * 5), ctc=f(-torch.rand(R_, generator=g) * 9),
                        s=f(-torch.rand(R_, generator=g) * 30)))
    return out


def _post_state(dev, U, beam, steps, sos):
    R_, Lmax = U * beam, steps + 1
    i32, f32, f64 = (dict(device=dev, dtype=t) for t in (torch.int32, torch.float32, torch.float64))
    score0 = torch.full((R_,), -INF)
    score0[::beam] = 0.0
    return dict(pos=torch.zeros(1, **i32), tok=torch.full((R_,), sos, **i32), score=score0.to(dev),
                sdec=torch.zeros(R_, **f64), sctc=torch.zeros(R_, **f64), s_prev=torch.zeros(R_, **f32),
                src=torch.zeros(2 * R_, **i32), bp_prev=torch.zeros(steps, R_, **i32), bp_tok=torch.zeros(steps, R_, **i32),
                end_flag=torch.zeros(steps, R_, **i32), end_score=torch.zeros(steps, R_, **f32),
                end_dec=torch.zeros(steps, R_, **f64), end_ctc=torch.zeros(steps, R_, **f64),
                best_len=torch.full((U, Lmax + 3), -INF, **f32), best_end=torch.full((U,), -INF, **f32),
                done=torch.zeros(U + 1, **i32))


@pytest.mark.parametrize("end_detect", [1, 0])
@pytest.mark.parametrize("U,beam,maxlen", [(3, 3, [3, 9, 6]), (90, 3, None), (300, 1, None)])
def test_beam_post_follows_the_scripted_search(dev, U, beam, maxlen, end_detect):
    """avsr_beam_post over 9 scripted steps against BeamPostRef, every output after every step
    (the double sums with ==): an eos pick, the forced end at maxlen - 1 (also on a row whose token
    is eos), an utterance with no live row left, rows that stay dead after done, end detection at
    three consecutive lengths 10 below the best (not with end_detect = 0); R = 270 and U = 300 run
    the strided loops past the 256 threads"""
    steps, P, eos = 9, 4, 39
    if maxlen is None:
        maxlen = [(3, 9, 6, 9, 9, 5)[u % 6] for u in range(U)]
    script = _post_script(U, beam, maxlen, eos, steps, seed=U + beam, P=P)
    ref = R.BeamPostRef(U, beam, P, maxlen, eos, eos, end_detect, steps)
    st = _post_state(dev, U, beam, steps, eos)
    ml = _i32(maxlen, dev)
    done_at = [None] * U
    for i in range(steps):
        sel = script[i]
        ref.step(sel)
        ops.beam_post(U=U, beam=beam, P=P, R=U * beam, Lmax=steps + 1, steps_cap=steps, eos=eos, end_detect=end_detect,
                      d_end=R.D_END, maxlen=ml, sel_prev=_i32(sel["prev"], dev), sel_tok=_i32(sel["tok"], dev),
                      sel_col=_i32(sel["col"], dev), sel_score=_f32(sel["score"], dev), sel_dec=_f32(sel["dec"], dev),
                      sel_ctc=_f32(sel["ctc"], dev), sel_s=_f32(sel["s"], dev), **st)
        for k in ("tok", "score", "sdec", "sctc", "s_prev", "src", "bp_prev", "bp_tok", "end_flag", "end_score",
                  "end_dec", "end_ctc", "best_len", "best_end", "done"):
            assert st[k].cpu().tolist() == getattr(ref, k), (i, k)
        assert int(st["pos"].item()) == ref.pos == i + 1
        done_at = [i if d and done_at[u] is None else done_at[u] for u, (d, _) in enumerate(zip(ref.done, done_at))]
    if beam > 1:
        want = {"eos", "forced", "forced_on_eos", "no_live_row", "dead_after_done"} | ({"end_detect"} if end_detect else set())
        assert ref.events == want, ref.events
        # maxlen 3 ends at its forced step 2; end detection stops utterance 1 at step 6, without it
        # the utterance runs to its forced end at step 8; utterance 2 has no live row after step 3
        assert done_at[:3] == [2, 6 if end_detect else 8, 3]


# ============================================================================ 4. dec_attn
H_ATT, D_ATT = 2, 128


def _store(x, bf16):
    return x.bfloat16() if bf16 else x


def _attn_rows_check(o, q, rows_k, rows_v, bf16):
    """o[i] against the fp64 attention of the stored q[i] over its (L_i, D) key / value rows"""
    for i in range(o.shape[0]):
        ref = R.attn_ref(q[i].cpu(), rows_k[i].cpu(), rows_v[i].cpu(), H_ATT)
        ok, over = R.attn_close(o[i], ref, bf16)
        assert ok, (i, over)


@pytest.mark.parametrize("bf16", [False, True])
def test_dec_attn_kmap(dev, bf16):
    """the ancestry-indexed self-attention cache: key j of hypothesis i is cache row kmap[i][j],
    rows repeated and out of order, klen 1 .. 300 (two outer iterations of 256 keys),
    ldmap > klen_max; entries past klen[i] are other valid rows and must not count"""
    g = torch.Generator().manual_seed(21)
    n, rows, klen, ldmap = 6, 400, [1, 2, 7, 33, 40, 300], 320
    q = _store(torch.randn(n, 3 * D_ATT, generator=g), bf16).to(dev)
    kc = _store(torch.randn(rows, D_ATT, generator=g), bf16).to(dev)
    vc = _store(torch.randn(rows, D_ATT, generator=g), bf16).to(dev)
    kmap = torch.randint(0, rows, (n, ldmap), generator=g, dtype=torch.int32)
    kmap[4, :40] = kmap[4, :20].repeat(2)                       # repeated rows
    kmap[5, :300] = torch.arange(299, -1, -1, dtype=torch.int32)    # descending
    o = torch.full((n, D_ATT), float("nan"), device=dev, dtype=q.dtype)
    ops.dec_attn(q[:, :D_ATT], kc, vc, o, n=n, H=H_ATT, klen_max=300, k_bstride=0, v_bstride=0, klen=_i32(klen, dev),
                 kmap=kmap.to(dev))
    idx = [kmap[i, :klen[i]].long() for i in range(n)]
    _attn_rows_check(o, q[:, :D_ATT], [kc.cpu()[j] for j in idx], [vc.cpu()[j] for j in idx], bf16)


@pytest.mark.parametrize("bf16", [False, True])
def test_dec_attn_kmap_on_a_cache_built_by_the_step_kernels(dev, bf16):
    """beam_step_prep + beam_kv_put over 5 positions with a reorder of the ancestry after each
    (as the search does), then self-attention through the table: equals fp64 attention over the
    K / V rows of each hypothesis's own history"""
    g = torch.Generator().manual_seed(22)
    R_, Lmax, steps, D = 6, 8, 5, D_ATT
    ld = 3 * D + 8
    dt = torch.bfloat16 if bf16 else torch.float32
    ck = torch.zeros(Lmax * R_, D, device=dev, dtype=dt)
    cv = torch.zeros(Lmax * R_, D, device=dev, dtype=dt)
    anc = torch.zeros(R_, Lmax, dtype=torch.int32, device=dev)
    klen = torch.zeros(R_, dtype=torch.int32, device=dev)
    pos = torch.zeros(1, dtype=torch.int32, device=dev)
    hist = [[] for _ in range(R_)]                    # per row: (K row, V row) of its ancestors
    for i in range(steps):
        pos.fill_(i)
        ops.beam_step_prep(R_, pos, anc, klen)
        qkv = _store(torch.randn(R_, ld, generator=g), bf16).to(dev)
        ops.beam_kv_put(qkv, ck, cv, pos, R_, D)
        for r in range(R_):
            hist[r].append((qkv[r, D:2 * D].cpu(), qkv[r, 2 * D:3 * D].cpu()))
        o = torch.full((R_, D), float("nan"), device=dev, dtype=dt)
        ops.dec_attn(qkv[:, :D], ck, cv, o, n=R_, H=H_ATT, klen_max=Lmax, k_bstride=0, v_bstride=0, klen=klen, kmap=anc)
        assert klen.cpu().tolist() == [i + 1] * R_
        _attn_rows_check(o, qkv[:, :D], [torch.stack([k for k, _ in hist[r]]) for r in range(R_)],
                         [torch.stack([v for _, v in hist[r]]) for r in range(R_)], bf16)
        src = torch.randint(0, R_, (R_,), generator=g)            # the beam reorder (non-monotonic, repeats)
        anc = anc[src.to(dev)].contiguous()
        hist = [list(hist[s]) for s in src.tolist()]


@pytest.mark.parametrize("bf16", [False, True])
@pytest.mark.parametrize("n,group", [(7, 3), (7, 2), (7, 8)])
def test_dec_attn_partial_last_group(dev, n, group, bf16):
    """n % group != 0: the last workgroup holds fewer than `group` queries; direct, kidx and
    grouped launches in fp32 and bf16 storage against fp64 (grouped = ungrouped bit for bit)"""
    g = torch.Generator().manual_seed(23 + group)
    U, T = (n + group - 1) // group, 45
    lens = [45, 20, 5, 33][:U]
    mem = _store(torch.randn(U * T, 2 * D_ATT, generator=g), bf16).to(dev)
    q = _store(torch.randn(n, D_ATT, generator=g), bf16).to(dev)
    uidx = [i // group for i in range(n)]
    klen = [lens[u] for u in uidx]
    outs = []
    for grp in (1, group):
        o = torch.full((n, D_ATT), float("nan"), device=dev, dtype=q.dtype)
        ops.dec_attn(q, mem[:, :D_ATT], mem[:, D_ATT:], o, n=n, H=H_ATT, klen_max=T, k_bstride=T * mem.stride(0),
                     v_bstride=T * mem.stride(0), kidx=_i32(uidx, dev), klen=_i32(klen, dev), group=grp)
        outs.append(o)
    assert torch.equal(outs[0], outs[1])
    mc = mem.cpu()
    _attn_rows_check(outs[1], q, [mc[u * T:u * T + lens[u], :D_ATT] for u in uidx],
                     [mc[u * T:u * T + lens[u], D_ATT:] for u in uidx], bf16)
    # direct: hypothesis i reads key block i (no kidx), one block per hypothesis
    kd = _store(torch.randn(n, T, D_ATT, generator=g), bf16).to(dev)
    vd = _store(torch.randn(n, T, D_ATT, generator=g), bf16).to(dev)
    o = torch.full((n, D_ATT), float("nan"), device=dev, dtype=q.dtype)
    ops.dec_attn(q, kd, vd, o, n=n, H=H_ATT, klen_max=T, k_bstride=T * D_ATT, v_bstride=T * D_ATT, klen=_i32(klen, dev))
    _attn_rows_check(o, q, [kd[i, :klen[i]] for i in range(n)], [vd[i, :klen[i]] for i in range(n)], bf16)


@pytest.mark.parametrize("bf16", [False, True])
@pytest.mark.parametrize("ksplit", [2, 3])
def test_dec_attn_ksplit_boundaries(dev, ksplit, bf16):
    """key split at klen 192 / 193 / 384 / 385 / 577 (1, 2, 2, 3, 4 chunks of at most 192 keys,
    capped at ksplit): equals fp64, leaves the arrival counters zero, and a second launch on the
    same counters is bit-identical; ungrouped rows and groups of 2"""
    g = torch.Generator().manual_seed(29 + ksplit)
    lens = [192, 193, 384, 385, 577]
    T = 577
    mem = _store(torch.randn(T, 2 * D_ATT, generator=g), bf16).to(dev)
    cnt = ops._skinny_ws(dev)[ops.SKINNY_WS:].view(torch.int32)
    for group in (1, 2):
        klen = [ln for ln in lens for _ in range(group)]
        n = len(klen)
        q = _store(torch.randn(n, D_ATT, generator=g), bf16).to(dev)
        outs = []
        for _ in range(2):
            o = torch.full((n, D_ATT), float("nan"), device=dev, dtype=q.dtype)
            ops.dec_attn(q, mem[:, :D_ATT], mem[:, D_ATT:], o, n=n, H=H_ATT, klen_max=T, k_bstride=0, v_bstride=0,
                         klen=_i32(klen, dev), group=group, ksplit=ksplit)
            assert int(cnt.abs().sum()) == 0
            outs.append(o)
        assert torch.equal(outs[0], outs[1])
        mc = mem.cpu()
        _attn_rows_check(outs[0], q, [mc[:ln, :D_ATT] for ln in klen], [mc[:ln, D_ATT:] for ln in klen], bf16)


# ============================================================================ 5. top-k
TOPK_V = [17, 300, 5049, 6144, 6145]
TOPK_K = [1, 7, 15, 16]


def _topk_rows(V, seed):
    """rows with many exact ties, rows that are LOGZERO but for a few entries (ctc_weight = 1), rows
    with -inf entries, and a row with fewer finite entries than any K > 3"""
    g = torch.Generator().manual_seed(seed)
    x = torch.empty(7, V)
    x[0] = (torch.randn(V, generator=g) * 2).round() / 4
    x[1] = (torch.randn(V, generator=g)).round()
    x[2] = LOGZERO
    x[2, torch.randperm(V, generator=g)[:5]] = -torch.rand(5, generator=g) * 30
    x[3] = LOGZERO
    x[3, V - 1] = -1.0
    x[4] = (torch.randn(V, generator=g) * 2).round() / 4
    x[4, torch.randperm(V, generator=g)[:V // 2]] = -INF
    x[5] = -INF
    x[5, torch.randperm(V, generator=g)[:3]] = torch.tensor([0.5, 0.5, -2.0])
    x[6] = 0.25                                           # all equal: ids 0 .. K-1
    return x


@pytest.mark.parametrize("V", TOPK_V)
def test_row_topk_ties(dev, V):
    """avsr_row_topk against lexsort (value descending, index ascending) on tied rows, K = 1, 7,
    15, 16, V below 256, at 5049 and on both sides of 6144"""
    x = _topk_rows(V, V)
    xd = torch.full((x.shape[0], V + 5), 9.0e9)      # ldx > V: columns past V are larger and must not count
    xd[:, :V] = x
    xd = xd.to(dev)
    for K in TOPK_K:
        ids = torch.full((x.shape[0], K), -1, dtype=torch.int32, device=dev)
        ops.row_topk(xd, V, K, ids)
        assert np.array_equal(ids.cpu().numpy(), R.topk_ref(x.numpy(), K)), K


@pytest.mark.parametrize("bf16", [False, True])
@pytest.mark.parametrize("V", TOPK_V)
def test_log_softmax_topk_ties(dev, V, bf16):
    """avsr_log_softmax_topk (register kernel up to V = 6144, two passes at 6145) on fp32 and bf16
    logits: log-probs within 1e-5 of the fp64 log-softmax of the stored logits, ids equal to the
    lexsort of the kernel's own fp32 output"""
    x = _topk_rows(V, V + 1)
    x[x == LOGZERO] = -20.0                              # (logits: a constant floor, all ties)
    xs = _store(x, bf16)
    xd = torch.full((x.shape[0], V + 8), 50.0, dtype=xs.dtype)
    xd[:, :V] = xs
    xd = xd.to(dev)
    want = torch.log_softmax(xs.double(), -1)
    for K in TOPK_K:
        lp = torch.full((x.shape[0], V), float("nan"), device=dev)
        ids = torch.full((x.shape[0], K), -1, dtype=torch.int32, device=dev)
        ops.log_softmax_topk(xd, V, lp, K, ids)
        got = lp.cpu()
        fin = torch.isfinite(want)
        assert torch.equal(torch.isfinite(got), fin) and bool((got[~fin] == -INF).all())
        assert float((got.double()[fin] - want[fin]).abs().max()) <= 1e-5
        assert np.array_equal(ids.cpu().numpy(), R.topk_ref(got.numpy(), K)), K


# ============================================================================ 6. data movement
def test_gather_rows_paths(dev):
    """dst[g][i] = src[g][idx[i]] exactly: the 16-byte path, the 4-byte path (row_bytes = 4 * 37),
    groups = 3 with group strides, repeated indices; nothing outside the rows is written"""
    g = torch.Generator().manual_seed(31)
    idx = [4, 4, 0, 9, 2, 9, 9, 1]
    n = len(idx)
    idx_d = _i32(idx, dev)
    for cols, ld_s, ld_d in ((64, 64, 64), (64, 72, 68), (37, 37, 37), (37, 41, 39)):
        src = torch.randn(10, ld_s, generator=g).to(dev)
        dst = torch.full((n, ld_d), -5.0, device=dev)
        ops.gather_rows(src, dst, idx_d, groups=1, n=n, row_bytes=cols * 4, src_gstride=0, src_rstride=ld_s * 4,
                        dst_gstride=0, dst_rstride=ld_d * 4)
        want = torch.full((n, ld_d), -5.0, device=dev)
        want[:, :cols] = src[idx, :cols]
        assert torch.equal(dst, want), (cols, ld_s, ld_d)
    for cols in (64, 37):
        src = torch.randn(3, 12, cols, generator=g).to(dev)          # 10 rows used of 12 per group
        dst = torch.full((3, n + 2, cols), -5.0, device=dev)
        ops.gather_rows(src, dst, idx_d, groups=3, n=n, row_bytes=cols * 4, src_gstride=12 * cols * 4,
                        src_rstride=cols * 4, dst_gstride=(n + 2) * cols * 4, dst_rstride=cols * 4)
        want = torch.full((3, n + 2, cols), -5.0, device=dev)
        want[:, :n] = src[:, idx]
        assert torch.equal(dst, want), cols


@pytest.mark.parametrize("R_", [6, 300])
@pytest.mark.parametrize("p", [0, 5])
def test_beam_step_prep(dev, R_, p):
    """anc[r][pos] = pos * R + r, klen[r] = pos + 1, nothing else touched"""
    Lmax = 8
    anc = torch.full((R_, Lmax), -3, dtype=torch.int32, device=dev)
    klen = torch.full((R_,), -3, dtype=torch.int32, device=dev)
    ops.beam_step_prep(R_, _i32([p], dev), anc, klen)
    want = torch.full((R_, Lmax), -3, dtype=torch.int32)
    want[:, p] = p * R_ + torch.arange(R_, dtype=torch.int32)
    assert torch.equal(anc.cpu(), want) and klen.cpu().tolist() == [p + 1] * R_


@pytest.mark.parametrize("bf16", [False, True])
def test_beam_kv_put(dev, bf16):
    """cache rows pos * R + r take qkv[r][D:2D] / qkv[r][2D:3D] (ldqkv > 3D), the rest is untouched"""
    g = torch.Generator().manual_seed(33)
    R_, D, Lmax, p = 6, D_ATT, 4, 2
    qkv = _store(torch.randn(R_, 3 * D + 8, generator=g), bf16).to(dev)
    ck = torch.full((Lmax * R_, D), -5.0, device=dev, dtype=qkv.dtype)
    cv = torch.full((Lmax * R_, D), -6.0, device=dev, dtype=qkv.dtype)
    ops.beam_kv_put(qkv, ck, cv, _i32([p], dev), R_, D)
    wk, wv = torch.full_like(ck, -5.0), torch.full_like(cv, -6.0)
    wk[p * R_:(p + 1) * R_] = qkv[:, D:2 * D]
    wv[p * R_:(p + 1) * R_] = qkv[:, 2 * D:3 * D]
    assert torch.equal(ck, wk) and torch.equal(cv, wv)


@pytest.mark.parametrize("bf16", [False, True])
def test_embed_fwd_with_device_position(dev, bf16):
    """y[r] = table[tok[r]] * scale + pe[pe_row[0]] for every row: exactly on values whose product
    and sum are exact in the storage type (multiples of 1/4, scale 4), and in fp32 within one
    rounding of the fp64 result on random values"""
    g = torch.Generator().manual_seed(35)
    R_, V, D, L = 9, 40, D_ATT, 7
    tok = torch.randint(0, V, (R_,), generator=g)
    table = _store(torch.randint(-8, 9, (V, D), generator=g).float() / 4, bf16).to(dev)
    pe = (torch.randint(-8, 9, (L, D), generator=g).float() / 4).to(dev)
    for p in (0, 5):
        y = torch.full((R_, D), float("nan"), device=dev, dtype=table.dtype)
        ops.embed_fwd(_i32(tok, dev), table, pe, 4.0, y, 1, pe_row=_i32([p], dev))
        assert torch.equal(y, (table[tok.to(dev)].float() * 4.0 + pe[p]).to(table.dtype)), p
    if not bf16:
        table, pe = torch.randn(V, D, generator=g), torch.randn(L, D, generator=g)
        y = torch.full((R_, D), float("nan"), device=dev)
        ops.embed_fwd(_i32(tok, dev), table.to(dev), pe.to(dev), 11.3137, y, 1, pe_row=_i32([3], dev))
        prod = table[tok].double() * float(np.float32(11.3137))
        bound = (prod.abs() + pe[3].double().abs()) * 2.0 ** -23      # a rounding of the product and one of the sum
        assert bool(((y.cpu().double() - (prod + pe[3].double())).abs() <= bound).all())
