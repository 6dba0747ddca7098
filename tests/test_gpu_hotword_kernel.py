"""The hot-word step kernel (avsr_hotword_step) and avsr_beam_select with its bonus array alone,
with an LM column alone and with both (candidates pass and full scan), against the restatements in tests/hotword_ref.py: R = 7 rows, P = 4 pre-beam ids, C = 8
continuation columns, V = 12, beta = 0.75 (every bonus a multiple of 1/4: exact in fp32)."""
import numpy as np
import pytest
import torch

from avsr_amd import hotwords as HW
from avsr_amd import ops
from tests import decode_ref as R
from tests import hotword_ref as H

pytestmark = pytest.mark.gpu

V, EOS, P, BETA = 12, 11, 4, 0.75
PHRASES = H.SET_A + H.SET_B + H.SET_FAN
TRIE = H.Trie(PHRASES, EOS)
at = lambda *toks: TRIE.walk(list(toks))[1]                 # the node after walking toks from the root
# (node, pre-beam ids) per row
ROWS = [
    (0, [3, 4, 9, EOS]),                 # the root: a one-token phrase, a phrase start, a miss, eos
    (at(4), [5, 9, 3, 0]),               # mid-phrase: match, cancel, cancel + restart, blank
    (at(4, 5), [9, 10, 1, 2]),           # mid-phrase with two children, neither in the pre-beam
    (at(2, 3), [4, 9, 2, EOS]),          # a terminal node with a child: nothing pending
    (at(1), [10, 0, EOS, 1]),           # exactly 8 children: every continuation column used
    (at(6, 6), [6, 8, 1, 5]),            # its only child (8) is in the pre-beam: not added twice
    (at(4, 5), [6, 2, 7, 3]),            # both children in the pre-beam
]


def _i32(a, dev):
    return torch.as_tensor(np.asarray(a), dtype=torch.int32).to(dev).contiguous()


def _f32(a, dev):
    return torch.as_tensor(np.asarray(a), dtype=torch.float32).to(dev).contiguous()


def _tree(dev):
    t = HW.build_tree(PHRASES, eos=EOS)
    return {k: _i32(getattr(t, k), dev) for k in ("child_off", "child_tok", "child_node", "pend", "terminal")}


def _step_launch(dev):
    Rn = len(ROWS)
    ids = torch.full((Rn, P + H.C), -7, dtype=torch.int32, device=dev)
    bonus = torch.full((Rn, P + H.C + 1), float("nan"), device=dev)
    nxt = torch.full((Rn, P + H.C + 1), -7, dtype=torch.int32, device=dev)
    ops.hotword_step(_tree(dev), _i32([n for n, _ in ROWS], dev), _i32([p for _, p in ROWS], dev), ids, bonus, nxt,
                     beta=BETA, blank=0, eos=EOS)
    return ids.cpu().numpy(), bonus.cpu().numpy(), nxt.cpu().numpy()


def _step_ref():
    return H.hotword_step_ref(TRIE, [n for n, _ in ROWS], [p for _, p in ROWS], BETA)


def test_rows_are_what_they_claim():
    """(no kernel) the rows sit where the comments say, from the reference tree alone"""
    assert len(ROWS) == 7 and len({n for n, _ in ROWS}) == 6 and all(0 <= n < len(TRIE.kids) for n, _ in ROWS)
    assert TRIE.terminal[at(2, 3)] and TRIE.kids[at(2, 3)] and TRIE.pend(at(2, 3)) == 0
    assert len(TRIE.kids[at(1)]) == 8 and TRIE.pend(at(4, 5)) == 2 and TRIE.pend(at(6, 6)) == 2
    ids, bonus, nxt = _step_ref()
    assert (ids[0, P:] == 0).all()                               # the root offers no continuation
    assert ids[2, P:].tolist() == [6, 7] + [0] * 6
    assert ids[4, P:].tolist() == list(range(2, 10))
    assert ids[5, P:].tolist() == [0] * 8 and ids[6, P:].tolist() == [0] * 8      # the dedup path
    assert bonus.min() == -1.5 and bonus.max() == 0.75 and (bonus == 0.0).any()


def test_hotword_step_matches_reference(dev):
    """continuation ids, the bonus of every column and of eos (== numpy float32) and the successor
    nodes"""
    ids, bonus, nxt = _step_launch(dev)
    rids, rbonus, rnxt = _step_ref()
    assert ids.tolist() == rids.tolist()
    assert bonus.dtype == rbonus.dtype == np.float32 and (bonus == rbonus).all(), (bonus, rbonus)
    assert nxt.tolist() == rnxt.tolist()


def test_hotword_step_reads_an_unwritten_node_as_root(dev):
    """a node outside the tree (a buffer no step has written) is the root, not an index"""
    tree = _tree(dev)
    pre = _i32([ROWS[0][1]] * 2, dev)
    outs = []
    for nodes in ([0, 0], [len(TRIE.kids), -3]):
        ids = torch.zeros(2, P + H.C, dtype=torch.int32, device=dev)
        bonus, nxt = torch.zeros(2, P + H.C + 1, device=dev), torch.zeros(2, P + H.C + 1, dtype=torch.int32, device=dev)
        ops.hotword_step(tree, _i32(nodes, dev), pre, ids, bonus, nxt, beta=BETA, blank=0, eos=EOS)
        outs.append((ids.cpu(), bonus.cpu(), nxt.cpu()))
    assert all(torch.equal(a, b) for a, b in zip(*outs))


# ------------------------------------------------------------------------------ beam_select
def _quant(g, shape, lo, hi):
    """multiples of 1/4 in [lo, hi): every product with 0.5 and every sum is exact in fp32"""
    return (torch.randint(int(lo * 4), int(hi * 4), shape, generator=g).float() / 4).numpy()


def _select_inputs(seed, spread):
    g = torch.Generator().manual_seed(seed)
    ids, bonus, nxt = _step_ref()
    n, Pw = ids.shape
    score = _quant(g, (n,), -3, 0.0)
    score[4] = R.NEG_INF                                         # a dead row inside a segment
    return dict(dec=_quant(g, (n, V), -spread, 0.25), ids=ids, psi=_quant(g, (n, Pw + 1), -spread - 1, 0.0),
                s_prev=_quant(g, (n,), -3, 0.0), score=score, bonus=bonus, next=nxt)


def _select_launch(dev, c, beam, seg, with_bonus, with_lm=False, w_ctc=0.5, **fusion):
    nseg = len(seg) - 1
    out = {**{k: torch.full((nseg * beam,), -77, dtype=torch.int32, device=dev)
              for k in ("prev", "tok", "col", "next", "lm_next")},
           **{k: torch.full((nseg * beam,), float("nan"), device=dev)
              for k in ("score", "dec", "ctc", "s", "bonus", "lm")}}
    dec = torch.zeros(c["dec"].shape[0], V + 3)                  # ld > V
    dec[:, :V] = torch.from_numpy(c["dec"])
    kw = dict(bonus=_f32(c["bonus"], dev), nxt=_i32(c["next"], dev)) if with_bonus else {}
    if with_lm:
        kw.update(lm=_f32(c["lm"], dev), lm_next=_i32(c["lm_next"], dev))
    ops.beam_select(dec.to(dev), V, _i32(c["ids"], dev), _f32(c["psi"], dev), _f32(c["s_prev"], dev),
                    _f32(c["score"], dev), out, n=c["dec"].shape[0], beam=beam, blank=0, eos=EOS, w_dec=0.5, w_ctc=w_ctc,
                    seg=_i32(seg, dev), **kw, **fusion)
    return {k: v.cpu().tolist() for k, v in out.items()}


@pytest.mark.parametrize("beam", [3, 5])
@pytest.mark.parametrize("seed,spread", [(11, 2.0), (12, 0.5)])
def test_beam_select_with_bonus(dev, beam, seed, spread):
    """the kernel's own candidate layout (12 columns with blank padding, eos inside a pre-beam)
    through avsr_beam_select in three segments (one with a dead row, one of a single row): with the
    bonus all nine outputs equal the reference that adds it between the CTC term and the running
    score; without it the seven outputs equal decode_ref.beam_select_ref unchanged and the two new
    ones stay untouched. The narrow spread gives exact ties."""
    seg = [0, 3, 6, 7]
    c = _select_inputs(seed, spread)
    kw = dict(beam=beam, blank=0, eos=EOS, w_dec=0.5, w_ctc=0.5, seg=seg)
    want = H.beam_select_bonus_ref(c["dec"], c["ids"], c["psi"], c["s_prev"], c["score"], c["bonus"], c["next"], **kw)
    got = _select_launch(dev, c, beam, seg, True)
    for k in want:
        assert got[k] == want[k], (k, got[k], want[k])
    plain = R.beam_select_ref(c["dec"], c["ids"], c["psi"], c["s_prev"], c["score"], **kw)
    got0 = _select_launch(dev, c, beam, seg, False)
    for k in plain:
        assert got0[k] == plain[k], (k, got0[k], plain[k])
    assert got0["next"] == [-77] * (3 * beam) and all(np.isnan(v) for v in got0["bonus"])
    assert got0["lm_next"] == [-77] * (3 * beam) and all(np.isnan(v) for v in got0["lm"])
    assert want["tok"] != plain["tok"] or want["prev"] != plain["prev"]      # the bonus does change the pick


LM_SEED, LM_SPREAD = 11, 2.0


def _lm_inputs():
    """_select_inputs plus LM scores in [-4, 0] (multiples of 1/4) and arbitrary successors per column"""
    c = _select_inputs(LM_SEED, LM_SPREAD)
    g = torch.Generator().manual_seed(LM_SEED + 100)
    shape = c["bonus"].shape
    c["lm"] = _quant(g, shape, -4, 0.25)
    c["lm_next"] = torch.randint(0, 1000, shape, generator=g, dtype=torch.int32).numpy()
    return c


def test_lm_changes_the_reference_picks():
    """(no kernel) at the seed of the test below the reference picks with the LM differ from those
    without it, in every case and at both beams: a dropped LM term would show"""
    seg = [0, 3, 6, 7]
    c = _lm_inputs()
    assert c["lm"].min() >= -4.0 and c["lm"].max() <= 0.0 and c["lm_next"].min() >= 0
    for beam in (3, 5):
        for with_bonus, w_ctc in ((False, 0.5), (True, 0.5), (True, 0.0)):
            kw = dict(beam=beam, blank=0, eos=EOS, w_dec=0.5, w_ctc=w_ctc, seg=seg, w_len=0.25)
            b = (c["bonus"], c["next"]) if with_bonus else (None, None)
            on = H.beam_select_bonus_ref(c["dec"], c["ids"], c["psi"], c["s_prev"], c["score"], *b, lm=c["lm"],
                                         lm_next=c["lm_next"], w_lm=0.5, **kw)
            off = H.beam_select_bonus_ref(c["dec"], c["ids"], c["psi"], c["s_prev"], c["score"], *b, **kw)
            assert on["tok"] != off["tok"] or on["prev"] != off["prev"], (beam, with_bonus, w_ctc)


@pytest.mark.parametrize("beam", [3, 5])
@pytest.mark.parametrize("with_bonus,w_ctc", [(False, 0.5), (True, 0.5), (True, 0.0)],
                         ids=["lm", "bonus_lm", "bonus_lm_full_scan"])
def test_beam_select_with_lm(dev, beam, with_bonus, w_ctc):
    """avsr_beam_select with an n-gram LM column (w_lm = 0.5, lm_hi = 0) and a length bonus (w_len =
    0.25) over the layout of the test above: the LM alone, the bonus and the LM together, and both
    with w_ctc = 0, where the kernel scans every (row, token) from the start, tokens outside ids[h]
    included (LM term 0, successor -1, the eos column's bonus). All eleven outputs equal the
    reference that sums in the documented order (the LM alone leaves "bonus" / "next" untouched)."""
    seg = [0, 3, 6, 7]
    c = _lm_inputs()
    b = (c["bonus"], c["next"]) if with_bonus else (None, None)
    want = H.beam_select_bonus_ref(c["dec"], c["ids"], c["psi"], c["s_prev"], c["score"], *b, beam=beam, blank=0, eos=EOS,
                                   w_dec=0.5, w_ctc=w_ctc, seg=seg, lm=c["lm"], lm_next=c["lm_next"], w_lm=0.5, w_len=0.25)
    got = _select_launch(dev, c, beam, seg, with_bonus, True, w_ctc, w_lm=0.5, w_len=0.25, lm_hi=0.0)
    assert len(want) == (11 if with_bonus else 9)
    for k in want:
        assert got[k] == want[k], (k, got[k], want[k])
    if not with_bonus:
        assert got["next"] == [-77] * (3 * beam) and all(np.isnan(v) for v in got["bonus"])
