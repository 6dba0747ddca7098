"""The scripted searches of tests/decode_ref.py through a decode session: 4 utterances per batch
through 2 slots in eager steps with poll = 1, so two utterances enter a reused slot at whatever
step their predecessor ended. Per utterance the n-best equals the one-utterance search with ==
(tokens, totals, per-scorer scores as floats) and, for every case the fp64 reference does not
mark as skipped, matches that reference by the existing rule (tokens equal, scores within 1e-4
relative). The decoder is a table looked up at each row's own position (st["rowpos"])."""
import pytest
import torch

from avsr_amd import ops
from avsr_amd.decode import BatchBeamSearch
from tests import decode_ref as R

pytestmark = pytest.mark.gpu


class ScriptedStream(BatchBeamSearch):
    """BatchBeamSearch whose decoder is a table: row r of slot u at position i with last token t
    gets the logits table[u][i][t][:] through the real log-softmax + pre-beam kernel. An input of
    a session is (T, V + V*V): the CTC log-probs beside the flattened table rows of T steps."""

    def __init__(self, beam, w, V, dev):
        super().__init__(None, beam_size=beam, vocab_size=V, weights={"decoder": 1.0 - w, "ctc": w}, sos=V - 1,
                         eos=V - 1, pre_beam_score_key=None if w == 1.0 else "decoder")
        self.dev = dev

    def _decoder_step(self, eng, st):
        R_, V = st["R"], self.n_vocab
        pos = st["rowpos"] if "rowpos" in st else st["pos"].expand(R_)
        logits = st["table"][st["uidx"].long(), pos.long(), st["tok"].long()].contiguous()
        logp = torch.empty(R_, V, device=logits.device, dtype=torch.float32)
        return ops.log_softmax_topk(logits, V, logp, self.pre_beam_size, st["ids"])

    # the session's two engine hooks, without an engine
    def _session_buffers(self, S, max_frames):
        logp = torch.zeros(S, max_frames, self.n_vocab, device=self.dev)
        return None, self.dev, torch.float32, 64, 0, logp, None, None

    def _session_admit(self, sess, slot, x):
        st, V = sess.st, self.n_vocab
        if "table" not in st:
            st["table"] = torch.zeros(sess.S, st["Lmax"], V, V, device=self.dev)
        T = x.shape[0]
        st["logp"][slot, :T] = x[:, :V]
        st["table"][slot, :T] = x[:, V:].view(T, V, V)

    def run_batch(self, table, ctc_logp, Ts):
        """decode_batch without an engine (as tests/test_gpu_decode_scripted.py runs it): all
        utterances in one state with the shared position, eager steps until every one is done"""
        U = len(Ts)
        st = self._new_state(self.dev, torch.float32, Ts, Ts, ctc_logp, None, 64, 0, end_detect=1)
        st["table"] = table
        for i in range(st["steps"]):
            self._step(None, st, i == 0, i & 1)
            if int(st["done"][U].item()) == U:
                break
        return [[h.asdict() for h in nbest] for nbest in self._collect(st, [None] * U, 0.0, 0.0)]

    def run_alone(self, table, ctc_logp):
        """the one-utterance search (Tm = T, its own buffers), eager steps"""
        T = ctc_logp.shape[0]
        st = self._new_state(self.dev, torch.float32, [T], [T], ctc_logp[None].contiguous(), None, 64, 0, end_detect=1)
        st["table"] = table[None].contiguous()
        for i in range(st["steps"]):
            self._step(None, st, i == 0, i & 1)
            if int(st["done"][1].item()) == 1:
                break
        return [h.asdict() for h in self._collect(st, [None], 0.0, 0.0)[0]]


def _assert_matches_reference(got, want, w):
    """n-best token sequences equal in order; total and per-scorer scores within 1e-4 relative"""
    assert [h["yseq"] for h in got] == [h.yseq for h in want]
    keys = {k for k, use in (("decoder", w != 1.0), ("ctc", w != 0.0)) if use}
    for h, r in zip(got, want):
        assert abs(h["score"] - r.score) <= 1e-4 * abs(r.score), (h["score"], r.score)
        assert set(h["scores"]) == set(r.scores) == keys
        for k in keys:
            assert abs(h["scores"][k] - r.scores[k]) <= 1e-4 * abs(r.scores[k]), (k, h["scores"][k], r.scores[k])


_ALONE = {}


def _case(dev, batch):
    """the batch's inputs on the device, the reference, and the one-utterance searches (once)"""
    c, refs = R.scripted_reference(batch)
    bs = ScriptedStream(c["beam"], c["w"], c["V"], dev)
    tables = [c["table"][u, :T].to(dev).contiguous() for u, T in enumerate(c["Ts"])]
    ctcs = [c["ctc"][u, :T].to(dev).contiguous() for u, T in enumerate(c["Ts"])]
    if batch not in _ALONE:
        _ALONE[batch] = [bs.run_alone(t, l) for t, l in zip(tables, ctcs)]
    xs = [torch.cat([l, t.view(t.shape[0], -1)], 1) for t, l in zip(tables, ctcs)]
    return c, refs, bs, xs, _ALONE[batch]


def _stream(bs, xs, order, slots):
    with bs.stream(slots=slots, max_frames=max(x.shape[0] for x in xs), poll=1, graphs=False) as session:
        out = dict(session.run([xs[u] for u in order]))
        book, steps = session.book, session.replays
    assert sorted(out) == list(range(len(xs)))
    return {order[i]: [h.asdict() for h in n] for i, n in out.items()}, book, steps


@pytest.mark.parametrize("batch", R.SCRIPTED_BATCHES, ids=lambda b: f"s{b[0]}-b{b[1]}-w{b[2]:g}-{b[3]}")
def test_scripted_stream_through_two_slots(dev, batch):
    c, refs, bs, xs, alone = _case(dev, batch)
    # input order: the utterances whose reference fires end detection last, so that they are the
    # ones admitted into a reused slot (decided from the reference alone)
    order = sorted(range(c["U"]), key=lambda u: bool(refs[u][1]["end_detect"]))
    got, book, steps = _stream(bs, xs, order, slots=2)
    refilled = [order[i] for n, (i, s) in enumerate(book.admitted) if s in [t for _, t in book.admitted[:n]]]
    assert len(refilled) == 2
    # the second admissions happen while the other slot is mid-search
    assert steps < sum(refs[u][1]["steps"] for u in range(c["U"]))
    if batch[3] != "random" and c["w"] != 1.0:
        assert any(refs[u][1]["end_detect"] for u in refilled), "end detection must fire in a refilled slot"
    for u, (want, info, skipped) in enumerate(refs):
        assert got[u] == alone[u], u                  # tokens, total and per-scorer scores as floats
        if not skipped:
            _assert_matches_reference(got[u], want, c["w"])


@pytest.mark.parametrize("slots", [3, 4])
def test_scripted_stream_slot_counts(dev, slots):
    """batch 1006 through 3 slots (one refill) and 4 slots (none: decode_batch's situation), equal
    to the batched search's results too"""
    batch = next(b for b in R.SCRIPTED_BATCHES if b[0] == 1006)
    c, refs, bs, xs, alone = _case(dev, batch)
    got, book, _ = _stream(bs, xs, list(range(c["U"])), slots)
    assert len({s for _, s in book.admitted}) == slots and len(book.admitted) == 4
    batched = bs.run_batch(c["table"].to(dev).contiguous(), c["ctc"].to(dev).contiguous(), c["Ts"])
    for u, (want, info, skipped) in enumerate(refs):
        assert got[u] == alone[u], u
        assert got[u] == batched[u], u                # the batched search with the shared position
        if not skipped:
            _assert_matches_reference(got[u], want, c["w"])
