"""A decode session over a stream of utterances (decode.DecodeSession: fixed slots, refilled as
utterances end, every step a graph replay) returns, per utterance, exactly the hypotheses of the
one-utterance search `bs(x)`: tokens, total and per-scorer scores equal as floats. Tiny config,
fp32, the encoder outputs of tests/golden/avsr_tiny.npz."""
import pytest
import torch

from avsr_amd import decode, evaluate
from avsr_amd.avhubert_avsr_model import AVHubertAVSR, get_beam_search_decoder
from avsr_amd.configuration_avhubert_avsr import AVHubertAVSRConfig
from oracle.weights import NO_DROPOUT, TINY_CONFIG
from tests.oracle_util import golden_state, load_golden

pytestmark = pytest.mark.gpu

TOKENS = ["<blank>"] + [f"u{i}" for i in range(1, 5048)] + ["<eos>"]


@pytest.fixture(scope="module")
def g():
    return load_golden()


@pytest.fixture(scope="module")
def model(g):
    m = AVHubertAVSR(AVHubertAVSRConfig(**TINY_CONFIG, **NO_DROPOUT)).eval()
    m.load_state_dict({k: torch.from_numpy(v) for k, v in golden_state(g).items()}, strict=True)
    m.setup_engine("cuda", torch.float32)
    return m


@pytest.fixture(scope="module")
def xs(g):
    e0, e1 = g["dec_enc_0"], g["dec_enc_1"]
    return [torch.from_numpy(a).cuda() for a in (e0, e1, e0[:11], e1[3:17], e0[:5], e1)]


_WANT = {}


def _alone(model, xs, beam, w=0.1):
    """[bs(x) for x in xs] as plain values, computed once per (beam, ctc_weight)"""
    if (beam, w) not in _WANT:
        bs = get_beam_search_decoder(model.avsr, TOKENS, ctc_weight=w, beam_size=beam)
        _WANT[beam, w] = [_plain(bs(x)) for x in xs]
    return _WANT[beam, w]


def _plain(nbest):
    """tokens, score and per-scorer scores of an n-best list as Python values (floats compare with ==)"""
    return [h.asdict() for h in nbest]


@pytest.mark.parametrize("beam", [1, 3, 5])
def test_stream_equals_per_utterance(g, model, xs, beam):
    """six utterances of 25, 25, 11, 14, 5 and 25 frames through 2 slots (four refills, at steps
    that differ per slot), graph replays, the default poll"""
    bs = get_beam_search_decoder(model.avsr, TOKENS, ctc_weight=0.1, beam_size=beam)
    got = bs.decode_stream(xs, slots=2, max_frames=25)
    assert [_plain(n) for n in got] == _alone(model, xs, beam)
    assert all(len(n) > 0 for n in got)
    if beam in (1, 3):
        assert got[0][0].asdict()["yseq"] == g[f"yseq_b{beam}_0"].tolist()


@pytest.mark.parametrize("w", [0.0, 1.0])
def test_stream_with_one_scorer(model, xs, w):
    """the decoder alone (every token a candidate) and the CTC prefix scorer alone (full-vocabulary
    scoring in chunks, per-row prefix lengths in each)"""
    bs = get_beam_search_decoder(model.avsr, TOKENS, ctc_weight=w, beam_size=3)
    got = bs.decode_stream(xs, slots=2, max_frames=25)
    assert [_plain(n) for n in got] == _alone(model, xs, 3, w)


def test_stream_without_folded_layernorms(model, xs):
    """FOLD_LN off: LayerNorm, QKV linear and avsr_beam_kv_put with per-row positions"""
    old = decode.FOLD_LN
    decode.FOLD_LN = False
    try:
        bs = get_beam_search_decoder(model.avsr, TOKENS, ctc_weight=0.1, beam_size=3)
        got = bs.decode_stream(xs, slots=2, max_frames=25)
        want = [_plain(bs(x)) for x in xs]
    finally:
        decode.FOLD_LN = old
    assert [_plain(n) for n in got] == want


def test_session_runs_twice_around_a_batched_search(model, xs):
    """one session, two streams, a decode_batch (its own graphs on the same capture stream, the
    shared split-K counters and attention workspaces) in between; run() yields every index once"""
    bs = get_beam_search_decoder(model.avsr, TOKENS, ctc_weight=0.1, beam_size=3)
    want = _alone(model, xs, 3)
    with bs.stream(slots=2, max_frames=25) as session:
        first = list(session.run(xs))
        batch = bs.decode_batch(xs[:4])
        second = list(session.run(iter(xs)))
        steps = session.replays
    assert sorted(i for i, _ in first) == sorted(i for i, _ in second) == list(range(len(xs)))
    assert [_plain(n) for _, n in sorted(first, key=lambda p: p[0])] == want
    assert [_plain(n) for _, n in sorted(second, key=lambda p: p[0])] == want
    assert [_plain(n) for n in batch] == want[:4]
    # (2 slots: never more steps than the utterances' step limits one after another, plus the poll)
    assert steps <= 2 * (sum(int(x.shape[0]) for x in xs) + session.poll)
    with pytest.raises(RuntimeError):
        next(session.run(xs))                    # closed


@pytest.mark.parametrize("w", [0.1, 1.0])
def test_session_of_a_single_row(model, xs, w):
    """slots = 1 at beam 1: one row, whose position tensor has one element; every utterance after
    the first starts on the previous one's CTC state unless the prefix kernels are told the
    lengths are per row"""
    bs = get_beam_search_decoder(model.avsr, TOKENS, ctc_weight=w, beam_size=1)
    got = bs.decode_stream(xs, slots=1, max_frames=25)
    assert [_plain(n) for n in got] == _alone(model, xs, 1, w)


def test_session_survives_a_new_positional_table(model, xs):
    """a longer search between two streams makes the engine allocate a new positional-encoding
    table; the session's graphs keep reading the one they were captured with, which the session
    holds. (Fresh allocations of the old table's size in between, so that memory the session did
    not hold would be handed out again and overwritten.)"""
    bs = get_beam_search_decoder(model.avsr, TOKENS, ctc_weight=0.1, beam_size=3)
    eng = model.avsr.engine()
    want = _alone(model, xs, 3)
    with bs.stream(slots=2, max_frames=25) as session:
        first = [_plain(n) for _, n in sorted(session.run(xs), key=lambda p: p[0])]
        old = eng._pe
        eng.ensure_pe(2 * old.shape[0])
        assert eng._pe.data_ptr() != old.data_ptr()
        shape = old.shape
        del old
        junk = [torch.full(shape, 1e3, device=eng._pe.device) for _ in range(4)]
        second = [_plain(n) for _, n in sorted(session.run(xs), key=lambda p: p[0])]
    assert first == want and second == want and len(junk) == 4


def test_oversize_input_is_decoded_alone(model, xs):
    """max_frames = 20: the 25-frame utterances go through bs(x), in their place"""
    bs = get_beam_search_decoder(model.avsr, TOKENS, ctc_weight=0.1, beam_size=3)
    got = bs.decode_stream(xs, slots=2, max_frames=20)
    assert [_plain(n) for n in got] == _alone(model, xs, 3)


def test_session_geometry_and_precision(model):
    bs = get_beam_search_decoder(model.avsr, TOKENS, ctc_weight=0.1, beam_size=5)
    with pytest.raises(ValueError):
        bs.stream(slots=13)                      # 65 rows
    with bs.stream(max_frames=8) as session:
        assert session.S == 8
    eng = model.avsr.engine()
    dtype, eng.dtype = eng.dtype, torch.bfloat16
    try:
        with pytest.raises(NotImplementedError):
            bs.stream(max_frames=8)
    finally:
        eng.dtype = dtype


def test_run_sharded_through_a_stream(model, xs):
    """evaluate.run_sharded(infer_stream=...) on one rank: texts in unit order, equal to the
    infer_batch path's"""
    bs = get_beam_search_decoder(model.avsr, TOKENS, ctc_weight=0.1, beam_size=3)

    def text(nbest):
        return " ".join(TOKENS[t] for t in nbest[0].asdict()["yseq"][1:])
    with bs.stream(slots=2, max_frames=25) as session:
        streamed = evaluate.run_sharded(xs, None, infer_stream=lambda us: ((i, text(n)) for i, n in session.run(us)))
    batched = evaluate.run_sharded(xs, None, infer_batch=lambda us: [text(n) for n in bs.decode_batch(us)], batch=4)
    assert streamed == batched and len(streamed) == len(xs)
