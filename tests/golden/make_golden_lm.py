"""Golden vectors for beam searches with an n-gram LM scorer and the length bonus, produced by
running the REFERENCE's own BatchBeamSearch (quanpn90/avsr, read-only at /root/reference) on CPU,
fp32, in this container. Never run on the GPU box; only the .npz output is committed:
  tests/golden/avsr_lm.npz

The reference's get_beam_search_decoder builds the scorer slots "length_bonus" and "lm" and
hard-wires them off. Here its BatchBeamSearch is built with the same four slots and non-zero
weights: scorers {"decoder", "ctc", "length_bonus": LengthBonus, "lm": NgramScorer}, the last a
subclass of its BatchScorerInterface defined below, which applies the rule of tests/ngram_ref.py
(RefLM, fp64) to every token of every hypothesis. Model: the tiny recipe (oracle/weights.py
TINY_CONFIG, gen_tensor weights, seed 0, dropouts 0, eval); inputs: the reference's own encoder
outputs stored in avsr_tiny.N.npz (dec_enc_0 / _1); beam 3, ctc_weight 0.1, for the settings
SETTINGS of (lm_weight, length_bonus).

The LM is a seeded (the first seed from 11 on with which everything asserted below holds) order-3 table over the 5049-token vocabulary whose entries are the 1- to 3-grams
of the token sequences the plain search (no LM) returns, <s> and </s> included, so higher-order
entries are hit; the n-grams only the plain best hypothesis holds score low, the others high, so
the LM moves the best hypothesis. Every other token scores unk_logp.

Stored: the table itself (so the test depends on no RNG), and per (setting, clip) EVERY returned
hypothesis (tokens, total / decoder / ctc / lm / length_bonus scores) and the number of steps the
search ran. Asserted here (and re-asserted from the fixture by tests/test_ngram_host.py): the best
hypothesis differs from yseq_b3_* of the plain golden; neighbouring n-best totals are at least 1e-3
relative apart (ten times the comparison tolerance); entries of order >= 2 were used.

usage: PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_lm.py   (about 1 min)
"""
import os
import sys
import time

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, "/root/reference")
sys.dont_write_bytecode = True

from oracle.weights import NO_DROPOUT, TINY_CONFIG, gen_tensor  # noqa: E402
from tests.golden.parts import load_parts  # noqa: E402
from tests.ngram_ref import RefLM  # noqa: E402

SETTINGS = ((1.0, 0.0), (0.7, 0.5))
BEAM, CTC_WEIGHT, ORDER, UNK = 3, 0.1, 3, -8.0
V = 5049
EOS = V - 1


def q(x):
    return round(float(x) * 64.0) / 64.0


def build_table(plain, seed):
    """plain: per clip the token sequences (sos first, eos last) of the plain search, best first"""
    rng = np.random.RandomState(seed)
    best_only, other = set(), set()
    for seqs in plain:
        for rank, y in enumerate(seqs):
            h = [int(t) for t in y]
            for i in range(1, len(h)):                  # the k-grams ending at every position after sos
                for k in range(1, min(ORDER, i + 1) + 1):
                    (best_only if rank == 0 else other).add(tuple(h[i - k + 1:i + 1]))
    best_only -= other
    ent = {}
    for g in sorted(best_only | other, key=lambda g: (len(g), g)):
        lo, hi = (-5.0, -3.0) if g in best_only else (-2.5, -0.1)
        if len(g) == 1:
            lo, hi = lo - 2.0, hi - 2.0
        ent[(g[:-1], g[-1])] = (q(rng.uniform(lo, hi)), q(rng.uniform(-0.5, -0.05)) if len(g) < ORDER else 0.0)
    ent.setdefault(((), EOS), (q(-3.0), q(-0.25)))
    return ent


def main():
    torch.manual_seed(0)
    torch.set_num_threads(8)
    from src.avhubert_avsr.avhubert_avsr_model import AVHubertAVSR, get_beam_search_decoder
    from src.avhubert_avsr.configuration_avhubert_avsr import AVHubertAVSRConfig
    from src.nets.batch_beam_search import BatchBeamSearch
    from src.nets.scorer_interface import BatchScorerInterface
    from src.nets.scorers.ctc import CTCPrefixScorer
    from src.nets.scorers.length_bonus import LengthBonus

    class NgramScorer(BatchScorerInterface):
        """a full scorer: the RefLM score of every vocabulary token after each hypothesis's prefix
        (the state is recomputed from the prefix, so the scorer keeps none)"""

        def __init__(self, lm):
            self.lm, self.calls, self.seen = lm, 0, {}

        def score(self, y, state, x):
            ctx = self.lm.state([int(t) for t in y])
            if ctx not in self.seen:                    # (the scores depend on the state only)
                self.seen[ctx] = torch.tensor([self.lm.score(ctx, v)[0] for v in range(V)], dtype=torch.float64)
            return self.seen[ctx].to(x.dtype), None

        def batch_score(self, ys, states, xs):
            self.calls += 1
            return torch.stack([self.score(y, None, xs)[0] for y in ys]), [None] * len(ys)

    t0 = time.time()
    model = AVHubertAVSR(AVHubertAVSRConfig(**TINY_CONFIG, **NO_DROPOUT))
    sd = model.state_dict()
    model.load_state_dict({k: torch.from_numpy(gen_tensor(k, v.shape, seed=0)) for k, v in sd.items()}, strict=True)
    model.eval()
    g = load_parts("avsr_tiny")
    token_list = ["<blank>"] + [f"u{i}" for i in range(1, V - 1)] + ["<eos>"]
    e2e = model.avsr
    assert e2e.sos == e2e.eos == EOS
    xs = [torch.from_numpy(g[f"dec_enc_{c}"]) for c in range(2)]
    plain_bs = get_beam_search_decoder(e2e, token_list, ctc_weight=CTC_WEIGHT, beam_size=BEAM)
    with torch.no_grad():
        plain = [[h.asdict()["yseq"] for h in plain_bs(x)] for x in xs]
    for c in range(2):
        assert plain[c][0] == g[f"yseq_b3_{c}"].tolist(), "the plain search is the stored golden"
    def generate(seed):
        ent = build_table(plain, seed)
        lm = RefLM(ORDER, ent, UNK, sos=EOS, eos=EOS)
        keys = sorted(ent, key=lambda k: (len(k[0]), k))
        out = {"seed": np.array(seed), "settings": np.array(SETTINGS), "unk": np.array(UNK), "order": np.array(ORDER),
               "tab_tok": np.array([[-1] * (ORDER - 1 - len(c)) + list(c) + [v] for c, v in keys], np.int32),
               "tab_logp": np.array([ent[k][0] for k in keys]), "tab_bo": np.array([ent[k][1] for k in keys])}
        print(f"table of {len(ent)} entries; model and plain search in {time.time() - t0:.1f} s", flush=True)
        for s, (w_lm, w_len) in enumerate(SETTINGS):
            scorer = NgramScorer(lm)
            bs = BatchBeamSearch(
                beam_size=BEAM, vocab_size=V,
                weights={"decoder": 1.0 - CTC_WEIGHT, "ctc": CTC_WEIGHT, "lm": w_lm, "length_bonus": w_len},
                scorers={"decoder": e2e.decoder, "ctc": CTCPrefixScorer(e2e.ctc, e2e.eos), "length_bonus": LengthBonus(V),
                         "lm": scorer},
                sos=e2e.sos, eos=e2e.eos, token_list=token_list, pre_beam_score_key="decoder")
            for c, x in enumerate(xs):
                scorer.calls = 0
                with torch.no_grad():
                    hyps = bs(x)
                d = [h.asdict() for h in hyps]
                key = f"lm{s}_{c}"
                out[key + "_steps"] = np.array(scorer.calls)
                out[key + "_len"] = np.array([len(h["yseq"]) for h in d])
                out[key + "_yseq"] = np.concatenate([np.array([int(t) for t in h["yseq"]]) for h in d])
                out[key + "_score"] = np.array([float(h["score"]) for h in d])
                for name in ("decoder", "ctc", "lm", "length_bonus"):
                    if name in d[0]["scores"]:
                        out[key + "_" + name] = np.array([float(h["scores"][name]) for h in d])
                assert ("length_bonus" in d[0]["scores"]) == (w_len != 0.0) and "lm" in d[0]["scores"]
                # what the fixture is for
                assert d[0]["yseq"] != plain[c][0], (key, "the LM does not move the best hypothesis")
                tot = out[key + "_score"]
                gaps = np.abs(np.diff(tot)) / np.maximum(np.abs(tot[:-1]), np.abs(tot[1:]))
                assert len(d) >= 2 and gaps.min() >= 1e-3, (key, gaps.min())
                orders, ctx = set(), lm.state((EOS,))
                for v in d[0]["yseq"][1:]:
                    _, ctx, (o, _) = lm.score(ctx, int(v))
                    orders.add(o)
                assert max(orders) >= 2, (key, orders)
                print(f"{key}: {len(d)} hyps, {scorer.calls} steps, lengths {out[key + '_len'].tolist()[:6]}, best "
                      f"{d[0]['score']:.4f} {d[0]['scores']}, min gap {gaps.min():.2e}, orders on the best path "
                      f"{sorted(orders)}", flush=True)
        return out

    out = None
    for seed in range(11, 300):
        try:
            out = generate(seed)
            break
        except AssertionError as e:
            print(f"seed {seed}: {e}", flush=True)
    assert out is not None
    path = os.path.join(HERE, "avsr_lm.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes in", round(time.time() - t0, 1), "s")


if __name__ == "__main__":
    main()
