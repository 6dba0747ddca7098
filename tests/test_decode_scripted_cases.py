"""What the scripted-search cases (tests/decode_ref.SCRIPTED_BATCHES, run on the GPU by
tests/test_gpu_decode_scripted.py) cover, decided from the fp64 reference alone: how many are
skipped for top scores closer than twice the project tolerance, and that enough of the rest meet
each ending rule."""
from tests import decode_ref as R


def test_scripted_cases_skip_share_and_coverage():
    cases = skipped = 0
    seen = dict(eos_early=0, forced=0, unscored=0, end_detect=0)
    combos = set()
    for batch in R.SCRIPTED_BATCHES:
        c, refs = R.scripted_reference(batch)
        assert len(refs) == R.SCRIPTED_U
        if batch[3] == "random":
            assert len(set(c["Ts"])) >= 3 and all(6 <= T <= 20 for T in c["Ts"])
            combos.add(batch[1:3])
        for hyps, info, skip in refs:
            cases += 1
            skipped += skip
            assert hyps                                  # every search ends at least one hypothesis
            if not skip:
                for k in seen:
                    seen[k] += bool(info[k])
    assert combos == {(b, w) for b in (1, 3, 5) for w in (0.0, 0.1, 0.5, 1.0)}
    assert cases >= 80 and skipped <= R.MAX_SKIP_SHARE * cases, (skipped, cases)
    assert all(n >= 5 for n in seen.values()), seen


def test_long_case_reference_is_well_separated():
    c = R.long_case()
    _, info = R.scripted_search_ref(c["table"][0], c["ctc"][0], c["beam"], c["w"], c["maxlenratio"])
    assert info["steps"] == 12 and info["margin"] >= 1.0
