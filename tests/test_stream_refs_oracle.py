"""What tests/stream_refs.py holds, proved on the oracle alone (CPU): the mixed group's schedule has ticks in which pictures with
one, two and three usable reference pictures are handed in together, and in those ticks every P picture holds macroblocks of every
ref_idx_l0 its count allows - so a shared step that gave a position another position's count would code other bytes."""
import numpy as np
import ref_mix as rm
import stream_refs as sr


def test_the_count_rule_restated():
    assert sr.ref_counts(3, 30, 7) == [0, 1, 2, 3, 3, 3, 3]
    assert sr.ref_counts(2, 4, 9, forced=(6,)) == [0, 1, 2, 2, 0, 1, 0, 1, 2]
    assert sr.ref_counts(0, 3, 5) == [0, 1, 1, 0, 1]


def test_mixed_ticks_exist_and_the_oracle_agrees_with_the_schedule():
    ticks = sr.mixed_ticks()
    print("ticks with counts 1, 2 and 3 together: %s of %d" % (list(ticks), sr.TICKS))
    assert len(ticks) >= 4
    assert len({m.case.gop for m in sr.MIXED}) >= 4 and all(m.case.refs == sr.REFS for m in sr.MIXED)
    assert any(what == "idr" for m in sr.MIXED for _, what in m.events) and any(what != "idr" for m in sr.MIXED for _, what in m.events)
    for m in sr.MIXED:
        want = sr.expected(m)
        counts = sr.member_counts(m)
        assert [p.idr for p in want] == [n == 0 for n in counts], m.case.name
        assert [p.facts["available"] for p in want] == counts, m.case.name      # the independent decoder's RefPicList0
    forced = [m for m in sr.MIXED if any(what == "idr" for _, what in m.events)][0]
    at = [a for a, what in forced.events if what == "idr"][0]
    assert sr.member_counts(forced)[at - 1:at + 3] == [sr.ref_counts(3, forced.case.gop, at)[at - 1], 0, 1, 2], "the forced IDR restarts the count in mid-GOP"


def test_every_allowed_reference_index_is_used_in_the_mixed_ticks():
    seen = np.zeros((4, 3), np.int64)        # [count][ref_idx_l0]: macroblocks over the mixed ticks
    for t in sr.mixed_ticks():
        for k, i, n in sr.schedule()[t]:
            if n == 0:
                continue
            per_ref = sr.expected(sr.MIXED[k])[i].facts["shapes"].sum(axis=0)
            print("tick %d stream %d picture %d: %d reference pictures, macroblocks by ref_idx_l0 %s" % (t, k, i, n, per_ref.tolist()))
            assert all(per_ref[r] > 0 for r in range(n)) and not per_ref[n:].any(), (t, k, i, n, per_ref)
            seen[n] += per_ref
    print("macroblocks by [count][ref_idx_l0] over the mixed ticks: %s" % seen[1:].tolist())
    assert all(seen[n, r] > 0 for n in (1, 2, 3) for r in range(n))


def test_single_stream_cases_are_the_reference_mix_cases():
    names = [c.name for c in sr.ONE]
    assert names == ["split_48x48", "s1_208x160", "split_96x80_high", "still_96x80", "fast_96x128", "two_refs_split", "nv12", "long_ring"]
    assert all(c in rm.CASES for c in sr.ONE) and {c.refs for c in sr.ONE} == {2, 3}
