"""What the sequence of tests/tq_sparse.py holds, proven on the CPU oracle alone (its own mbinfo and levels): the parts whose
stores k_tq / k_tq8 now leave out, and - the new failure mode - parts that are empty in a picture although the picture before left
non-zero levels in the same place.  tests/test_gpu_tq_sparse.py runs the same sequence on the GPU."""
import numpy as np
import tq_sparse as ts


def test_sequence_reaches_every_sparse_store():
    pics = ts.expected(*ts.SIZE)
    assert [p.idr for p in pics] == [True] + [False] * (len(ts.QPS) - 1), "one GOP"
    cov = ts.coverage(pics)
    print({k: (sorted(v) if isinstance(v, set) else v) for k, v in cov.items()})
    assert cov["luma_patterns"] == set(range(16)), "all 16 luma patterns among the coded inter macroblocks"
    assert cov["chroma_cbp"] == {0, 1, 2}
    assert cov["types"] & {5, 6, 7}, "a partitioned macroblock"
    assert cov["stale_quadrants"] >= 500
    assert cov["stale_chroma_ac"] >= 100


def test_high_profile_sequence_has_stale_8x8_quadrants():
    """k_tq8 stores a quadrant's four lists, its TotalCoeff word and its samples together: the sequence must hold quadrants that
    go from coded to empty there as well"""
    cov = ts.coverage(ts.expected(*ts.SIZE, prof=100))
    print({k: (sorted(v) if isinstance(v, set) else v) for k, v in cov.items()})
    assert cov["stale_quadrants"] >= 500 and cov["stale_chroma_ac"] >= 100
    # (in k_tq8 a lane IS a quadrant and decides alone: what counts is every quadrant coded and empty, not the combinations)
    for q in range(4):
        assert {(p >> q) & 1 for p in cov["luma_patterns"]} == {0, 1}, q
    assert cov["chroma_cbp"] == {0, 1, 2}


def test_small_size_is_less_than_one_wave():
    pics = ts.expected(*ts.SMALL)
    assert len(pics[0].stages.mbinfo) == 6
    assert any(np.isin(p.stages.mbinfo["type"], (1, 5, 6, 7)).any() for p in pics[1:]), "an inter macroblock that k_tq codes"


def test_batch_calls_put_dense_in_front_of_sparse():
    """the lockstep case's order runs over the calls: item 0's last picture of a sparse call has quadrants that are empty where the
    dense call before it left levels"""
    exp = ts.expected_batch(*ts.SIZE)
    for call in (1, 3):
        pics = [ts.Pic(None, False, ts.BATCH_QPS[c], exp[c][0][1]) for c in (call - 1, call)]
        cov = ts.coverage(pics)
        assert cov["stale_quadrants"] >= 50, (call, cov)
