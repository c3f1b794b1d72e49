"""The multi-reference cases of tests/ref_mix.py on the CPU oracle alone (no GPU): proof that the list, which
tests/test_gpu_ref_mix.py runs on the GPU, holds what it is there for.  The older reference pictures are CHOSEN, under every
partition shape; neighbours differ in their reference index, with and without residual; P_Skip lies beside them; vectors of the
older references cross slice boundaries; the window restarts inside every run.  And every access unit means what the writer's
side information says: the independent decoder reads the same reference index and vector for every block (ref_mix.expected
checks that while it builds the stream) - the oracle's reference-list order is what the GPU tests inherit.

Counts of the exhaustive search, ref_idx_l0 0 / 1 / 2, shapes 16x16 / P_Skip / 16x8 / 8x16 / 8x8 (the seeded search differs by
a macroblock or two):
  s1_208x160         [369, 4, 8, 17, 0]       [335, 0, 4, 15, 0]     [305, 0, 1, 16, 0]     96 intra macroblocks in P pictures
  split_208x160      [51, 0, 135, 101, 249]   [11, 0, 58, 62, 192]   [0, 0, 59, 67, 149]
  split_96x80_high   [9, 0, 14, 30, 51]       [1, 0, 18, 8, 20]      [0, 0, 17, 8, 27]
  split_48x48        [2, 0, 17, 17, 12]       [0, 0, 4, 7, 3]        [0, 0, 4, 0, 6]
  still_96x80        [34, 60, 0, 0, 0]        [57, 0, 0, 0, 0]       [70, 0, 0, 0, 0]       71 left and 60 top pairs differ, 47 + 38 with cbp 0
  fast_96x128        [133, 2, 9, 2, 0]        [119, 0, 3, 3, 0]      [83, 0, 3, 0, 0]       63 vectors across a slice edge
  two_refs_s1_96x80  [126, 25, 0, 0, 0]       [25, 0, 0, 1, 0]
  scroll_112x96      [116, 0, 5, 6, 1]        [109, 0, 1, 0, 0]      [127, 0, 0, 1, 0]
  long_ring          [2, 0, 74, 64, 67]       [0, 0, 15, 36, 27]     [0, 0, 22, 0, 52]
  two_refs_split     [2, 0, 46, 34, 112]      [0, 0, 5, 6, 4]"""
import numpy as np
import pytest
import ref_mix as rm

BOTH = [(c, s) for c in rm.CASES for s in rm.SEARCHES]
IDS = ["%s-search%d" % (c.name, s) for c, s in BOTH]


def test_the_list_is_the_one_the_modules_name():
    assert [(c.base, c.w, c.h, c.prof, c.refs, c.slices, c.qp, c.gop, c.pictures) for c in rm.CASES] == [
        ("s1", 208, 160, 66, 3, 0, 27, 8, 11), ("split", 208, 160, 77, 3, 0, 24, 8, 11), ("split", 96, 80, 100, 3, 2, 26, 7, 9),
        ("split", 48, 48, 66, 3, 0, 26, 8, 10), ("still", 96, 80, 66, 3, 0, 30, 8, 10), ("still", 96, 80, 100, 3, 2, 30, 8, 10),
        ("fast", 96, 128, 77, 3, 4, 26, 8, 10), ("s1", 96, 80, 100, 2, 0, 30, 6, 8), ("scroll", 112, 96, 66, 3, 3, 22, 9, 11),
        ("split", 48, 48, 66, 3, 0, 26, 40, 42), ("split", 96, 80, 100, 2, 0, 26, 7, 9), ("split", 96, 80, 100, 3, 2, 26, 7, 9)]
    assert rm.BY_NAME["nv12"].nv12 and sum(c.nv12 for c in rm.CASES) == 1
    assert rm.BY_NAME["nv12"]._replace(name="split_96x80_high", nv12=False) == rm.BY_NAME["split_96x80_high"]
    assert {c.name for c in rm.THREE} | {c.name for c in rm.TWO} == set(rm.BY_NAME)


def test_the_content_is_what_its_description_says():
    w, h = 96, 80
    for base in rm.BASES:
        pm = rm.period_map(w, h, 3, 1)
        assert set(pm.ravel()) == {1, 2, 3}
        left = pm[:, : pm.shape[1] // 2]
        assert (left[:, 1:] != left[:, :-1]).any(), "left half: neighbours differ"
        right = pm[:, pm.shape[1] // 2 + 1:]          # (from the first whole 2x2 group on)
        assert np.array_equal(right[:, 0::2][:, : right.shape[1] // 2], right[:, 1::2]), "right half: drawn per 2x2 macroblocks"
        for t in (4, 7, 9):
            f = rm.frame_ref_mix(base, w, h, t, 3, 1)
            y = f[: w * h].reshape(h, w)
            for p in (1, 2, 3):
                want = rm.variant(rm.base_frame(base, w, h, t // p), w, h, t % p)[0]
                mask = np.kron(pm == p, np.ones((16, 16), bool))
                assert np.array_equal(y[mask], np.ascontiguousarray(want)[mask]), (base, t, p)
    # the variants are unlike each other and unlike the picture (mean absolute luma difference of tens of levels)
    f = rm.base_frame("s1", w, h, 3)
    v = [rm.variant(f, w, h, k)[0].astype(np.int32) for k in range(3)]
    assert all(np.abs(v[a] - v[b]).mean() > 20 for a, b in ((0, 1), (0, 2), (1, 2)))
    # still: a region of period p repeats picture t - p exactly and no picture between
    pm = np.kron(rm.period_map(w, h, 3, 1), np.ones((16, 16), np.int32))
    ys = [rm.frame_ref_mix("still", w, h, t, 3, 1)[: w * h].reshape(h, w) for t in range(8)]
    for p in (1, 2, 3):
        for t in range(3, 8):
            assert np.array_equal(ys[t][pm == p], ys[t - p][pm == p])
            assert all(not np.array_equal(ys[t][pm == p], ys[t - k][pm == p]) for k in range(1, p))


@pytest.mark.parametrize("c,search", BOTH, ids=IDS)
def test_every_access_unit_decodes_to_what_the_writer_says(c, search):
    """planes, reference index per 4x4 block and vectors: asserted picture by picture in ref_mix.expected"""
    pics = rm.expected(c, search)
    assert len(pics) == c.pictures and [p.idr for p in pics] == [i % c.gop == 0 for i in range(c.pictures)]
    for p in pics:
        if not p.idr:   # RefPicList0 is the sliding window, newest first: entry r was decoded r pictures before the last one
            assert p.facts["ref_ages"][: p.facts["available"]] == tuple(range(p.facts["available"])), p.facts["ref_ages"]
            assert p.facts["available"] == min(c.refs, p.facts["since_idr"])
            refs_used = p.facts["ref"][p.facts["inter"]]
            assert refs_used.size == 0 or refs_used.max() < p.facts["available"]


@pytest.mark.parametrize("search", rm.SEARCHES)
def test_every_shape_takes_every_reference_index(search):
    total = sum(rm.totals(rm.expected(c, search))["shapes"] for c in rm.THREE if not c.nv12)
    print(total.T.tolist())
    for s in (0, 2, 3, 4):
        for r in range(3):
            assert total[s, r] >= 10, "%s with ref_idx_l0 %d: %d macroblocks" % (rm.SHAPES[s], r, total[s, r])


@pytest.mark.parametrize("c,search", BOTH, ids=IDS)
def test_the_older_pictures_are_chosen_in_every_case(c, search):
    shapes = rm.totals(rm.expected(c, search))["shapes"]
    print(c.name, shapes.T.tolist())
    if c.refs == 3:
        assert shapes[:, 2].sum() >= 5
    else:
        assert shapes[:, 1].sum() >= 10 and shapes[:, 2].sum() == 0


@pytest.mark.parametrize("name", rm.STILL)
@pytest.mark.parametrize("search", rm.SEARCHES)
def test_still_skips_beside_older_references_and_pairs_that_differ_in_the_reference_alone(name, search):
    tot = rm.totals(rm.expected(rm.BY_NAME[name], search))
    print(name, {k: v for k, v in tot.items() if k != "shapes"}, tot["shapes"].T.tolist())
    assert tot["shapes"][1].sum() >= 30, "P_Skip macroblocks"
    assert tot["skip_beside_older"] >= 10
    assert tot["diff_left"] + tot["diff_top"] >= 40
    assert tot["diff_left_cbp0"] + tot["diff_top_cbp0"] >= 10, "pairs whose filter strength comes from the reference difference alone"


@pytest.mark.parametrize("name", rm.STILL)
@pytest.mark.parametrize("search", rm.SEARCHES)
def test_still_a_region_of_period_p_takes_ref_idx_p_minus_1(name, search):
    """the selection means what the construction intends: once p references are available, at least 90 % of the inter
    macroblocks of the period-p regions take ref_idx_l0 = p - 1.  The oracle's shares: period 1 73 of 80 (High with two slices
    72 of 80; a region that repeats every picture is found unchanged in every reference), period 2 42 of 42, period 3 65 of 65
    (seeded search 64 of 65)"""
    c = rm.BY_NAME[name]
    pm = rm.period_map(c.w, c.h, c.refs, c.seed)
    for p in (1, 2, 3):
        hit = n = 0
        for pic in rm.expected(c, search):
            if not pic.idr and pic.facts["available"] >= p:
                sel = pic.facts["inter"] & (pm == p)
                n += int(sel.sum())
                hit += int((sel & (pic.facts["ref"] == p - 1)).sum())
        print(name, "period", p, hit, "of", n)
        assert n >= 20 and 10 * hit >= 9 * n, (p, hit, n)


@pytest.mark.parametrize("search", rm.SEARCHES)
def test_s1_has_intra_macroblocks_where_three_references_were_searched(search):
    pics = rm.expected(rm.BY_NAME["s1_208x160"], search)
    assert sum(p.facts["intra_in_p"] for p in pics if p.facts["available"] == 3) > 0


@pytest.mark.parametrize("search", rm.SEARCHES)
def test_fast_vectors_of_older_references_cross_inner_slice_boundaries(search):
    c = rm.BY_NAME["fast_96x128"]
    assert rm.slice_rows(c) == 2
    assert rm.totals(rm.expected(c, search))["across_slice_edge"] >= 5


@pytest.mark.parametrize("c", rm.THREE, ids=[c.name for c in rm.THREE])
def test_the_window_restarts_inside_every_run(c):
    """pictures with 1, 2 and 3 available references all occur, and P pictures lie before and after the IDR picture inside the
    run: three references before it, one right after it"""
    pics = rm.expected(c, 1)
    assert {p.facts["available"] for p in pics if not p.idr} == {1, 2, 3}
    inner = [i for i, p in enumerate(pics) if p.idr and i]
    assert inner and inner[0] + 1 < len(pics)
    assert pics[inner[0] - 1].facts["available"] == 3 and pics[inner[0] + 1].facts["available"] == 1


def test_long_ring_goes_round_and_frame_num_runs_on():
    c = rm.BY_NAME["long_ring"]
    assert c.gop - 1 >= 12 * c.refs and c.gop > max(k.gop for k in rm.CASES if k is not c) * 4


def test_me_launches_formula():
    assert rm.me_launches(3, [True, False, False, False, False, True, False]) == 1 + 2 + 3 + 3 + 1
    assert rm.me_launches(0, [True, False, False]) == 2


@pytest.mark.parametrize("b", rm.BATCHES, ids=lambda b: b.name)
def test_batch_items_take_different_references_in_the_same_launch(b):
    """the items of a lockstep batch are streams of their own, and in one and the same P step their macroblocks at the same
    position take different reference indices"""
    items, _ = rm.batch_expected(b, 1)
    assert (b.G, b.case.w, b.case.h) in ((8, 48, 48), (3, 96, 80)) and b.case.refs == 3
    assert len({b"".join(p.au for p in gop) for gop in items}) == b.G
    mixed = 0
    for i in range(3, b.case.gop):      # (three references available)
        refs = np.stack([np.where(gop[i].facts["inter"], gop[i].facts["ref"], -1) for gop in items])
        mixed += int(((refs.max(axis=0) > refs.min(axis=0)) & (refs.min(axis=0) >= 0)).sum())
        assert all(len({int(r) for r in gop[i].facts["ref"][gop[i].facts["inter"]]}) >= 2 for gop in items), "picture %d: an item with one reference index only" % i
    assert mixed >= 10


def test_the_window_restarts_at_a_forced_idr():
    """what tests/test_gpu_ref_mix.py drives: an IDR picture forced in the middle of a GOP, then QP 20 and QP 40"""
    c = rm.BY_NAME["s1_208x160"]
    pics = rm.expected(c, 1, rm.WINDOW_EVENTS)
    plain = rm.expected(c, 1)
    assert pics[4].idr and not plain[4].idr
    assert [p.facts["available"] for p in pics[3:8]] == [3, 0, 1, 2, 3]
    assert all(a.au != b.au for a, b in zip(pics[4:], plain[4:]))
    assert sum(p.facts["shapes"][:, 1:].sum() for p in pics[5:]) >= 50, "the older pictures are chosen after the restart as well"
