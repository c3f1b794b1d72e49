"""The loop filter hands a macroblock's bottom rows down only where the row below filters its top edge, and stores only macroblocks
the filter can have changed (media_amd/csrc/k_deblock.h: db_hands_down, db_dirty).  What can go wrong is a sample without a writer
(the upper row leaves its bottom rows to a row that does not take them), a sample with a stale writer, a wait without a publish,
and a macroblock taken for clean that the right neighbour's left edge changed.  The inputs (tests/deblock_sparse.py) are short
sequences whose P pictures differ from the previous source in chosen macroblocks only: a sparse checkerboard, stripes of whole rows
and of whole columns, one macroblock in the bottom row and one in the last column, all macroblocks, none.  Sizes are the smallest
at which each path differs: 6 x 5 macroblocks (an odd row count: the last pair has an upper row only), 4 x 4, one column, one row,
and three slices (row form only).  Forms: one picture in flight in the row form and with the pair form forced, a lockstep batch of
8 in both.  Every access unit equals the oracle's, all three planes equal the oracle's before the filter and after it for every
picture, and a filter wait that timed out fails the call (the engine turns the filter's error word into an error).

The CPU part states of the oracle alone that each case contains what it is for.  Pictures 2 and 3 of a sequence are the settled
ones: in P picture 1 some unchanged macroblocks still code the IDR picture's quantisation error, so the clean fractions are asserted
from picture 2 on (picture 1 is compared on the GPU like every other).

Mutations of the committed kernel, each of which fails this file (profiles/deblock_sparse_headline.json): the upper row never
stores its bottom rows; the publish condition inverted; dirty without the right neighbour's left edge."""
import numpy as np
import pytest
from media_amd import capi, h264dec
import deblock_sparse as ds

gpu = pytest.mark.gpu
NPIC = 4
# w, h, slices -> the masks coded one GOP after the other
CASES = {
    (96, 80, 0): ds.MASKS,
    (64, 64, 0): ("checker", "rows", "columns", "all"),
    (16, 64, 0): ("checker", "all", "none"),          # one column (its checkerboard is every other row)
    (64, 16, 0): ("columns", "one_right", "all"),     # one row
    (112, 96, 3): ("checker", "rows", "all"),         # three slices of two rows
}
SIZES = list(CASES)
SIZE_IDS = ["%dx%d" % (w, h) + ("-%dslices" % s if s else "") for w, h, s in SIZES]
FORMS = ["rows", "pairs"]
BIG = (96, 80, 0)
# pictures of several slices are filtered in the row form only
SIZE_FORMS = [(s, f) for s in SIZES for f in FORMS if not (s[2] and f == "pairs")]
SIZE_FORM_IDS = ["%s-%s" % (SIZE_IDS[SIZES.index(s)], f) for s, f in SIZE_FORMS]


def _pictures(size, **kw):
    """[(mask, picture index in its GOP, picture)] of a size's cases"""
    w, h, sl = size
    _, out = ds.oracle(CASES[size], w, h, NPIC, sl, **kw)
    return [(CASES[size][i // NPIC], i % NPIC, o) for i, o in enumerate(out)]


def _cond(size, mask, pics=(1, 2, 3)):
    return [ds.conditions(o) for m, i, o in _pictures(size) if m == mask and i in pics]


# ---- conditions, stated of the oracle alone (no GPU needed)

@pytest.mark.parametrize("size", SIZES, ids=SIZE_IDS)
def test_oracle_filter_changes_only_what_the_strengths_allow(size):
    """the restated strengths agree with the oracle's filter: a macroblock the filter changed is dirty, or hands its bottom rows
    down to a filtered top edge"""
    for m, i, o in _pictures(size):
        stray = o["changed"] & ~(o["maps"]["dirty"] | o["maps"]["down"])
        assert not stray.any(), "%s picture %d: changed macroblocks without a strength %s" % (m, i, np.argwhere(stray).tolist())


@pytest.mark.parametrize("size", SIZES, ids=SIZE_IDS)
def test_oracle_every_p_picture_is_filtered_except_where_nothing_changes(size):
    for m, i, o in _pictures(size):
        if m == "none" and i >= 2:
            assert not o["changed"].any() and o["maps"]["clean"].all(), "picture %d of 'none' is settled: no strength at all" % i
        elif m != "none":
            assert o["changed"].any(), "%s picture %d: the filter changes nothing" % (m, i)


def test_oracle_named_cases_contain_what_they_are_for():
    for mask in ("checker", "rows", "columns"):
        for c in _cond(BIG, mask, (2, 3)):
            assert c["clean_fraction"] >= 1 / 3, (mask, c)
    for c in _cond(BIG, "checker"):
        for k in ("dirty_above_unfiltered_top", "clean_above_filtered_top", "mixed_tops_even_row", "mixed_tops_odd_row", "quiet_left_of_filtered_edge"):
            assert c[k], ("checker", k)
    for c in _cond(BIG, "rows"):
        assert c["clean_above_filtered_top"] and not c["mixed_tops_even_row"] and not c["mixed_tops_odd_row"], ("rows", c)
    for c in _cond(BIG, "columns"):
        assert c["mixed_tops_even_row"] and c["mixed_tops_odd_row"] and c["dirty_last_column"] and c["quiet_left_of_filtered_edge"], ("columns", c)
    for c in _cond(BIG, "one_bottom"):
        assert c["dirty_last_row"] and c["clean_fraction"] >= 0.8, ("one_bottom", c)
    for c in _cond(BIG, "one_right"):
        assert c["dirty_last_column"] and c["clean_fraction"] >= 0.8, ("one_right", c)
    for c in _cond(BIG, "all", (1, 3)):
        assert c["clean_fraction"] == 0.0, ("all", c)
    # a lone upper row (6 x 5 macroblocks: row 4) with a filtered and an unfiltered top edge
    assert any(o["maps"]["top"][4].any() and not o["maps"]["top"][4].all() for m, i, o in _pictures(BIG) if i), "mixed top edges in the lone upper row"
    # one column and one row: dirty and clean macroblocks above each other / beside each other
    assert any(c["clean_above_filtered_top"] for c in _cond((16, 64, 0), "checker"))
    assert any(c["quiet_left_of_filtered_edge"] for c in _cond((64, 16, 0), "one_right"))
    # slices: the last row of a slice is dirty above a first row that waits for nobody
    assert any(c["dirty_above_unfiltered_top"] and c["clean_above_filtered_top"] for c in _cond((112, 96, 3), "checker"))


def test_oracle_cases_between_them_contain_every_situation():
    seen = {}
    for size in SIZES:
        for m, i, o in _pictures(size):
            if i:
                for k, v in ds.conditions(o).items():
                    seen[k] = seen.get(k, False) or bool(v and k != "clean_fraction")
    seen.pop("clean_fraction")
    assert all(seen.values()), seen


def test_oracle_a_sparse_p_picture_with_intra_macroblocks_and_a_cut():
    """the bS 4 body of the P-step kernels meets clean macroblocks too; the cut makes a P picture of intra macroblocks"""
    assert any(0 < o["intra"] and ds.conditions(o)["clean_fraction"] >= 1 / 3 for m, i, o in _pictures(BIG) if i)
    cut = _pictures(BIG, cut=True)
    assert all(o["intra"] > 0 and o["changed"].any() for m, i, o in cut if i == NPIC - 1)


def test_oracle_unfiltered_stream_is_unfiltered():
    for m, i, o in _pictures(BIG, disable_deblock=1):
        assert all(np.array_equal(o["pre"][p], o["post"][p]) for p in range(3))


# ---- the GPU cases

def _set_form(monkeypatch, form):
    monkeypatch.setenv("MI355X_H264_PAIR_FILTER", "1" if form == "pairs" else "0")


def _same(got, want, what):
    bad = np.argwhere(got != want)
    assert bad.size == 0, "%s: first differing sample (row, column) %s" % (what, bad[0])


def _single(size, **kw):
    """GOP after GOP through one encoder, one picture in flight; the planes before and after the filter compared after every picture"""
    w, h, sl = size
    frames, _ = ds.oracle(CASES[size], w, h, NPIC, sl, **kw)
    enc = capi.Encoder(w, h, qp=ds.QP, gop=NPIC, slices=sl)
    try:
        enc.keep_pre()
        for f, (m, i, o) in zip(frames, _pictures(size, **kw)):
            assert enc.encode(f)[0] == o["au"], "%s picture %d: access unit" % (m, i)
            for p in range(3):
                _same(enc.debug_read(capi.DBG_PRE_Y + p), o["pre"][p], "%s picture %d plane %d before the filter" % (m, i, p))
                _same(enc.debug_read(capi.DBG_RECON_Y + p), o["post"][p], "%s picture %d plane %d" % (m, i, p))
    finally:
        enc.close()


@gpu
@pytest.mark.parametrize("size,form", SIZE_FORMS, ids=SIZE_FORM_IDS)
def test_one_picture_in_flight(monkeypatch, size, form):
    _set_form(monkeypatch, form)
    _single(size)


@gpu
@pytest.mark.parametrize("form", FORMS)
def test_scene_cut_makes_a_p_picture_of_intra_macroblocks(monkeypatch, form):
    _set_form(monkeypatch, form)
    _single(BIG, cut=True)


@gpu
@pytest.mark.parametrize("size,form", SIZE_FORMS, ids=SIZE_FORM_IDS)
def test_lockstep_batch_of_8(monkeypatch, size, form):
    """eight GOPs in lockstep, the size's masks in turn: every item's stream, and the first item's last picture before and after
    the filter"""
    import torch
    w, h, sl = size
    n, fbytes = 8, w * h * 3 // 2
    names = tuple(CASES[size][g % len(CASES[size])] for g in range(n))
    frames, want = ds.oracle(names, w, h, NPIC, sl)   # (the items of a batch are consecutive GOPs of one stream)
    refs = [want[g * NPIC:(g + 1) * NPIC] for g in range(n)]
    dev = torch.from_numpy(np.stack(frames)).cuda()
    _set_form(monkeypatch, form)
    enc = capi.Encoder(w, h, qp=ds.QP, gop=NPIC, slices=sl, batch=n)
    try:
        enc.keep_pre()
        cap = 4 * NPIC * fbytes + 4096
        out, szs, gb = np.zeros(n * cap, np.uint8), np.zeros(n * NPIC, np.uint32), np.zeros(n, np.uint64)
        enc.encode_gops_device(dev.data_ptr(), fbytes, NPIC * fbytes, NPIC, out, cap, szs, gb)
        for g in range(n):
            assert out[g * cap: g * cap + int(gb[g])].tobytes() == b"".join(o["au"] for o in refs[g]), "item %d (%s)" % (g, names[g])
        for p in range(3):
            _same(enc.debug_read(capi.DBG_PRE_Y + p), refs[0][-1]["pre"][p], "item 0 plane %d before the filter" % p)
            _same(enc.debug_read(capi.DBG_RECON_Y + p), refs[0][-1]["post"][p], "item 0 plane %d" % p)
    finally:
        enc.close()


def _decode(size, **kw):
    dec = h264dec.Decoder()
    try:
        for m, i, o in _pictures(size, **kw):
            assert dec.decode(o["au"]), "%s picture %d: no picture" % (m, i)
            for p in range(3):
                _same(dec.plane(p), o["post"][p], "%s picture %d decoded plane %d" % (m, i, p))
    finally:
        dec.close()


@gpu
def test_decoder_on_the_oracles_streams():
    """k_deblock_rows<.., PERMB, IND>: thresholds per macroblock; every mask, the checkerboard first"""
    _decode(BIG)


@gpu
def test_decoder_on_a_stream_with_the_filter_switched_off():
    """disable_deblocking_filter_idc 1: the pictures are not filtered at all"""
    _decode(BIG, disable_deblock=1)
