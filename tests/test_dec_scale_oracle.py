"""What the case list of tests/dec_scale.py holds, proved on the CPU from scale.taps and the numerators (tests/scale.py) and from
the packing restated in tests/dec_output.py: the GPU tests compare with nothing but these restatements, so this file shows that the
cases reach what the kernel can get wrong - five taps, exact ties, an identity dimension, odd chroma planes, rows that start off
16 bytes - and that the identity case IS the unscaled output."""
import numpy as np

import dec_output as do
import dec_scale as ds
import scale


def taps_used(S, D):
    """the largest number of taps with a non-zero weight of a result sample on an axis S -> D"""
    return int((scale.taps(S, D)[1] > 0).sum(axis=1).max())


def planes_of(case, k, t=0):
    """[(source plane, W, H)] of picture t of stream k: Y, Cb, Cr"""
    src = ds.source(case)
    _, _, i420, (w, h) = do.pictures(src, k)[t]
    W, H = ds.target_of(case, k)
    y, u, v = do.planes_of(i420, (w, h))
    return [(y, W, H), (u, W // 2, H // 2), (v, W // 2, H // 2)]


def test_every_target_can_be_made_and_is_even():
    for c in ds.CASES:
        for k in range(len(ds.source(c).streams)):
            (w, h), (W, H) = ds.size_of(c, k), ds.target_of(c, k)
            assert W % 2 == 0 and H % 2 == 0 and 2 <= W <= w <= 4 * W and 2 <= H <= h <= 4 * H, (c.name, k)
    src, tg = ds.MIXED
    assert sum(t is None for t in tg) == 2 and len(tg) == len(do.BY_NAME[src].streams)
    for k, t in enumerate(tg):
        w, h = do.pictures(do.BY_NAME[src], k)[0][3]
        assert t is None or (t[0] <= w <= 4 * t[0] and t[1] <= h <= 4 * t[1]), (k, t)


def test_five_taps_per_axis_in_luma_and_in_chroma():
    c = ds.BY_NAME[ds.FIVE]
    for k in range(len(ds.source(c).streams)):
        for sw, sh, w, h in ds.plane_shapes(c, k):
            assert taps_used(sw, w) == 5 and taps_used(sh, h) == 5, (k, sw, sh, w, h)
    # and the limit case reaches four source samples with no partial one
    c = ds.BY_NAME["96_to_24x20"]
    assert [taps_used(sw, w) for sw, _, w, _ in ds.plane_shapes(c, 0)] == [4, 4]


def test_exact_ties_in_every_plane_of_the_2_to_1_case_round_up():
    c = ds.BY_NAME[ds.TIES]
    k = [k for k in range(len(ds.source(c).streams)) if ds.size_of(c, k) == (96, 80)][0]
    for t in range(ds.STEPS):
        for p, (plane, W, H) in enumerate(planes_of(c, k, t)):
            n, D = scale.numerators(plane, W, H)
            tie = (n % D) * 2 == D
            assert tie.any(), "picture %d plane %d has no exact tie" % (t, p)
            out = scale.scale_plane(plane, W, H)
            assert (out[tie] == n[tie] // D + 1).all(), "a tie rounds up"


def test_an_identity_dimension_equals_its_source():
    c = ds.BY_NAME[ds.IDENTITY_DIM]
    for k in range(len(ds.source(c).streams)):
        (w, h), (W, H) = ds.size_of(c, k), ds.target_of(c, k)
        assert W == w and H < h
        for plane, pw, ph in planes_of(c, k):
            # the vertical resampling of a plane commutes with nothing being done horizontally: each column alone gives the same
            whole = scale.scale_plane(plane, pw, ph)
            col = scale.scale_plane(plane[:, 3:4], 1, ph)
            assert np.array_equal(whole[:, 3:4], col), k
            # and with both dimensions identical the plane is its source
            assert np.array_equal(scale.scale_plane(plane, plane.shape[1], plane.shape[0]), plane)


def test_odd_chroma_plane_widths_at_source_and_result():
    c = ds.BY_NAME[ds.FIVE]
    shapes = [ds.plane_shapes(c, k)[1] for k in range(len(ds.source(c).streams))]
    assert any(sw % 2 == 1 and w % 2 == 1 for sw, _, w, _ in shapes), shapes       # 25 -> 7 and 23 -> 7
    assert any(sh % 2 == 1 and h % 2 == 1 for _, sh, _, h in shapes), shapes       # 17 -> 5 and 15 -> 5
    assert all(ds.target_of(c, k)[0] % 4 == 2 for k in range(len(ds.source(c).streams)))


def test_result_rows_start_off_16_bytes_in_the_packed_destination():
    c = ds.BY_NAME[ds.FIVE]
    last = [0] * len(ds.source(c).streams)
    for lay in do.LAYOUTS:
        _, _, desc, _ = do.pack(ds.expected_pics(c.source, ds.targets(c), last), lay, 1)
        starts = [d["offset"] + r * d["stride"] for d in desc for r in range(d["height"])]
        assert any(s % 16 for s in starts), lay
    # with row_align 16 and 256 every row starts on 16 bytes: both kinds of destination are in the list
    for ra in (16, 256):
        _, _, desc, _ = do.pack(ds.expected_pics(c.source, ds.targets(c), last), do.I420, ra)
        assert all(d["stride"] % 16 == 0 and d["chroma_stride"] % 16 == 0 for d in desc)


def test_the_identity_case_equals_the_unscaled_output_byte_for_byte():
    c = ds.BY_NAME[ds.IDENTITY]
    src = ds.source(c)
    S = len(src.streams)
    for t in range(ds.STEPS):
        last = [t] * S
        plain = [(do.pictures(src, k)[t][2], do.pictures(src, k)[t][3]) for k in range(S)]
        for lay in do.LAYOUTS:
            for ra in ds.ROW_ALIGNS:
                a = do.pack(ds.expected_pics(c.source, ds.targets(c), last), lay, ra)
                b = do.pack(plain, lay, ra)
                assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2] == b[2] and a[3] == b[3], (t, lay, ra)


def test_every_case_has_the_pictures_the_gpu_tests_walk_through():
    for c in ds.CASES:
        assert ds.source(c).pictures >= ds.STEPS, c.name
    assert do.BY_NAME[ds.MIXED[0]].pictures >= ds.STEPS
