"""What tests/scale.py holds (CPU): the restated resampling arithmetic against known answers and against round-half-up in Python
integers, and the properties the case list of tests/test_gpu_scale.py relies on."""
from fractions import Fraction
import numpy as np
import pytest
import scale


def test_two_to_one_is_the_rounded_mean_of_four():
    rng = np.random.RandomState(3)
    p = rng.randint(0, 256, (48, 64)).astype(np.uint8)
    q = p.astype(np.int64)
    want = (q[0::2, 0::2] + q[0::2, 1::2] + q[1::2, 0::2] + q[1::2, 1::2] + 2) >> 2
    assert np.array_equal(scale.scale_plane(p, 32, 24), want)


def test_known_row():
    row = np.array([[0, 255, 0, 255, 255, 0]], np.uint8)
    assert scale.scale_plane(row, 4, 1).tolist() == [[85, 85, 255, 85]]


def test_identity_is_the_identity():
    p = np.random.RandomState(4).randint(0, 256, (18, 34)).astype(np.uint8)
    assert np.array_equal(scale.scale_plane(p, 34, 18), p)


@pytest.mark.parametrize("value", [0, 1, 127, 201, 255])
def test_a_constant_stays_constant(value):
    for c in scale.CASES[:7]:
        for sw, sh, w, h in scale.plane_shapes(c):
            assert (scale.scale_plane(np.full((sh, sw), value, np.uint8), w, h) == value).all(), c.name


def test_weights_sum_to_the_source_size_and_lie_inside_it():
    for c in scale.CASES:
        for sw, sh, w, h in scale.plane_shapes(c):
            for S, D in ((sw, w), (sh, h)):
                idx, wt = scale.taps(S, D)
                assert (wt.sum(axis=1) == S).all()
                assert idx.min() == 0 and idx.max() == S - 1
                # every source sample is used with total weight D: the result is a mean of means
                tot = np.zeros(S, np.int64)
                np.add.at(tot, idx.ravel(), wt.ravel())
                assert (tot == D).all()


def _max_taps(S, D):
    return int((scale.taps(S, D)[1] > 0).sum(axis=1).max())


def _has_tie(sw, sh, w, h):
    """some result sample CAN fall on a half: D even and a numerator residue of D / 2 reachable - looked for with random content"""
    D = sw * sh
    if D & 1:
        return False
    p = np.random.RandomState(9).randint(0, 256, (sh, sw)).astype(np.uint8)
    n, _ = scale.numerators(p, w, h)
    return bool(((n % D) == D // 2).any())


def test_the_list_holds_what_it_is_for():
    shapes = [s for c in scale.CASES for s in scale.plane_shapes(c)]
    assert any(_max_taps(sw, w) == 5 and _max_taps(sh, h) == 5 for sw, sh, w, h in shapes), "a plane with 5 taps in both dimensions"
    for S, D in ((70, 18), (62, 16), (35, 9), (31, 8)):
        assert _max_taps(S, D) == 5
    assert _max_taps(70, 34) == 3
    assert _has_tie(64, 48, 32, 24) and _has_tie(64, 64, 16, 16) and _has_tie(96, 64, 64, 48), "ties at 2:1, 4:1 and 3:2"
    assert any((sw * sh) & 1 for sw, sh, w, h in shapes), "a plane of odd D (no tie exists)"
    assert any(sw == w or sh == h for sw, sh, w, h in shapes), "a 1:1 dimension"
    assert any(w % 4 == 2 for sw, sh, w, h in shapes) and any(w & 1 for sw, sh, w, h in shapes)
    assert any(c.h % 16 for c in scale.CASES), "a coded height that is not the display height"
    assert any(sw == 4 * w and sh == 4 * h for sw, sh, w, h in shapes), "the limit"
    for c in scale.CASES:
        assert c.w <= c.sw <= 4 * c.w and c.h <= c.sh <= 4 * c.h and not (c.sw | c.sh | c.w | c.h) & 1
    assert sum(1 for c in scale.CASES if c.rgba) == 5


def test_the_largest_numerator_stays_below_two_to_the_32():
    worst = 0
    for c in scale.CASES:
        for sw, sh, w, h in scale.plane_shapes(c):
            worst = max(worst, 255 * sw * sh + ((sw * sh) >> 1))
    assert worst == 255 * 4096 * 4096 + (4096 * 4096 >> 1) and worst < 1 << 32
    # and the list's own content reaches the largest numerator: the top half of the 4096 x 4096 picture is all 255
    c = scale.BY_NAME["max_4096x4096"]
    y = scale.planes_i420(scale.source_i420(c.name)[0], c.sw, c.sh)[0]
    n, D = scale.numerators(y[:64], c.w, 16)
    assert int(n.max()) == 255 * D


def _half_up(n, D):
    """round-half-up of n / D in Python integers"""
    f = Fraction(int(n), int(D))
    fl = f.numerator // f.denominator
    return fl + 1 if f - fl >= Fraction(1, 2) else fl


@pytest.mark.parametrize("case", [c.name for c in scale.CASES])
def test_the_expression_is_round_half_up_for_every_sample(case):
    """floor((N + (D >> 1)) / D) against round-half-up, for every sample of every plane of the case's first picture: in whole as
    2 D out <= 2 N + D < 2 D (out + 1) in 64-bit integers (exact: 2 N + D < 2^34), and for up to 3000 distinct numerators, the
    halves first, in Python integers"""
    c = scale.BY_NAME[case]
    planes = scale.planes_i420(scale.source_i420(case)[0], c.sw, c.sh)
    for p, (sw, sh, w, h) in zip(planes, [scale.plane_shapes(c)[0]] + [scale.plane_shapes(c)[1]] * 2):
        n, D = scale.numerators(p, w, h)
        got = (n + (D >> 1)) // D
        assert ((2 * n + D >= 2 * D * got) & (2 * n + D < 2 * D * (got + 1))).all()
        assert np.array_equal(got, scale.scale_plane(p, w, h))
        u = np.unique(n)
        halves = u[(2 * (u % D)) == D]
        for v in np.concatenate([halves[:1000], u[:: max(1, len(u) // 2000)]]):
            assert int((int(v) + (D >> 1)) // D) == _half_up(v, D)
