"""The four colour variants on the CPU (tests/colour.py restates include/mi355x_h264.h, "colour description"): what the header
claims about them, checked over the whole RGB cube and the whole YUV cube (tests/value_cube.py: rgb_luma_cube 0..15 carries every
(R, G, B) once, yuv_cube 0..15 every (Y, U, V) once); that the BT.601 limited restatement IS the arithmetic there has always
been (the oracle's conversion, value_cube's and dec_output's restatements); the round trip; and that no two variants agree on a
picture - otherwise a GPU test could not tell them apart."""
import functools
import itertools

import numpy as np
import pytest

import colour as col
import dec_output
import value_cube as vc
from oracle_lib import rgba_to_i420 as oracle_rgba_to_i420

IDS = [col.NAMES[v] for v in col.VARIANTS]
ROUND_TRIP_BOUND = 3   # the header's claim; the measured maxima are in DESIGN.md section 10


@functools.lru_cache(maxsize=None)
def rgb(k):
    """(R, G, B) of RGB cube picture k as int64 arrays: every triple with B in 16 k .. 16 k + 15"""
    p = vc.rgb_luma_cube(k).astype(np.int64)
    out = (p[..., 0], p[..., 1], p[..., 2])
    for a in out:
        a.setflags(write=False)
    return out


def test_the_tables_hold_what_the_header_states():
    hdr = open(__file__.replace("tests/test_colour_oracle.py", "include/mi355x_h264.h")).read()
    rows = {"BT.601 limited": (col.BT601, 0), "BT.709 limited": (col.BT709, 0), "BT.601 full": (col.BT601, 1), "BT.709 full": (col.BT709, 1)}
    import re
    found = {name: [] for name in rows}
    for line in hdr.splitlines():
        m = re.match(r"\s*\*\s+(BT\.\d+ (?:limited|full))\s+(-?\d[-\d,\s]*\d)", line)
        if m:
            found[m.group(1)].append(tuple(int(x) for x in re.findall(r"-?\d+", m.group(2))))
    for name, v in rows.items():
        assert len(found[name]) == 2, (name, found[name])
        way_in, way_out = found[name]
        assert way_in == col.IN[v]["y"] + col.IN[v]["cb"] + col.IN[v]["cr"], name
        k = col.OUT[v]
        assert way_out == (k["m"], k["o"], k["rv"], k["gu"], k["gv"], k["bu"]), name


@pytest.mark.parametrize("variant", col.VARIANTS, ids=IDS)
def test_ranges_grey_and_clip_sites_over_the_whole_rgb_cube(variant):
    full = variant[1]
    for key in ("cb", "cr"):
        assert sum(col.IN[variant][key]) == 0, "a chroma row that does not sum to 0 gives grey a colour"
    grey = np.arange(256, dtype=np.int64)
    cb, cr = col.chroma_raw(grey, grey, grey, variant)
    assert (cb == 128).all() and (cr == 128).all()
    y = col.luma_raw(grey, grey, grey, variant)
    assert (y[0], y[255]) == ((0, 255) if full else (16, 235))
    lo, hi = {"y": 999, "cb": 999, "cr": 999}, {"y": -999, "cb": -999, "cr": -999}
    sites = {"cb": [], "cr": []}
    for k in range(vc.LUMA_PICTURES):
        R, G, B = rgb(k)
        vals = dict(zip(("y", "cb", "cr"), [col.luma_raw(R, G, B, variant)] + col.chroma_raw(R, G, B, variant)))
        for key, a in vals.items():
            lo[key], hi[key] = min(lo[key], int(a.min())), max(hi[key], int(a.max()))
            if key != "y":
                for r, c in np.argwhere((a < 0) | (a > 255)):
                    sites[key].append((int(R[r, c]), int(G[r, c]), int(B[r, c]), int(a[r, c])))
    if not full:   # inside the studio ranges without the clip
        assert (lo["y"], hi["y"]) == (16, 235) and (lo["cb"], hi["cb"]) == (16, 240) and (lo["cr"], hi["cr"]) == (16, 240), (lo, hi)
        assert sites == {"cb": [], "cr": []}
    else:          # luma fills 0..255 and never leaves it; chroma reaches 256 at pure blue / pure red and nowhere else
        assert (lo["y"], hi["y"]) == (0, 255), (lo, hi)
        assert lo["cb"] >= 0 and lo["cr"] >= 0 and hi["cb"] == 256 and hi["cr"] == 256, (lo, hi)
        assert sites == {"cb": [(0, 0, 255, 256)], "cr": [(255, 0, 0, 256)]}, sites


def test_bt601_limited_is_the_arithmetic_there_has_always_been():
    """the way in against the oracle's conversion and value_cube's restatement, the way out against dec_output's, over both cubes"""
    for k in range(vc.LUMA_PICTURES):
        p = vc.rgb_luma_cube(k)
        mine = col.rgba_to_i420(p, col.DEFAULT)
        assert np.array_equal(mine, oracle_rgba_to_i420(p, vc.N, vc.N)), k
        if k % 5 == 0:
            assert np.array_equal(mine, vc.rgba_to_i420(p)), k
        y, u, v = vc.yuv_cube(k)
        up = lambda a: a.repeat(2, 0).repeat(2, 1)
        got = col.rgb_from_yuv(y, up(u), up(v), col.DEFAULT)
        for a, b in zip(got, dec_output.rgba_from_yuv(y, up(u), up(v))):
            assert np.array_equal(a, b), k
    for p in (vc.rgb_chroma_cube(0), vc.rgb_chroma_cube(63), vc.rounding_picture()):   # the block means and their rounding
        assert np.array_equal(col.rgba_to_i420(p, col.DEFAULT), oracle_rgba_to_i420(p, vc.N, vc.N))


@pytest.mark.parametrize("variant", col.VARIANTS, ids=IDS)
def test_round_trip_per_sample_over_the_whole_rgb_cube(variant):
    """out and back, 4:4:4 and no coding: every (R, G, B) through the variant's way in (its own sample as the block mean) and the
    variant's way out.  The bound is measured here, from the restatement, and printed"""
    worst = [0, 0, 0]
    for k in range(vc.LUMA_PICTURES):
        R, G, B = rgb(k)
        y = np.clip(col.luma_raw(R, G, B, variant), 0, 255)
        cb, cr = (np.clip(a, 0, 255) for a in col.chroma_raw(R, G, B, variant))
        back = col.rgb_from_yuv(y, cb, cr, variant)
        for c, (a, b) in enumerate(zip((R, G, B), back)):
            worst[c] = max(worst[c], int(np.abs(a - b.astype(np.int64)).max()))
    print("round trip %s: largest |difference| R %d G %d B %d" % (col.NAMES[variant], *worst))
    assert max(worst) <= ROUND_TRIP_BOUND, worst
    assert worst == MEASURED_ROUND_TRIP[variant], "DESIGN.md section 10 states %s" % (MEASURED_ROUND_TRIP[variant],)


# what the test above measures, as DESIGN.md section 10 records it: (R, G, B) per variant
MEASURED_ROUND_TRIP = {(col.BT601, 0): [2, 2, 3], (col.BT709, 0): [2, 2, 3], (col.BT601, 1): [2, 1, 2], (col.BT709, 1): [2, 1, 2]}


def test_every_variant_differs_from_every_other_on_the_test_pictures():
    """on the way in for the pictures the GPU cube tests feed (and the edge pictures), on the way out for every YUV cube picture"""
    pics = [("luma %d" % k, vc.rgb_luma_cube(k)) for k in (0, 7, 15)] + [("chroma %d" % k, vc.rgb_chroma_cube(k)) for k in (0, 31, 63)]
    pics += [("rounding", vc.rounding_picture())] + [("edge %dx%d/%d" % (w, h, i), p) for w, h in vc.EDGE_SIZES for i, p in enumerate(vc.edge_rgba(w, h))]
    for name, p in pics:
        outs = {v: col.rgba_to_i420(p, v) for v in col.VARIANTS}
        for a, b in itertools.combinations(col.VARIANTS, 2):
            assert not np.array_equal(outs[a], outs[b]), (name, col.NAMES[a], col.NAMES[b])
    for k in range(vc.YUV_PICTURES):
        y, u, v = vc.yuv_cube(k)
        outs = {var: col.rgba_picture(y, u, v, var) for var in col.VARIANTS}
        for a, b in itertools.combinations(col.VARIANTS, 2):
            assert not np.array_equal(outs[a], outs[b]), (k, col.NAMES[a], col.NAMES[b])


def test_variant_selection_by_matrix_code():
    assert col.variant_of(1, 1) == (col.BT709, 1) and col.variant_of(6, 0) == (col.BT601, 0) and col.variant_of(5, 1) == (col.BT601, 1)
    for m in (0, 2, 9, None, 4, 7, 255):
        assert col.variant_of(m, 1) == col.DEFAULT, m
    assert col.colour_word((col.BT709, 1)) == 0x101 and col.colour_word(col.DEFAULT) == 6
