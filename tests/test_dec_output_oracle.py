"""Decoder output in four layouts, on the CPU: the Python restatement (tests/dec_output.py) against known answers and the
properties the header states, and what the case list holds that tests/test_gpu_dec_output.py relies on.  The conditions on the
list are conditions, not measurements: a list that lacks one fails here."""
import numpy as np
import pytest

import dec_output as do

# (Y, U, V) -> (R, G, B) by c = 298 (Y - 16), d = U - 128, e = V - 128, R = clip((c + 409 e + 128) >> 8),
# G = clip((c - 100 d - 208 e + 128) >> 8), B = clip((c + 516 d + 128) >> 8), worked out by hand from the formula
KNOWN = [((235, 128, 128), (255, 255, 255)), ((16, 128, 128), (0, 0, 0)), ((82, 90, 240), (255, 1, 0)), ((144, 54, 34), (0, 254, 0)),
         ((41, 240, 110), (0, 0, 255)), ((210, 16, 146), (255, 255, 0)), ((0, 0, 0), (0, 135, 0)), ((255, 255, 255), (255, 125, 255)),
         ((255, 0, 255), (255, 225, 20)), ((0, 255, 0), (0, 36, 237))]


def test_rgba_known_answers():
    for yuv, rgb in KNOWN:
        got = tuple(int(c) for c in do.rgba_from_yuv(*yuv))
        assert got == rgb, (yuv, got, rgb)
    # as a picture: one chroma sample serves its 2x2 block, alpha is 255
    y = np.array([[235, 16], [82, 144]], np.uint8)
    i420 = np.concatenate([y.ravel(), [128], [128]]).astype(np.uint8)
    (_, row0), (_, row1) = do.rows_of(i420, (2, 2), do.RGBA)
    assert row0.tolist() == [255, 255, 255, 255, 0, 0, 0, 255]
    r, g, b = do.rgba_from_yuv([82, 144], 128, 128)
    assert row1.tolist() == [r[0], g[0], b[0], 255, r[1], g[1], b[1], 255]


def test_interleaved_chroma_rows():
    i420 = np.arange(4 * 2 + 2 + 2, dtype=np.uint8)   # 4x2: Y 0..7, U 8 9, V 10 11
    assert [r.tolist() for _, r in do.rows_of(i420, (4, 2), do.NV12)][2] == [8, 10, 9, 11]
    assert [r.tolist() for _, r in do.rows_of(i420, (4, 2), do.NV21)][2] == [10, 8, 11, 9]
    assert [r.tolist() for _, r in do.rows_of(i420, (4, 2), do.I420)][2:] == [[8, 9], [10, 11]]


@pytest.mark.parametrize("row_align", [1, 16, 64, 256])
@pytest.mark.parametrize("lay", do.LAYOUTS)
def test_layout_properties(lay, row_align):
    sizes = [(46, 30), None, (50, 34), (14, 16), (1920, 1080), (18, 18)]
    desc, total = do.layout(sizes, lay, row_align)
    end = 0
    for size, d in zip(sizes, desc):
        if size is None:
            assert d["offset"] == -1
            continue
        w, h = size
        row = 4 * w if lay == do.RGBA else w
        assert d["offset"] % 256 == 0 and d["offset"] >= end and d["offset"] - end < 256      # 256-byte starts, no overlap, no gap of 256
        assert d["stride"] % row_align == 0 and row <= d["stride"] < row + row_align
        if lay == do.I420:
            assert d["chroma_stride"] % row_align == 0 and w // 2 <= d["chroma_stride"] < w // 2 + row_align
            n = d["stride"] * h + 2 * d["chroma_stride"] * (h // 2)
        elif lay == do.RGBA:
            assert d["chroma_stride"] == 0
            n = d["stride"] * h
        else:
            assert d["chroma_stride"] == d["stride"]
            n = d["stride"] * (h + h // 2)
        assert do.geometry(w, h, lay, row_align)[2] == n
        end = d["offset"] + n
    assert total == end
    if row_align == 1 and lay == do.I420:   # the tight form is the I420 picture itself
        assert do.geometry(46, 30, lay, 1) == (46, 23, 46 * 30 * 3 // 2)


def test_pack_writes_rows_and_nothing_else():
    rng = np.random.default_rng(5)
    pics = [(rng.integers(0, 256, 46 * 30 * 3 // 2, dtype=np.uint8), (46, 30)), None, (rng.integers(0, 256, 18 * 18 * 3 // 2, dtype=np.uint8), (18, 18))]
    for lay in do.LAYOUTS:
        for ra in (1, 64):
            buf, written, desc, total = do.pack(pics, lay, ra, size=None)
            assert buf.size == total and desc[1]["offset"] == -1
            want = sum((4 if lay == do.RGBA else 1) * w * h * (1 if lay == do.RGBA else 3) // (1 if lay == do.RGBA else 2) for _, (w, h) in (p for p in pics if p))
            assert int(written.sum()) == want
            assert (buf[~written] == 0xA5).all()
    tight, _, _, _ = do.pack(pics[:1], do.I420, 1)
    assert np.array_equal(tight, pics[0][0])


def _window(plane, crop, w, h):
    return plane[crop[1]:crop[1] + h, crop[0]:crop[0] + w]


def test_case_list_holds_what_the_gpu_tests_rely_on():
    names = [c.name for c in do.CASES]
    assert len(set(names)) == len(names) and {"out_50x34", "out_18x18", "twelve_96x80", "forty_32x32", "five_64x48", "sixtyfour_32x32"} <= set(names)
    assert len(do.BY_NAME["sixtyfour_32x32"].streams) == 64
    for name, sizes in (("out_50x34", [(46, 30), (50, 34), (50, 34), (46, 30)]), ("out_18x18", [(14, 16), (18, 18)])):
        case = do.BY_NAME[name]
        got = [do.pictures(case, k)[0][3] for k in range(len(case.streams))]
        assert got == sizes, (name, got)                      # two different cropped sizes in one group
        assert any(w % 4 for w, _ in got)                     # widths that are no multiple of 4
        for k in range(len(case.streams)):
            for _, planes, i420, size in do.pictures(case, k):
                assert planes[0].shape == ((48, 64) if name == "out_50x34" else (32, 32))
    # a stream whose crop origin is not (0, 0) in both axes: its cropped luma lies in the coded plane at an origin with x > 0 and
    # y > 0, and the window at (0, 0) differs (a build that ignores the origin fails the GPU test on it)
    shifted = 0
    for name in ("out_50x34", "out_18x18"):
        case = do.BY_NAME[name]
        for k in range(len(case.streams)):
            for _, planes, i420, (w, h) in do.pictures(case, k):
                y = i420[:w * h].reshape(h, w)
                at = [(cx, cy) for cy in range(0, planes[0].shape[0] - h + 1, 2) for cx in range(0, planes[0].shape[1] - w + 1, 2)
                      if np.array_equal(_window(planes[0], (cx, cy), w, h), y)]
                if at and all(cx > 0 and cy > 0 for cx, cy in at):
                    assert not np.array_equal(_window(planes[0], (0, 0), w, h), y)
                    shifted += 1
    assert shifted >= 2
    # a stream whose picture before a step it sits out is a non-reference picture (its next picture lands in the same ring slot),
    # under the schedules the GPU test uses
    found = 0
    for name, sched in do.SCHEDULES.items():
        case = do.BY_NAME[name]
        S = len(case.streams)
        nxt, sat_out_after_nonref, some_sit_out = [0] * S, 0, 0
        for t in range(8 * case.pictures):
            part = [k for k in range(S) if nxt[k] < case.pictures and sched(t, k)]
            some_sit_out += 0 < len(part) < S
            for k in range(S):
                if k not in part and 0 < nxt[k] < case.pictures and part and not do.facts(case, k)[nxt[k] - 1]["is_ref"]:
                    sat_out_after_nonref += 1
            for k in part:
                nxt[k] += 1
        assert min(nxt) == case.pictures, name          # the schedule finishes
        assert some_sit_out, name                        # calls in which some streams sit out
        found += sat_out_after_nonref
    assert found >= 1
