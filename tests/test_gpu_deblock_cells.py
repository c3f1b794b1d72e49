"""The decoder's loop filter (k_deblock_rows<.., PERMB>: thresholds per edge from the two macroblocks' QPs, the filter offsets and
the chroma offsets; filt_uni; the wave-uniform skip of whole edges) on the streams of tests/deblock_cells.py, which
tests/test_deblock_cells_oracle.py proves to change samples at every (plane kind, bS, indexA 16 .. 51), to filter at every indexB
and to meet every branch of 8.7.2.3 / 8.7.2.4.  The oracle's independent decoder says what every picture decodes to: integers, no
tolerance."""
import numpy as np
import pytest

import deblock_cells as D
import mem_guard as mg
from media_amd import h264dec

pytestmark = pytest.mark.gpu


def first_difference(got, want, w, tag, row):
    """None, or the first wrong sample of the picture: plane, position, values, its macroblock, the edges of the 4x4 grid it lies
    within three samples of, and the schedule row"""
    for p in range(3):
        if np.array_equal(got[p], want[p]):
            continue
        ys, xs = np.nonzero(got[p] != want[p])
        y, x = int(ys[0]), int(xs[0])
        s, g = (16, 4) if p == 0 else (8, 4)
        mb = (y // s) * ((w + 15) // 16) + x // s
        edges = []
        for name, v in (("vertical", x % s), ("horizontal", y % s)):
            e = (v + g // 2) // g % (s // g)   # the nearest edge of the grid (edge 0 of the next macroblock when past the last)
            edges.append("%s edge %d" % (name, e if p == 0 else 2 * e))
        return ("%s plane %d: %d samples differ, first at (x %d, y %d): %d, the independent decoder has %d; macroblock %d, nearest %s; %s"
                % (tag, p, ys.size, x, y, int(got[p][y, x]), int(want[p][y, x]), mb, " / ".join(edges),
                   "random syntax" if row is None else "QP %d (coded at %d) oa %d ob %d idc %d" % (row.qp, row.coded, row.oa, row.ob, row.idc)))
    return None


def run_single(case):
    """[planes per picture] of a Decoder of the case's own; asserts each against the independent decoder"""
    dec, out = h264dec.Decoder(), []
    try:
        for i, pic in enumerate(D.stream(case)):
            assert dec.decode(pic.au), "%s picture %d" % (case.name, i)
            got = [dec.plane(p) for p in range(3)]
            bad = first_difference(got, pic.planes, case.w, "%s picture %d (%s)" % (case.name, i, "IDR" if pic.idr else "P"), pic.row)
            assert bad is None, bad
            out.append(got)
    finally:
        dec.close()
    return out


@pytest.mark.parametrize("case", D.CASES, ids=[c.name for c in D.CASES])
def test_decoder_equals_the_independent_decoder_in_every_cell(case):
    run_single(case)


GROUP = ("main_00_66_split", "main_02_100_s1", "rand_64x48_66_ends", "chroma_00_100_contrast", "low_66_split", "clip_66_gradient")
SITS_OUT = (3, 4)     # stream, step


def run_group():
    cases = [D.BY_NAME[n] for n in GROUP]
    assert {(c.w, c.h) for c in cases} == {(64, 48)} and sum(c.kind == "rand" for c in cases) == 1
    want = [D.stream(c) for c in cases]
    single = [run_single(c) for c in cases]
    S = len(cases)
    at = [0] * S
    mixed = offsets = 0
    grp = h264dec.DecoderGroup(S)
    try:
        for t in range(D.PICTURES + 1):
            part = [k for k in range(S) if at[k] < len(want[k]) and (k, t) != SITS_OUT]
            if not part:
                break
            res = grp.decode([want[k][at[k]].au if k in part else None for k in range(S)])
            assert all(res[k] == (0, 1) for k in part) and grp.last_step()["pictures"] == len(part), (t, res, [grp.error(k) for k in range(S)])
            pics = [want[k][at[k]] for k in part]
            intra = [bool(np.isin(p.kinds, (1, 2, 3)).any()) for p in pics]
            mixed += any(intra) and not all(intra)
            offsets += len({(p.row.oa, p.row.ob) for p in pics if p.row is not None}) > 1
            for k in part:
                got = grp.debug_planes(k)
                tag = "step %d stream %d (%s) picture %d" % (t, k, cases[k].name, at[k])
                bad = first_difference(got, want[k][at[k]].planes, 64, tag, want[k][at[k]].row)
                assert bad is None, bad
                assert all(np.array_equal(got[p], single[k][at[k]][p]) for p in range(3)), tag + ": differs from the single decoder"
                at[k] += 1
        assert at == [len(w) for w in want]
        assert mixed >= 4 and offsets >= 8, "steps with and without intra macroblocks, and with different offsets per position: %d, %d" % (mixed, offsets)
    except BaseException:
        grp.close()
        raise
    return grp


def test_group_of_six_streams_at_different_schedule_rows():
    """six 64x48 streams in one DecoderGroup, each at its own schedule rows, a random stream among them, stream 3 sitting step 4
    out: steps hold pictures with and without intra macroblocks (both need_intra launches) under different offsets per position.
    Per stream the result equals a Decoder's and the independent decoder's"""
    run_group().close()


def test_under_guard_mode():
    """two cases and the group with 262144 guard bytes around every block and poison: every guard intact"""
    with mg.guarded() as seen:
        for name in ("main_16_77_contrast", "rand_96x80_100"):
            run_single(D.BY_NAME[name])
        grp = run_group()
        try:
            assert grp.mem_check()[0] == 0
        finally:
            grp.close()
    mg.clean(seen, kinds=["decoder", "group"])
