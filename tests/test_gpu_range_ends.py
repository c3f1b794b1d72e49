"""The decoder peer on the GPU at the ends of the QP, level and vector ranges: the streams of tests/range_ends.py
(tests/test_range_ends_oracle.py proves on the CPU what they hold and that they are conforming).  QP_Y 0 .. 51 in every kind of
residual (k_dec_resid, intra_mb_core<DEC>: every row of the dequantiser tables, chroma qPi clipped at both ends), the largest
levels level_prefix 15 and 16 code and whole blocks of levels just beyond a signed byte (put_level, Picture::big, k_dec_patch,
the growth of the lists of large levels), vectors at the limits of A.3.1 with reference blocks wholly outside the picture on every
side (mc_luma4, chroma_fetch4).  The oracle's independent decoder says what every picture decodes to: integer kernels, no
tolerance."""
import numpy as np
import pytest

import range_ends as R
from media_amd import h264dec

pytestmark = pytest.mark.gpu


def differences(got, pic, w, tag):
    """the planes of one picture against the independent decoder's; a difference names the macroblock, its type and its QP"""
    bad = []
    for p in range(3):
        want = pic.planes[p]
        if not np.array_equal(got[p], want):
            ys, xs = np.nonzero(got[p] != want)
            s = 16 if p == 0 else 8
            k = (int(ys[0]) // s) * ((w + 15) // 16) + int(xs[0]) // s
            bad.append("%s (%s) plane %d: %d samples differ, first in macroblock %d (type %d, QP %d)"
                       % (tag, "IDR" if pic.idr else "P", p, ys.size, k, int(pic.mb["type"][k]), int(pic.mbqp[k])))
    return bad


@pytest.mark.parametrize("case", R.CASES, ids=[c.name for c in R.CASES])
def test_decoder_equals_the_independent_decoder_at_the_range_ends(case):
    dec = h264dec.Decoder()
    for i, pic in enumerate(R.stream(case)):
        assert dec.decode(pic.au), "%s picture %d" % (case.name, i)
        bad = differences([dec.plane(p) for p in range(3)], pic, case.w, "%s picture %d" % (case.name, i))
        assert not bad, bad
    dec.close()


def test_group_of_four_streams_and_the_growth_of_the_lists_of_large_levels():
    """R.GROUP: four 96x80 streams, the third written without the new bit.  Every stream's picture of every step equals the
    independent decoder's and what a Decoder of its own gives that stream.  The memory the group holds (last_step's device_bytes /
    pinned_bytes) rises at the two steps whose large levels outgrow the lists - R.GROUP_GROWTH, which the CPU test derives from
    the streams - and at no other step."""
    S = len(R.GROUP)
    want = [R.stream(c) for c in R.GROUP]
    single = []
    for k in range(S):
        d = h264dec.Decoder()
        single.append([])
        for pic in want[k]:
            assert d.decode(pic.au)
            single[k].append([d.plane(p) for p in range(3)])
        d.close()
    grp = h264dec.DecoderGroup(S)
    bad, held = [], []
    for t in range(R.PICTURES):
        res = grp.decode([want[k][t].au for k in range(S)])
        step = grp.last_step()
        assert res == [(0, 1)] * S and step["pictures"] == S, (t, res, [grp.error(k) for k in range(S)])
        for k in range(S):
            got = grp.debug_planes(k)
            bad += differences(got, want[k][t], R.GROUP[k].w, "step %d stream %d (%s)" % (t, k, R.GROUP[k].name))
            if not all(np.array_equal(got[p], single[k][t][p]) for p in range(3)):
                bad.append("step %d stream %d: differs from the single decoder" % (t, k))
        step = grp.last_step()   # (after the step's reads: what they stage is held from the first step on)
        held.append((step["device_bytes"], step["pinned_bytes"]))
    grp.close()
    assert not bad, bad[:8]
    rises = [tuple(t for t in range(1, R.PICTURES) if held[t][j] > held[t - 1][j]) for j in range(2)]
    assert rises[0] == R.GROUP_GROWTH and rises[1] == R.GROUP_GROWTH, (rises, held)
    assert all(held[t][j] >= held[t - 1][j] for t in range(1, R.PICTURES) for j in range(2)), held
