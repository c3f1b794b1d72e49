"""The decoder's prediction (k_dec_inter_pos / mc_luma4 with chroma_fetch4 / chroma_pred4: a vector per 4x4 block, a reference
picture per 8x8 quadrant; intra_mb_core<DEC> under k_pintra_rows<true, true>: neighbour availability from the parser's bits) on the
streams of tests/pred_cells.py, which tests/test_pred_cells_oracle.py proves to meet every cell of the oracle decoder's prediction
account at least eight times: every luma and chroma fraction, every relation of a window to the picture's edges, every Clip1 of the
interpolation, every Intra4x4 / Intra16x16 / chroma mode under every availability the standard allows, intra macroblocks beside
inter ones.  The oracle's independent decoder says what every picture decodes to: integers, no tolerance."""
import numpy as np
import pytest

import mem_guard as mg
import pred_cells as P
from media_amd import h264dec

pytestmark = pytest.mark.gpu


def first_difference(got, pic, case, tag):
    """None, or the first wrong sample of the picture: plane, position, values, and what the independent decoder's side information
    says about it (P.describe: macroblock, kind, vector / fractions / reference index / edge relation, or mode / availability)"""
    cw, ch = pic.planes[0].shape[1], pic.planes[0].shape[0]
    for p in range(3):
        if np.array_equal(got[p], pic.planes[p]):
            continue
        ys, xs = np.nonzero(got[p] != pic.planes[p])
        y, x = int(ys[0]), int(xs[0])
        return "%s plane %d: %d samples differ, first at (x %d, y %d): %d, the independent decoder has %d; %s" % (
            tag, p, ys.size, x, y, int(got[p][y, x]), int(pic.planes[p][y, x]), P.describe(pic, cw, ch, p, x, y))
    return None


def run_single(case):
    """[planes per picture] of a Decoder of the case's own; asserts each against the independent decoder"""
    dec, out = h264dec.Decoder(), []
    try:
        for i, pic in enumerate(P.stream(case)):
            assert dec.decode(pic.au), "%s picture %d" % (case.name, i)
            got = [dec.plane(p) for p in range(3)]
            bad = first_difference(got, pic, case, "%s picture %d (%s)" % (case.name, i, "IDR" if pic.idr else "non-IDR"))
            assert bad is None, bad
            out.append(got)
    finally:
        dec.close()
    return out


@pytest.mark.parametrize("case", P.CASES, ids=[c.name for c in P.CASES])
def test_decoder_equals_the_independent_decoder_in_every_cell(case):
    run_single(case)


GROUP = ("rand_64x48_77_r3_ci", "rand_64x48_100_r3_pc", "rand_64x48_66_r1_ci_pc", "rand_64x48_66_r2_pc_b", "rand_64x48_77_r3_ci_pc_b", "enc_64x48_66_r1_gradient_q24")
SITS_OUT = (2, 3)     # stream, step


def run_group():
    cases = [P.BY_NAME[n] for n in GROUP]
    assert {(c.w, c.h) for c in cases} == {(64, 48)} and any(c.refs == 3 for c in cases) and any(c.kind == "rand" and c.features & P.CI for c in cases)
    want = [P.stream(c) for c in cases]
    single = [run_single(c) for c in cases]
    S = len(cases)
    at = [0] * S
    mixed = 0
    grp = h264dec.DecoderGroup(S)
    try:
        for t in range(max(len(w) for w in want) + 1):
            part = [k for k in range(S) if at[k] < len(want[k]) and (k, t) != SITS_OUT]
            if not part:
                break
            res = grp.decode([want[k][at[k]].au if k in part else None for k in range(S)])
            assert all(res[k] == (0, 1) for k in part) and grp.last_step()["pictures"] == len(part), (t, res, [grp.error(k) for k in range(S)])
            intra = [bool(np.isin(want[k][at[k]].kinds, (1, 2, 3)).all()) for k in part]
            mixed += any(intra) and not all(intra)
            for k in part:
                got = grp.debug_planes(k)
                tag = "step %d stream %d (%s) picture %d" % (t, k, cases[k].name, at[k])
                bad = first_difference(got, want[k][at[k]], cases[k], tag)
                assert bad is None, bad
                assert all(np.array_equal(got[p], single[k][at[k]][p]) for p in range(3)), tag + ": differs from the single decoder"
                at[k] += 1
        assert at == [len(w) for w in want]
        assert mixed >= 1, "a step with all-intra pictures beside pictures that predict from references"
    except BaseException:
        grp.close()
        raise
    return grp


def test_group_of_six_streams():
    """six 64x48 streams in one DecoderGroup: three references, constrained_intra_pred_flag, windows at every edge, the encoder's own
    pictures; stream 2 sits step 3 out, so its IDR pictures fall beside the others' P pictures from then on.  Per stream the result
    equals a Decoder's and the independent decoder's"""
    run_group().close()


def test_under_guard_mode():
    """two cases and the group with guard bytes around every block and poison: every guard intact"""
    with mg.guarded() as seen:
        for name in ("rand_16x16_77_r3_ci_pc", "rand_112x64_100_r3_ci_pc"):
            run_single(P.BY_NAME[name])
        grp = run_group()
        try:
            assert grp.mem_check()[0] == 0
        finally:
            grp.close()
    mg.clean(seen, kinds=["decoder", "group"])
