"""Saturating content at both ends of the QP range, on the CPU oracle (no GPU).

Six adversarial contents (tests/adversarial.py) x QP {10, 11, 12, 49, 50, 51} x profile x reference pictures.  For every
picture: the independent decoder (oracle/h264_dec.c) reproduces the encoder's reconstruction, the stream keeps the A.2 / A.3.1
limits (macroblock_layer() <= 3200 bits, level_prefix <= 15), and every prediction-only region equals the prediction restated
from the standard (tests/spec_pred.py).  The coverage floors then pin the content: hard minimums of how many blocks reached
each saturating path (clamped 6-tap intermediates, clamped plane predictions, level_prefix 15, TotalCoeff 16, I_PCM, vectors
outside the picture).  tests/test_gpu_saturation.py holds the HIP encoder to the same floors."""
import numpy as np
import pytest
import adversarial
import spec_pred
from oracle_lib import OracleEncoder, OracleDecoder

# Coverage of each content over its matrix (adversarial.matrix).  The oracle's counts are deterministic; the floors are
# those counts less about a tenth, so that a mode-decision change can move them a little but a tamer content cannot pass.
FLOORS = {
    "glyphs": {"inter_quadrants": 23518, "frac_x": 2286, "frac_y": 2097, "frac_xy": 1614, "j_pos": 37,
        "mc_clipped": 2235, "mv_outside": 1339, "chroma_mc_blocks": 2512, "i16_checked": 508, "i16_plane": 55,
        "i4_blocks": 12502, "chroma_intra_checked": 215, "pcm": 1134, "lp15_qp10_12": 70, "lp15_qp49_51": 11,
        "tc16": 3588, "i16_plane_mbs": 115, "mc_clipped_qp49_51": 2235},
    "checker": {"inter_quadrants": 27698, "frac_x": 846, "frac_y": 381, "frac_xy": 243, "j_pos": 1, "mc_clipped": 992,
        "mv_outside": 545, "chroma_mc_blocks": 13917, "i4_blocks": 7074, "chroma_intra_checked": 58, "pcm": 2001,
        "lp15_qp10_12": 70, "lp15_qp49_51": 19, "tc16": 865, "mc_clipped_qp49_51": 990},
    "gradient": {"inter_quadrants": 15570, "frac_x": 814, "frac_y": 1004, "frac_xy": 1812, "j_pos": 161,
        "mc_clipped": 351, "mv_outside": 154, "chroma_mc_blocks": 7740, "i16_checked": 5809, "i16_plane": 261,
        "i16_plane_clamped": 117, "i4_blocks": 12927, "chroma_intra_checked": 4989, "chroma_plane_clamped": 572,
        "pcm": 14, "lp15_qp10_12": 70, "lp15_qp49_51": 40, "tc16": 6, "i16_plane_mbs": 981, "mc_clipped_qp49_51": 288},
    "flat_flip": {"inter_quadrants": 9976, "i16_checked": 11248, "i4_blocks": 820, "chroma_intra_checked": 11313,
        "lp15_qp10_12": 58, "lp15_qp49_51": 58},
    "contrast": {"inter_quadrants": 18905, "frac_x": 2179, "frac_y": 1639, "frac_xy": 8165, "j_pos": 231,
        "mc_clipped": 757, "mv_outside": 864, "chroma_mc_blocks": 8071, "i16_checked": 57, "i16_plane": 5,
        "i16_plane_clamped": 2, "i4_blocks": 13024, "pcm": 2965, "lp15_qp10_12": 70, "tc16": 852, "i16_plane_mbs": 185,
        "mc_clipped_qp49_51": 581},
    "bars": {"inter_quadrants": 35733, "frac_x": 949, "frac_y": 428, "frac_xy": 82, "mc_clipped": 206,
        "chroma_mc_blocks": 22478, "i16_checked": 3938, "i16_plane": 3, "i4_blocks": 3175, "chroma_intra_checked": 4194,
        "lp15_qp10_12": 70, "lp15_qp49_51": 11, "i16_plane_mbs": 5, "mc_clipped_qp49_51": 206},
}


def run_oracle_stream(kind, qps, prof, refs, cov, slices=0, search=1):
    """encode PICTURES pictures of `kind`, picture i at qps[i]; check every picture; add coverage to `cov`"""
    w, h = adversarial.SIZE
    orc = OracleEncoder(w, h, qp=qps[0], gop=adversarial.GOP, profile_idc=prof, refs=refs, slices=slices, search=search)
    dec = OracleDecoder()
    srows = adversarial.slice_rows(orc.ch // 16, slices)
    history = []
    aus = []
    for i, f in enumerate(adversarial.sequence(kind, w, h, len(qps))):
        if i and qps[i] != qps[i - 1]:
            orc.set_qp(qps[i])
        au, idr = orc.encode(f)
        aus.append(au)
        tag = "%s qp %d profile %d refs %d picture %d" % (kind, qps[i], prof, refs, i)
        assert dec.decode(au) == 1, tag + ": no picture decoded"
        for p in range(3):
            got, want = dec.plane(p), orc.recon(p)
            if not np.array_equal(got, want):
                yx = np.argwhere(got != want)[0]
                raise AssertionError("%s: decoder plane %d differs from the encoder's reconstruction first at (%d, %d), mb (%d, %d)"
                                     % (tag, p, yx[1], yx[0], yx[1] // (16 >> (p > 0)), yx[0] // (16 >> (p > 0))))
        assert dec.max_mb_bits <= 3200, "%s: a macroblock of %d bits (A.3.1)" % (tag, dec.max_mb_bits)
        assert dec.max_level_prefix <= 15, "%s: level_prefix %d (A.2)" % (tag, dec.max_level_prefix)
        if idr:
            history = []
        mbinfo = orc.mbinfo()
        before = dict(cov)
        spec_pred.check_picture([orc.recon_pre(p) for p in range(3)], history, spec_pred.coded_planes(f, w, h, orc.cw, orc.ch),
                                mbinfo, orc.mvq(), orc.mbaux(), orc.levels(), srows, tag=tag, counters=cov)
        adversarial.tally(cov, qps[i], mbinfo, dec.max_level_prefix, before, cov)
        history = ([tuple(orc.recon(p) for p in range(3))] + history)[: max(refs, 1)]
    orc.close()
    dec.close()
    return aus


def check_floors(kind, cov):
    short = ["%s %d < %d" % (k, cov.get(k, 0), v) for k, v in FLOORS[kind].items() if cov.get(k, 0) < v]
    assert not short, "%s: coverage below its floor: %s (counts %s)" % (kind, ", ".join(short), cov)


@pytest.mark.parametrize("kind", list(adversarial.GENERATORS))
def test_saturating_content_at_the_qp_range_ends(kind):
    cov = {}
    for qp, prof, refs in adversarial.matrix(kind):
        run_oracle_stream(kind, [qp] * adversarial.PICTURES, prof, refs, cov)
    check_floors(kind, cov)


def test_qp_jump_10_51_10_inside_a_gop():
    """set_qp between P pictures of one GOP, 10 -> 51 -> 10: the chroma QP, the dequantisation rows and the loop filter's
    tables change from one picture to the next while the references were coded at the other end of the range"""
    qps = [10, 10, 51, 51, 10, 10]
    for kind in adversarial.GENERATORS:
        cov = {}
        run_oracle_stream(kind, qps, 100, 3, cov)
        assert cov["inter_quadrants"] > 0


@pytest.mark.parametrize("qp", [10, 51])
def test_slice_bands_and_exhaustive_search(qp):
    """three slice bands (spec_pred's availability cut at the band edges) and the exhaustive integer search beside the seeded
    one of the matrix: the cases tests/test_gpu_saturation.py runs on the HIP encoder"""
    for kind in ("glyphs", "gradient", "contrast"):
        cov = {}
        run_oracle_stream(kind, [qp] * adversarial.PICTURES, 66, 3, cov, slices=3)
        run_oracle_stream(kind, [qp] * adversarial.PICTURES, 100, 0, cov, search=0)
        assert cov["inter_quadrants"] > 0 and cov["i4_blocks"] + cov["i16_checked"] + cov["pcm"] > 0
