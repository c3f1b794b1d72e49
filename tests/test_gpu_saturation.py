"""Saturating content at both ends of the QP range through the HIP encoder (run with -m gpu on an MI355X).

The matrix of tests/test_saturation_oracle.py - six adversarial contents x QP {10, 11, 12, 49, 50, 51} x profile x reference
pictures - through capi.Encoder with the pre-filter planes kept.  For every picture: the access unit equals the oracle's, every
stage agrees with it (test_gpu_parity._compare_all), the independent decoder reproduces the GPU's reconstruction, and every
prediction-only region of the GPU's own pre-filter planes equals the prediction restated from the standard (tests/spec_pred.py),
the references being the GPU's previous reconstructions.  The coverage floors are those of the oracle test: the two paths are
bit-exact, so they count the same blocks.  Then one case each for the lockstep batch, slice bands, NV12 device input, the
exhaustive search and the GPU decoder peer."""
import numpy as np
import pytest
import adversarial
import spec_pred
from media_amd import capi, h264dec
from oracle_lib import OracleEncoder, OracleDecoder
from test_gpu_parity import _compare_all, _to_nv12

pytestmark = pytest.mark.gpu

# the floors of tests/test_saturation_oracle.py (the oracle's counts less about a tenth), the same numbers
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


def _check_gpu_picture(enc, orc, dec, f, au, want, qp, history, srows, cov, tag):
    """one picture the GPU coded: equal to the oracle's, decodable to the GPU's reconstruction, its prediction-only regions
    equal to the standard's prediction.  Returns the GPU's reconstruction (the next picture's ref_idx 0)."""
    w, h = adversarial.SIZE
    assert au == want, tag + ": access unit differs from the oracle's"
    _compare_all(enc, orc, tag)
    assert dec.decode(au) == 1, tag + ": no picture decoded"
    recon = tuple(enc.debug_read(capi.DBG_RECON_Y + p) for p in range(3))
    for p in range(3):
        assert np.array_equal(dec.plane(p), recon[p]), "%s: decoder plane %d differs from the GPU reconstruction" % (tag, p)
    assert dec.max_mb_bits <= 3200 and dec.max_level_prefix <= 15, tag
    mbinfo = enc.debug_read(capi.DBG_MBINFO)
    before = dict(cov)
    spec_pred.check_picture([enc.debug_read(capi.DBG_PRE_Y + p) for p in range(3)], history,
                            spec_pred.coded_planes(f, w, h, enc.cw, enc.ch), mbinfo, enc.debug_read(capi.DBG_MVQ),
                            enc.debug_read(capi.DBG_MBAUX), enc.debug_read(capi.DBG_LEVELS), srows, tag=tag + " (GPU)", counters=cov)
    adversarial.tally(cov, qp, mbinfo, dec.max_level_prefix, before, cov)
    return recon


def run_gpu_stream(kind, qps, prof, refs, cov, slices=0, search=1, nv12=False):
    w, h = adversarial.SIZE
    enc = capi.Encoder(w, h, qp=qps[0], gop=adversarial.GOP, profile_idc=prof, refs=refs, slices=slices, search=search,
                       input_format=1 if nv12 else 0)
    enc.keep_pre(True)
    orc = OracleEncoder(w, h, qp=qps[0], gop=adversarial.GOP, profile_idc=prof, refs=refs, slices=slices, search=search)
    dec = OracleDecoder()
    srows = adversarial.slice_rows(enc.ch // 16, slices)
    frames = adversarial.sequence(kind, w, h, len(qps))
    if nv12:
        import torch
        dev = torch.from_numpy(np.stack([_to_nv12(f, w, h) for f in frames])).cuda()
    history, aus = [], []
    for i, f in enumerate(frames):
        if i and qps[i] != qps[i - 1]:
            enc.set_qp(qps[i])
            orc.set_qp(qps[i])
        au, ft = enc.encode_device(dev[i].data_ptr()) if nv12 else enc.encode(f)
        want, idr = orc.encode(f)
        assert (ft == capi.FRAME_IDR) == idr
        if idr:
            history = []
        tag = "%s qp %d profile %d refs %d slices %d search %d%s picture %d" % (kind, qps[i], prof, refs, slices, search,
                                                                               " nv12" if nv12 else "", i)
        recon = _check_gpu_picture(enc, orc, dec, f, au, want, qps[i], history, srows, cov, tag)
        history = ([recon] + history)[: max(refs, 1)]
        aus.append(au)
    enc.close()
    orc.close()
    dec.close()
    return aus


@pytest.mark.parametrize("kind", list(adversarial.GENERATORS))
def test_gpu_saturating_content_at_the_qp_range_ends(kind):
    cov = {}
    for qp, prof, refs in adversarial.matrix(kind):
        run_gpu_stream(kind, [qp] * adversarial.PICTURES, prof, refs, cov)
    short = ["%s %d < %d" % (k, cov.get(k, 0), v) for k, v in FLOORS[kind].items() if cov.get(k, 0) < v]
    assert not short, "%s: coverage below its floor: %s (counts %s)" % (kind, ", ".join(short), cov)


def test_gpu_qp_jump_10_51_10_inside_a_gop():
    for kind in adversarial.GENERATORS:
        run_gpu_stream(kind, [10, 10, 51, 51, 10, 10], 100, 3, {})


@pytest.mark.parametrize("qp", [10, 51])
def test_gpu_slice_bands_exhaustive_search_and_nv12(qp):
    """slice bands (3 slices: intra and vector neighbours cut at the band edges), the exhaustive integer search beside the
    seeded one of the matrix, and device-resident NV12 pictures of saturated chroma bars"""
    for kind in ("glyphs", "gradient", "contrast"):
        run_gpu_stream(kind, [qp] * adversarial.PICTURES, 66, 3, {}, slices=3)
        run_gpu_stream(kind, [qp] * adversarial.PICTURES, 100, 0, {}, search=0)
    cov = {}
    run_gpu_stream("bars", [qp] * adversarial.PICTURES, 100, 3, cov, nv12=True)
    assert cov["chroma_mc_blocks"] > 0


@pytest.mark.parametrize("G,qp", [(2, 51), (3, 10)])
def test_gpu_lockstep_batch_of_adversarial_gops(G, qp):
    """encode_gops_device: G closed GOPs of different adversarial contents in one lockstep batch concatenate to the oracle's
    serial stream, which the independent decoder decodes within the A.2 / A.3.1 limits"""
    import torch
    w, h = adversarial.SIZE
    gop, fbytes = 3, w * h * 3 // 2
    kinds = list(adversarial.GENERATORS)
    frames = []
    for g in range(G):
        frames += adversarial.sequence(kinds[(g + qp) % len(kinds)], w, h, gop, start=g)
    orc = OracleEncoder(w, h, qp=qp, gop=gop, profile_idc=100)
    want = [orc.encode(f)[0] for f in frames]
    dev = torch.from_numpy(np.stack(frames)).cuda()
    enc = capi.Encoder(w, h, qp=qp, gop=gop, profile_idc=100, batch=G)
    cap = 4 * gop * fbytes
    out, sizes, gb = np.zeros(G * cap, np.uint8), np.zeros(G * gop, np.uint32), np.zeros(G, np.uint64)
    enc.encode_gops_device(dev.data_ptr(), fbytes, gop * fbytes, gop, out, cap, sizes, gb)
    enc.close()
    dec = OracleDecoder()
    for g in range(G):
        assert out[g * cap: g * cap + int(gb[g])].tobytes() == b"".join(want[g * gop:(g + 1) * gop]), "GOP %d" % g
        for t in range(gop):
            assert dec.decode(want[g * gop + t]) == 1
            assert dec.max_mb_bits <= 3200 and dec.max_level_prefix <= 15, "GOP %d picture %d" % (g, t)


@pytest.mark.parametrize("kind", list(adversarial.GENERATORS))
def test_gpu_decoder_peer_on_saturating_streams(kind):
    """the GPU decoder peer (media_amd/h264dec.py) decodes the HIP encoder's streams of saturating content at QP 10 and 51
    to the encoder's reconstruction"""
    w, h = adversarial.SIZE
    for qp, prof, refs in ((10, 100, 3), (51, 66, 0)):
        enc = capi.Encoder(w, h, qp=qp, gop=adversarial.GOP, profile_idc=prof, refs=refs)
        dec = h264dec.Decoder()
        for i, f in enumerate(adversarial.sequence(kind, w, h, adversarial.PICTURES)):
            au = enc.encode(f)[0]
            assert dec.decode(au), "%s qp %d picture %d" % (kind, qp, i)
            for p in range(3):
                assert np.array_equal(dec.plane(p), enc.debug_read(capi.DBG_RECON_Y + p)), "%s qp %d picture %d plane %d" % (kind, qp, i, p)
        dec.close()
        enc.close()
