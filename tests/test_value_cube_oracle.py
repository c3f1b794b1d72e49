"""What tests/value_cube.py and tests/pcm_stream.py claim, proved without a GPU: the cubes hold every triple exactly once, the oracle's
RGBA ingest (oracle/h264_rgba.c) equals the header's formula restated in numpy over the whole RGB cube, and the I_PCM access units
carry exactly the samples they were given through the oracle decoder (and are accepted by the library's own parser)."""
import numpy as np
import pytest

import dec_output as do
import pcm_stream
import value_cube as vc
from media_amd import h264dec
from oracle_lib import OracleDecoder, rgba_to_i420


def once_each(codes):
    """every 24-bit code exactly once"""
    codes = np.concatenate([np.asarray(c).ravel() for c in codes])
    return codes.size == 1 << 24 and bool((np.bincount(codes, minlength=1 << 24) == 1).all())


def code(a, b, c):
    return (a.astype(np.int64) << 16) | (b.astype(np.int64) << 8) | c.astype(np.int64)


def test_rgb_luma_cube_holds_every_triple_once_as_a_sample():
    assert once_each(code(p[..., 0], p[..., 1], p[..., 2]) for p in map(vc.rgb_luma_cube, range(vc.LUMA_PICTURES)))


def test_rgb_chroma_cube_holds_every_triple_once_as_a_block_mean():
    codes = []
    for k in range(vc.CHROMA_PICTURES):
        p = vc.rgb_chroma_cube(k)
        q = p[..., :3]
        m = q[0::2, 0::2]   # four equal samples a: the rounded mean (4 a + 2) >> 2 is a
        assert all((q[r::2, c::2] == m).all() for r, c in ((0, 1), (1, 0), (1, 1))), "picture %d: a 2x2 block is not of one colour" % k
        codes.append(code(m[..., 0], m[..., 1], m[..., 2]))
    assert once_each(codes)


def test_rounding_picture_block_sums_take_all_four_residues_in_every_channel():
    p = vc.rounding_picture().astype(np.int64)
    sums = p.reshape(vc.N // 2, 2, vc.N // 2, 2, 4).sum(axis=(1, 3))
    for c in range(3):
        assert set(np.unique(sums[..., c] % 4)) == {0, 1, 2, 3}, "channel %d" % c
    # and the cubes, as said: 0 or 2 only - what this picture is for
    for p in (vc.rgb_luma_cube(5), vc.rgb_chroma_cube(17)):
        s = p[..., :3].astype(np.int64).reshape(vc.N // 2, 2, vc.N // 2, 2, 3).sum(axis=(1, 3))
        assert set(np.unique(s % 4)) <= {0, 2}


def test_yuv_cube_holds_every_triple_once_as_a_pixel():
    up = lambda p: p.repeat(2, 0).repeat(2, 1)
    assert once_each(code(y, up(u), up(v)) for y, u, v in map(vc.yuv_cube, range(vc.YUV_PICTURES)))


@pytest.mark.parametrize("w,h", vc.EDGE_SIZES)
def test_edge_pictures_hold_every_extreme_triple_as_a_whole_block(w, h):
    want = {tuple(t) for t in vc.edge_triples().tolist()}
    assert len(want) == len(vc.EDGE_VALUES) ** 3
    assert w % 4 == 2
    seen_rgb, seen_yuv = set(), set()
    blocks = vc.edge_blocks(w, h)
    for (b, valid), p, (y, u, v) in zip(blocks, vc.edge_rgba(w, h), vc.edge_yuv(w, h)):
        assert p.shape == (h, w, 4) and y.shape == (h, w) and u.shape == v.shape == (h // 2, w // 2)
        q = p[..., :3].reshape(h // 2, 2, w // 2, 2, 3)
        one = (q == q[:, :1, :, :1]).all(axis=(1, 3, 4))
        assert one[valid].all()
        seen_rgb |= {tuple(t) for t in q[:, 0, :, 0][valid].tolist()}
        yq = y.reshape(h // 2, 2, w // 2, 2)
        assert (yq == yq[:, :1, :, :1]).all(axis=(1, 3))[valid].all()
        seen_yuv |= {tuple(t) for t in np.stack([yq[:, 0, :, 0], u, v], axis=-1)[valid].tolist()}
    assert seen_rgb == want and seen_yuv == want
    # the padding: not block-constant, and about half of it extreme
    b, valid = blocks[-1]
    if not valid.all():
        pad = vc.edge_rgba(w, h)[-1][~valid.repeat(2, 0).repeat(2, 1)]
        share = np.isin(pad, (0, 255)).mean()
        assert 0.4 < share < 0.62, share


# ---- the oracle's ingest against the header's words, over the whole cube ----
def oracle_equals_restatement(p):
    got, want = rgba_to_i420(p, p.shape[1], p.shape[0]), vc.rgba_to_i420(p)
    why = vc.explain_i420(got, want, p)
    assert not why, why


@pytest.mark.parametrize("part", range(4))
def test_oracle_ingest_equals_the_restatement_on_the_luma_cube(part):
    for k in range(4 * part, 4 * part + 4):
        oracle_equals_restatement(vc.rgb_luma_cube(k))


@pytest.mark.parametrize("part", range(4))
def test_oracle_ingest_equals_the_restatement_on_the_chroma_cube(part):
    for k in range(16 * part, 16 * part + 16):
        oracle_equals_restatement(vc.rgb_chroma_cube(k))


def test_oracle_ingest_equals_the_restatement_on_the_rounding_and_edge_pictures():
    oracle_equals_restatement(vc.rounding_picture())
    for w, h in vc.EDGE_SIZES:
        for p in vc.edge_rgba(w, h):
            oracle_equals_restatement(p)
    # rows that lie further apart than they are long: the padding is not read
    p = vc.edge_rgba(50, 34)[0]
    wide = np.random.RandomState(5).randint(0, 256, (34, 4 * 50 + 8)).astype(np.uint8)
    wide[:, :200] = p.reshape(34, 200)
    assert np.array_equal(rgba_to_i420(wide, 50, 34, stride=208), vc.rgba_to_i420(p))


def test_restatement_known_answers():
    """the restatement itself, on the primaries (the values oracle/h264_rgba.c names) and on a negative chroma sum"""
    for rgb, yuv in (((255, 255, 255), (235, 128, 128)), ((0, 0, 0), (16, 128, 128)), ((255, 0, 0), (82, 90, 240)),
                     ((0, 255, 0), (144, 54, 34)), ((0, 0, 255), (41, 240, 110))):
        p = np.zeros((2, 2, 4), np.uint8)
        p[..., :3] = rgb
        out = vc.rgba_to_i420(p)
        assert tuple(out[[0, 4, 5]]) == yuv and (out[:4] == yuv[0]).all()
    p = np.zeros((2, 2, 4), np.uint8)
    p[..., :3] = (1, 3, 0)   # Cb: (-38 - 222 + 128) / 256 = -0.52 -> floor -1 -> 127 (truncation would give 128)
    assert vc.rgba_to_i420(p)[4] == 127
    p[0, 0, :3] = (2, 3, 0)   # the mean of red: (1 + 1 + 1 + 2 + 2) >> 2 = 1, still
    assert vc.rgba_to_i420(p)[4] == 127
    p[0, 1, :3] = (2, 3, 0)   # (6 + 2) >> 2 = 2: half rounds up
    assert vc.rgba_to_i420(p)[4] == 128 + ((-76 - 222 + 128) // 256)


# ---- I_PCM access units ----
def decodes_to(au, coded, size, origin):
    dec = OracleDecoder()
    try:
        assert dec.decode(au) == 1
        assert dec.size == size and dec.crop == origin
        for p in range(3):
            assert np.array_equal(dec.plane(p), coded[p]), "plane %d" % p
        assert (dec.mb_kinds() == OracleDecoder.KIND_IPCM).all()
    finally:
        dec.close()
    par = h264dec.Parser()
    try:
        assert par.parse(au)
        i = par.info()
        assert (i["width"], i["height"], i["mbw"] * 16, i["mbh"] * 16) == size + (coded[0].shape[1], coded[0].shape[0])
        assert i["idr"] == 1 and i["has_pcm"] == 1 and i["deblock_idc"] == 1
    finally:
        par.close()


def test_ipcm_unit_of_a_yuv_cube_picture_decodes_to_its_planes():
    planes = vc.yuv_cube(9)
    au = pcm_stream.access_unit(*planes)
    assert len(au) > vc.N * vc.N * 3 // 2
    decodes_to(au, planes, (vc.N, vc.N), (0, 0))


@pytest.mark.parametrize("w,h", vc.EDGE_SIZES)
def test_ipcm_units_of_the_edge_pictures_with_and_without_crop(w, h):
    for i, planes in enumerate(vc.edge_yuv(w, h)):
        for cw, ch, left, top in vc.EDGE_CODED[(w, h)]:
            au, coded = pcm_stream.cropped_unit(planes, cw, ch, left, top, 7 * i + left)
            decodes_to(au, coded, (w, h), (left, top))
            dec = OracleDecoder()
            dec.decode(au)
            for p in range(3):
                assert np.array_equal(dec.cropped(p), planes[p])
            dec.close()
        if i == 0:   # the same coded planes without frame cropping: the whole coded picture is the picture
            decodes_to(pcm_stream.access_unit(*coded), coded, (cw, ch), (0, 0))


def test_output_restatement_names_the_first_wrong_pixel():
    y, u, v = (np.full((2, 2), 200, np.uint8), np.full((1, 1), 90, np.uint8), np.full((1, 1), 30, np.uint8))
    rows = do.rows_of(vc.i420_of(y, u, v), (2, 2), do.RGBA)
    want = np.stack([r for _, r in rows]).reshape(2, 2, 4)
    assert vc.explain_rgba(want, want, y, u, v) == ""
    got = want.copy()
    got[1, 0, 2] ^= 1
    assert "(0, 1)" in vc.explain_rgba(got, want, y, u, v) and "(200, 90, 30)" in vc.explain_rgba(got, want, y, u, v)


def test_debug_values_of_the_binding_are_the_headers():
    """capi.DBG_* against the enum of include/mi355x_h264.h, MI355X_H264_DBG_SRC = 10 among them"""
    import os
    import re
    from media_amd import capi
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "mi355x_h264.h")).read()
    values = {name: int(v) for name, v in re.findall(r"MI355X_H264_(DBG_[A-Z_]+) = (\d+)", text)}
    assert values["DBG_SRC"] == 10 and len(values) == 11
    for name, v in values.items():
        assert getattr(capi, name) == v, name
