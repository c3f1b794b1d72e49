"""The decoder's RGBA output under a colour description, on the GPU (include/mi355x_h264_dec.h, "colour"; k_dec_out.h): the 16
pictures of the YUV cube (tests/value_cube.py) go through the real decoder as I_PCM access units (tests/pcm_stream.py) under a
sequence parameter set of each description, written by tests/colour.py's writer and spliced in place of pcm_stream's; every RGBA
byte from Decoder.read, DecoderGroup.read_all and an armed group's output equals the restated inverse of that variant.  Then what
names the variant, the override, four descriptions in one launch, streams that say nothing the library has numbers for, the way
from an RGBA picture through a described encoder stream and back, and the decoder plugin."""
import functools

import numpy as np
import pytest

import colour as col
import pcm_stream
import value_cube as vc
from media_amd import capi, h264dec
from media_amd import videodecoder as vd
from oracle_lib import OracleDecoder

pytestmark = pytest.mark.gpu
N = vc.N
RGBA = h264dec.PIX_RGBA
IDS = [col.NAMES[v] for v in col.VARIANTS]


def unit(planes, vui, coded=None, seed=0):
    """the I_PCM access unit of a picture under an SPS with this VUI (None: pcm_stream's own SPS, no VUI); coded = (cw, ch, left,
    top) embeds the picture as the cropped part of a larger coded one"""
    h, w = planes[0].shape
    if coded is None:
        au, crop, (cw, ch) = pcm_stream.access_unit(*planes), None, (w, h)
    else:
        cw, ch, left, top = coded
        au, _ = pcm_stream.cropped_unit(planes, cw, ch, left, top, seed)
        crop = (left, cw - w - left, top, ch - h - top)
    return au if vui is None else col.replace_sps(au, col.pcm_sps(cw // 16, ch // 16, vui, crop=crop))


def same(got, planes, variant, what):
    """got: tight RGBA bytes of one picture; the restated inverse of the variant, the first wrong pixel named by its triple"""
    h, w = planes[0].shape
    want = col.rgba_picture(*planes, variant)
    why = vc.explain_rgba(np.asarray(got).reshape(h, w, 4), want, *planes)
    assert not why, "%s (%s): %s" % (what, col.NAMES[variant], why)


@functools.lru_cache(maxsize=None)
def cube_unit(k, variant):
    return unit(vc.yuv_cube(k), col.described_vui(*variant))


@pytest.mark.parametrize("part", range(4))
@pytest.mark.parametrize("variant", col.VARIANTS, ids=IDS)
def test_every_yuv_triple_through_the_described_rgba_output(variant, part):
    """all 2^24 (Y, U, V) per variant: four cube pictures per case, each out through Decoder.read, through an armed group's output
    and through the group's read_all"""
    dec, grp = h264dec.Decoder(), h264dec.DecoderGroup(2)
    try:
        grp.set_output(RGBA, 1)
        for k in range(4 * part, 4 * part + 4):
            planes = vc.yuv_cube(k)
            au = cube_unit(k, variant)
            assert dec.decode(au)
            for p in range(3):
                assert np.array_equal(dec.plane(p), planes[p]), "cube picture %d: plane %d is not the one given" % (k, p)
            c = dec.colour()
            assert (c["described"], c["matrix"], c["full_range"]) == (1,) + variant, c
            got, pic = dec.read(RGBA, 1)
            assert pic["bytes"] == 4 * N * N and pic["colour"] == col.colour_word(variant), pic
            same(got, planes, variant, "cube picture %d, Decoder.read" % k)
            assert grp.decode([None, au]) == [(0, 0), (0, 1)]
            data, pics = grp.output(0)
            assert pics[0]["offset"] == -1 and pics[1]["offset"] == 0 and pics[1]["colour"] == col.colour_word(variant), pics
            same(data[:4 * N * N], planes, variant, "cube picture %d, armed output" % k)
            got, pics = grp.read_all(RGBA, 1)
            assert pics[1]["colour"] == col.colour_word(variant) and grp.read_bytes == 4 * N * N
            same(got, planes, variant, "cube picture %d, read_all" % k)
    finally:
        dec.close()
        grp.close()


EDGE = [(w, h) + v for (w, h) in vc.EDGE_SIZES[1:] for v in vc.EDGE_CODED[(w, h)]]


@pytest.mark.parametrize("edge", EDGE, ids=["%dx%d_in_%dx%d_at_%d_%d" % e for e in EDGE])
def test_edge_pictures_and_the_override(edge):
    """extreme triples at widths with w % 4 == 2, cropped (the sample-by-sample branch of rgba_chunk), under each description; the
    override changes the bytes to the overridden variant's from the next read on, and null puts them back; other layouts say 0"""
    w, h, cw, ch, left, top = edge
    dec = h264dec.Decoder()
    try:
        for i, planes in enumerate(vc.edge_yuv(w, h)[:2]):
            for variant in col.VARIANTS:
                assert dec.decode(unit(planes, col.described_vui(*variant), (cw, ch, left, top), seed=i))
                assert dec.info() == (w, h, cw, ch)
                got, pic = dec.read(RGBA, 1)
                assert pic["colour"] == col.colour_word(variant)
                same(got, planes, variant, "picture %d" % i)
                assert dec.read(h264dec.PIX_NV12, 1)[1]["colour"] == 0 and dec.read(h264dec.PIX_I420, 1)[1]["colour"] == 0
                for forced in col.VARIANTS:
                    dec.set_rgba_colour(col.WORDS[forced])
                    got, pic = dec.read(RGBA, 1)
                    assert pic["colour"] == col.colour_word(forced)
                    same(got, planes, forced, "picture %d described %s, overridden" % (i, col.NAMES[variant]))
                    c = dec.colour()     # what the stream says is not what is applied
                    assert (c["matrix"], c["full_range"]) == variant
                dec.set_rgba_colour(None)
                got, pic = dec.read(RGBA, 1)
                assert pic["colour"] == col.colour_word(variant)
                same(got, planes, variant, "picture %d, following the stream again" % i)
        for bad in ((2, 0), (6, 2)):
            with pytest.raises(capi.EncoderError) as ei:
                dec.set_rgba_colour(bad)
            assert ei.value.rc == capi.E_ARG
        same(dec.read(RGBA, 1)[0], planes, variant, "after a refused override")
    finally:
        dec.close()


def test_four_descriptions_in_one_launch():
    """a group of four streams with four different descriptions in ONE step: each stream gets its own variant from one launch,
    through read_all and through the armed output; a group override holds for its stream alone"""
    w, h, coded = 50, 34, (64, 48, 2, 2)
    pics = vc.edge_yuv(w, h)
    planes = [pics[k % len(pics)] for k in range(4)]
    grp = h264dec.DecoderGroup(4)
    try:
        grp.set_output(RGBA, 64)
        aus = [unit(planes[k], col.described_vui(*col.VARIANTS[k]), coded, seed=k) for k in range(4)]
        assert grp.decode(aus) == [(0, 1)] * 4
        step = grp.last_step()
        assert step["pictures"] == 4 and (step["output_launches"], step["output_transfers"]) == (1, 1), step
        data, armed = grp.output(0)
        got, pics_ = grp.read_all(RGBA, 1)
        assert grp.last_step()["read_launches"] == 1, grp.last_step()
        for k in range(4):
            v = col.VARIANTS[k]
            assert pics_[k]["colour"] == armed[k]["colour"] == col.colour_word(v), (k, pics_[k], armed[k])
            assert (grp.colour(k)["matrix"], grp.colour(k)["full_range"]) == v
            same(got[pics_[k]["offset"]:pics_[k]["offset"] + 4 * w * h], planes[k], v, "stream %d, read_all" % k)
            rows = np.lib.stride_tricks.as_strided(data[armed[k]["offset"]:], (h, 4 * w), (armed[k]["stride"], 1))
            same(np.ascontiguousarray(rows), planes[k], v, "stream %d, armed output" % k)
        grp.set_rgba_colour(2, ("bt709", "full"))
        got, pics_ = grp.read_all(RGBA, 1)
        assert grp.last_step()["read_launches"] == 1
        for k in range(4):
            v = (col.BT709, 1) if k == 2 else col.VARIANTS[k]
            assert pics_[k]["colour"] == col.colour_word(v)
            same(got[pics_[k]["offset"]:pics_[k]["offset"] + 4 * w * h], planes[k], v, "stream %d, stream 2 overridden" % k)
        grp.set_rgba_colour(2, None)
        assert grp.decode(aus) == [(0, 1)] * 4      # the armed step after the override is gone again
        data, armed = grp.output(0)
        assert [a["colour"] for a in armed] == [col.colour_word(v) for v in col.VARIANTS]
        with pytest.raises(capi.EncoderError):
            grp.set_rgba_colour(4, None)             # no such stream
    finally:
        grp.close()


def test_streams_that_say_nothing_the_library_has_numbers_for():
    """matrix codes 0, 2 and 9, a video signal type without a description, a damaged VUI and no VUI at all: BT.601 limited, as
    before there were descriptions; code 5 has the BT.601 numbers, with the range the stream names"""
    planes = (np.ascontiguousarray(vc.yuv_cube(9)[0][300:364, 100:164]), np.ascontiguousarray(vc.yuv_cube(9)[1][150:182, 50:82]),
              np.ascontiguousarray(vc.yuv_cube(9)[2][150:182, 50:82]))
    cases = [(None, col.DEFAULT, 0, 2)] + [(col.described_vui(m, 1), col.variant_of(m, 1), 1, m) for m in col.UNKNOWN_MATRICES]
    cases += [({"pic_struct": 0, "signal": {"video_format": 5, "full_range": 1}}, col.DEFAULT, 0, 2),
              (dict(col.described_vui(1, 1), chroma_loc=(6, 0)), col.DEFAULT, 0, 2)]           # out of range: the whole VUI counts as absent
    assert [c[1] for c in cases[1:5]] == [col.DEFAULT, col.DEFAULT, (col.BT601, 1), col.DEFAULT]
    dec = h264dec.Decoder()
    try:
        for vui, variant, described, matrix in cases:
            assert dec.decode(unit(planes, vui))
            c = dec.colour()
            assert (c["described"], c["matrix"]) == (described, matrix), (vui, c)
            got, pic = dec.read(RGBA, 1)
            assert pic["colour"] == col.colour_word(variant), (vui, pic)
            same(got, planes, variant, "VUI %s" % (vui,))
    finally:
        dec.close()


def flat_block_picture(w, h, seed):
    """RGBA with one colour per 8x8 block: what survives coding well enough to keep every variant's output apart"""
    rng = np.random.RandomState(seed)
    blocks = rng.randint(0, 256, ((h + 7) // 8, (w + 7) // 8, 4)).astype(np.uint8)
    return np.ascontiguousarray(blocks.repeat(8, 0).repeat(8, 1)[:h, :w])


@pytest.mark.parametrize("variant", col.VARIANTS, ids=IDS)
def test_from_rgba_through_a_described_stream_and_back(variant):
    """Stream(colour=v, input_format=RGBA) into a DecoderGroup: the RGBA output is the restated inverse of v applied to the planes
    the oracle's independent decoder makes of the same access units, exactly - and not what any other variant would give"""
    w, h = 50, 34
    s = capi.Stream(w, h, qp=24, gop=3, input_format=capi.INPUT_RGBA, colour=col.WORDS[variant])
    grp, orc = h264dec.DecoderGroup(2), OracleDecoder()
    try:
        for i in range(4):
            p = flat_block_picture(w, h, 10 * i + variant[0] + variant[1])
            bs, _ = s.encode_rgba(p)
            assert orc.decode(bs) == 1
            assert grp.decode([bs, None]) == [(0, 1), (0, 0)]
            planes = tuple(orc.cropped(pl) for pl in range(3))
            c = grp.colour(0)
            prim = 1 if variant[0] == col.BT709 else 6
            assert c == {"described": 1, "matrix": variant[0], "full_range": variant[1], "primaries": prim, "transfer": prim, "chroma_loc": 1, "fps": 30,
                         "reorder": 0}, c
            got, pics = grp.read_all(RGBA, 1)
            assert pics[0]["colour"] == col.colour_word(variant) and pics[1]["offset"] == -1
            same(got, planes, variant, "picture %d" % i)
            for other in col.VARIANTS:
                if other != variant:
                    assert not np.array_equal(got.reshape(h, w, 4), col.rgba_picture(*planes, other))
    finally:
        s.close()
        grp.close()
        orc.close()


def test_decoder_plugin_gives_rgba_of_the_described_variant():
    """libVideoDecoder.so with the out port set to PIXEL_FORMAT_RGBA_8888 follows the stream; the default port format is unchanged"""
    w, h = 64, 48
    y, u, v = vc.yuv_cube(5)
    planes = (np.ascontiguousarray(y[500:500 + h, 200:200 + w]), np.ascontiguousarray(u[250:250 + h // 2, 100:100 + w // 2]),
              np.ascontiguousarray(v[250:250 + h // 2, 100:100 + w // 2]))
    d = vd.PluginDecoder()
    try:
        assert d.rc_create == vd.SUCCESS and d.create_decoder() == vd.SUCCESS and d.init() == vd.SUCCESS
        assert d.port_format(vd.OUT_PORT) == (vd.SUCCESS, vd.PIXEL_FORMAT_YUV_420P)
        assert d.set_port_format(vd.OUT_PORT, 3) == vd.SET_PARAMS_FAIL and d.set_port_format(vd.IN_PORT, vd.PIXEL_FORMAT_RGBA_8888) == vd.SET_PARAMS_FAIL
        assert d.set_port_format(vd.OUT_PORT, vd.PIXEL_FORMAT_RGBA_8888) == vd.SUCCESS
        assert d.port_format(vd.OUT_PORT) == (vd.SUCCESS, vd.PIXEL_FORMAT_RGBA_8888)
        assert d.set_pic_info(w, h) == vd.SUCCESS and d.start() == vd.SUCCESS
        for vui, variant in [(col.described_vui(*x), x) for x in col.VARIANTS] + [(None, col.DEFAULT), (None, col.DEFAULT), (col.described_vui(9, 1), col.DEFAULT)]:
            assert d.send(unit(planes, vui)) == vd.SUCCESS
            rc, got = d.retrieve(4 * w * h)
            assert rc == vd.SUCCESS and got.size == 4 * w * h
            same(got, planes, variant, "plugin, VUI %s" % (vui,))
            report, _ = d.colour()
            assert (report[0], report[1]) == ((1, vui["signal"]["colour"][2]) if vui else (0, 2))
        assert d.colour()[1] == 6, "one change (one INFO line) per new description: the second undescribed picture is none"
        assert d.stop() == vd.SUCCESS
    finally:
        d.delete()
