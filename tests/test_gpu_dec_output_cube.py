"""Decoder output on the GPU over every (Y, U, V) (tests/value_cube.py): the YUV cube's pictures go through the real decoder as
I_PCM access units (tests/pcm_stream.py: no prediction, no transform, no loop filter - the planes in the ring are the planes given)
and come out through k_dec_out (media_amd/csrc/k_dec_out.h).  Expected bytes: tests/dec_output.pack() of the same picture, the
header's formula restated; every comparison is exact, and a wrong RGBA pixel is named with the triple it was made from.  The edge
pictures - extreme triples at widths with w % 4 == 2, cropped on the right and bottom or on all four sides - run the
sample-by-sample branches of rgba_chunk and weave_chunk through Decoder.read, DecoderGroup.read_all and an armed group."""
import numpy as np
import pytest

import dec_output as do
import pcm_stream
import value_cube as vc
from media_amd import h264dec

pytestmark = pytest.mark.gpu
N = vc.N
FILL = 0xA5


def same_rgba(got, want, planes, w, h, stride, what):
    """got / want: one picture's bytes, rows `stride` apart; only the rows' own bytes are compared"""
    g = np.lib.stride_tricks.as_strided(got, (h, 4 * w), (stride, 1)).reshape(h, w, 4)
    t = np.lib.stride_tricks.as_strided(want, (h, 4 * w), (stride, 1)).reshape(h, w, 4)
    why = vc.explain_rgba(g, t, *planes)
    assert not why, "%s: %s" % (what, why)


@pytest.mark.parametrize("part", range(4))
def test_every_yuv_triple_through_the_rgba_output(part):
    """all 2^24 (Y, U, V) through rgba_pixel in the full-chunk path: four pictures of the cube per case"""
    dec = h264dec.Decoder()
    try:
        for k in range(4 * part, 4 * part + 4):
            planes = vc.yuv_cube(k)
            assert dec.decode(pcm_stream.access_unit(*planes))
            assert dec.info() == (N, N, N, N)
            for p in range(3):
                assert np.array_equal(dec.plane(p), planes[p]), "cube picture %d: plane %d is not the one given" % (k, p)
            want, written, desc, total = do.pack([(vc.i420_of(*planes), (N, N))], do.RGBA, 1)
            assert total == 4 * N * N and written.all()
            got, pic = dec.read(do.RGBA, 1)
            assert pic["bytes"] == total and pic["stride"] == 4 * N
            same_rgba(got, want, planes, N, N, 4 * N, "cube picture %d" % k)
            assert np.array_equal(got, want)
    finally:
        dec.close()


def test_one_cube_picture_in_the_copying_layouts():
    """I420, NV12 and NV21 are copies: value coverage is not the point, one picture is enough"""
    import torch
    planes = vc.yuv_cube(6)
    i420 = vc.i420_of(*planes)
    dec = h264dec.Decoder()
    try:
        assert dec.decode(pcm_stream.access_unit(*planes))
        assert np.array_equal(dec.i420(), i420)
        for lay in (do.I420, do.NV12, do.NV21):
            for ra in (1, 64):
                want, written, desc, total = do.pack([(i420, (N, N))], lay, ra)
                got, pic = dec.read(lay, ra)
                assert pic["bytes"] == total and np.array_equal(got[written], want[written]), (lay, ra)
            dev = torch.full((total + 64,), FILL, dtype=torch.uint8, device="cuda")
            dec.read(lay, 64, device_tensor=dev)
            assert np.array_equal(dev.cpu().numpy(), do.pack([(i420, (N, N))], lay, 64, size=total + 64, fill=FILL)[0]), lay
    finally:
        dec.close()


# ---- edge pictures ----
VARIANTS = [(w, h) + v for (w, h) in vc.EDGE_SIZES for v in vc.EDGE_CODED[(w, h)]]
VARIANT_IDS = ["%dx%d_in_%dx%d_at_%d_%d" % v for v in VARIANTS]
_units = {}


def units(variant):
    """[(access unit, cropped I420, planes)] of the edge pictures of one variant: made once, shared by the three ways out"""
    if variant not in _units:
        w, h, cw, ch, left, top = variant
        out = []
        for i, planes in enumerate(vc.edge_yuv(w, h)):
            au, _ = pcm_stream.cropped_unit(planes, cw, ch, left, top, 7 * i + left)
            i420 = vc.i420_of(*planes)
            i420.setflags(write=False)
            out.append((au, i420, planes))
        _units[variant] = out
    return _units[variant]


def check_packed(got, pics, lay, ra, what, written_only=True, size=None):
    """got: the bytes of an output of `pics` ((cropped I420, size, planes) per stream or None).  The written bytes must be the
    restatement's; with written_only False every other byte must still be the fill (device destinations)"""
    want, written, desc, total = do.pack([None if p is None else p[:2] for p in pics], lay, ra, size=size, fill=FILL)
    assert got.size == want.size, (what, got.size, want.size)
    if lay == do.RGBA:   # name the first wrong pixel
        for k, (p, d) in enumerate(zip(pics, desc)):
            if p is not None:
                w, h = p[1]
                same_rgba(got[d["offset"]:], want[d["offset"]:], p[2], w, h, d["stride"], "%s, stream %d" % (what, k))
    assert np.array_equal(got[written], want[written]), what
    if not written_only:
        assert np.array_equal(got, want), "%s: bytes between the rows or behind the output were written" % what
    return desc, total


@pytest.mark.parametrize("variant", VARIANTS, ids=VARIANT_IDS)
def test_edge_pictures_through_decoder_read(variant):
    import torch
    w, h = variant[:2]
    dec = h264dec.Decoder()
    try:
        for i, (au, i420, planes) in enumerate(units(variant)):
            assert dec.decode(au)
            assert dec.info() == (w, h, variant[2], variant[3])
            for lay in (do.RGBA, do.NV12, do.NV21):   # (NV12 / NV21: weave_chunk's sample-by-sample branch)
                for ra in (1, 64):
                    what = "picture %d layout %s row_align %d" % (i, do.LAYOUT_NAMES[lay], ra)
                    got, pic = dec.read(lay, ra)
                    desc, total = check_packed(got, [(i420, (w, h), planes)], lay, ra, what)
                    assert pic["bytes"] == total and all(pic[k] == desc[0][k] for k in ("offset", "width", "height", "stride", "chroma_stride"))
                    dev = torch.full((total + 64,), FILL, dtype=torch.uint8, device="cuda")
                    dec.read(lay, ra, device_tensor=dev)
                    check_packed(dev.cpu().numpy(), [(i420, (w, h), planes)], lay, ra, what + " (device)", written_only=False, size=total + 64)
    finally:
        dec.close()


def group_steps(variant, grp):
    """three streams walk the variant's pictures, each from its own start; in step t stream t % 3 sits out.  Yields
    (t, part, last): who took part and every stream's last picture (cropped I420, size, planes) or None"""
    U = units(variant)
    w, h = variant[:2]
    P = len(U)
    todo = [[(n + (P // 3 + 1) * k) % P for n in range(P)] for k in range(3)]
    last = [None] * 3
    t = 0
    while any(todo):
        part = [k for k in range(3) if k != t % 3 and todo[k]]
        if not part:   # (only the stream whose turn it is to sit out has pictures left)
            t += 1
            continue
        idx = {k: todo[k].pop(0) for k in part}
        res = grp.decode([U[idx[k]][0] if k in part else None for k in range(3)])
        assert all(res[k] == ((0, 1) if k in part else (0, 0)) for k in range(3)), res
        for k in part:
            last[k] = (U[idx[k]][1], (w, h), U[idx[k]][2])
        yield t, part, list(last)
        t += 1
    assert t >= P


@pytest.mark.parametrize("variant", VARIANTS, ids=VARIANT_IDS)
def test_edge_pictures_through_group_read_all(variant):
    import torch
    grp = h264dec.DecoderGroup(3)
    try:
        for t, part, last in group_steps(variant, grp):
            for ra in (1, 64):
                what = "step %d row_align %d" % (t, ra)
                got, pics = grp.read_all(do.RGBA, ra)
                desc, total = check_packed(got, last, do.RGBA, ra, what)
                assert grp.read_bytes == total
                for k in range(3):
                    assert all(pics[k][key] == desc[k][key] for key in ("offset", "width", "height", "stride", "chroma_stride")), (what, k)
                    if last[k] is not None:
                        assert pics[k]["fresh"] == (1 if k in part else 0)
                dev = torch.full((total + 256,), FILL, dtype=torch.uint8, device="cuda")
                grp.read_all(do.RGBA, ra, device_tensor=dev)
                check_packed(dev.cpu().numpy(), last, do.RGBA, ra, what + " (device)", written_only=False, size=total + 256)
    finally:
        grp.close()


@pytest.mark.parametrize("variant", VARIANTS, ids=VARIANT_IDS)
def test_edge_pictures_through_an_armed_group(variant):
    for ra in (1, 64):
        grp = h264dec.DecoderGroup(3)
        try:
            grp.set_output(do.RGBA, ra)
            for t, part, last in group_steps(variant, grp):
                step = grp.last_step()
                assert (step["output_launches"], step["output_transfers"]) == (1, 1), step
                data, pics = grp.output(0)
                only = [last[k] if k in part else None for k in range(3)]
                desc, total = check_packed(data, only, do.RGBA, ra, "armed step %d row_align %d" % (t, ra))
                for k in range(3):
                    assert (pics[k]["offset"] >= 0) == (k in part)
                    assert all(pics[k][key] == desc[k][key] for key in ("offset", "width", "height", "stride", "chroma_stride")), (t, k)
        finally:
            grp.close()
