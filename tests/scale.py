"""Scaled streams (include/mi355x_h264.h, mi355x_h264_stream_open_scaled): the arithmetic restated in numpy from the words of the
header alone, the case list and the content that tests/test_scale_oracle.py (CPU) and tests/test_gpu_scale.py (GPU) share.

Area resampling of a plane of SW x SH samples to W x H: result sample x covers [x SW, (x + 1) SW) on an axis where source sample i
covers [i W, (i + 1) W); the weight is the integer length of the overlap, at most 5 source samples are touched, and
out = floor((N + (D >> 1)) / D) with N the doubly weighted sum and D = SW SH.  The restatement works on TAP LISTS (index and weight
of the up to five taps of every result sample), vectorised over the taps - no dense matrix.  Everything is a closed formula or a
fixed seed, computed once per process, shared and never changed."""
import functools
from collections import namedtuple
import numpy as np
import value_cube
from media_amd import synth

TAPS = 5
I420, NV12, RGBA = 0, 1, 2


def taps(S, D):
    """the tap lists of an axis of S source samples resampled to D: (index (D, 5), weight (D, 5)), int64; taps past the last one
    of a result sample have weight 0 (and an index held inside the axis)"""
    x = np.arange(D, dtype=np.int64)[:, None]
    lo, hi = x * S, (x + 1) * S
    i = lo // D + np.arange(TAPS, dtype=np.int64)[None, :]
    w = np.clip(np.minimum(hi, (i + 1) * D) - np.maximum(lo, i * D), 0, None)
    assert ((hi - 1) // D < lo // D + TAPS).all(), "more than five taps: a ratio above 4"
    return np.minimum(i, S - 1), w


def numerators(src, W, H):
    """(N (H, W) int64, D) of a plane src (SH, SW): nothing is rounded between the horizontal and the vertical sum"""
    SH, SW = src.shape
    assert W <= SW <= 4 * W and H <= SH <= 4 * H
    ix, wx = taps(SW, W)
    iy, wy = taps(SH, H)
    s = np.asarray(src).astype(np.int64)
    hs = np.zeros((SH, W), np.int64)
    for t in range(TAPS):
        hs += s[:, ix[:, t]] * wx[None, :, t]
    n = np.zeros((H, W), np.int64)
    for t in range(TAPS):
        n += hs[iy[:, t]] * wy[:, t, None]
    return n, SW * SH


def scale_plane(src, W, H):
    n, D = numerators(src, W, H)
    out = (n + (D >> 1)) // D
    assert out.min() >= 0 and out.max() <= 255
    return out.astype(np.uint8)


def planes_i420(f, w, h):
    f = np.asarray(f).ravel()
    return f[: w * h].reshape(h, w), f[w * h: w * h * 5 // 4].reshape(h // 2, w // 2), f[w * h * 5 // 4:].reshape(h // 2, w // 2)


def scale_i420(f, sw, sh, w, h):
    """tight I420 sw x sh -> tight I420 w x h"""
    y, u, v = planes_i420(f, sw, sh)
    return value_cube.i420_of(scale_plane(y, w, h), scale_plane(u, w // 2, h // 2), scale_plane(v, w // 2, h // 2))


def to_nv12(f, w, h):
    y, u, v = planes_i420(f, w, h)
    return np.concatenate([y.ravel(), np.stack([u, v], axis=2).ravel()])


def scale_nv12(f, sw, sh, w, h):
    """tight NV12 sw x sh -> tight I420 w x h: the chroma samples taken from the interleaved plane"""
    f = np.asarray(f).ravel()
    y, uv = f[: sw * sh].reshape(sh, sw), f[sw * sh:].reshape(sh // 2, sw // 2, 2)
    return value_cube.i420_of(scale_plane(y, w, h), scale_plane(uv[..., 0], w // 2, h // 2), scale_plane(uv[..., 1], w // 2, h // 2))


def scale_rgba(p, w, h):
    """RGBA (sh, sw, 4) -> tight I420 w x h: R, G and B resampled as planes, then the RGBA arithmetic (value_cube.rgba_to_i420)"""
    out = np.zeros((h, w, 4), np.uint8)
    for c in range(3):
        out[..., c] = scale_plane(p[..., c], w, h)
    return value_cube.rgba_to_i420(out)


def restate(fmt, pic, sw, sh, w, h):
    if fmt == I420:
        return scale_i420(pic, sw, sh, w, h)
    if fmt == NV12:
        return scale_nv12(pic, sw, sh, w, h)
    return scale_rgba(np.asarray(pic).reshape(sh, sw, 4), w, h)


Case = namedtuple("Case", "name sw sh w h content pictures rgba")
CASES = (
    Case("2to1_64x48", 64, 48, 32, 24, "noise", 4, True),            # 2:1 ties; the coded height (32) is not the display height (24)
    Case("3to2_96x64", 96, 64, 64, 48, "noise", 4, True),            # 3:2 and 4:3
    Case("odd_70x38", 70, 38, 34, 18, "noise", 4, True),             # 3 taps; w % 4 == 2; odd chroma planes 35x19 -> 17x9
    Case("five_70x62", 70, 62, 18, 16, "noise", 4, False),           # 5 taps in both dimensions, in luma and in chroma
    Case("4to1_64x64", 64, 64, 16, 16, "noise", 4, False),           # exactly 4:1, the limit
    Case("row_66x16", 66, 16, 64, 16, "constant", 4, False),         # identity vertically, a ratio just above 1 horizontally (picture 0 constant, then noise)
    Case("mid_320x240", 320, 240, 208, 160, "pan", 4, True),         # mid size, content worth coding
    Case("hd_1920x1080", 1920, 1080, 1280, 720, "pan", 2, True),     # the product's own size; IDR + 1 P only
    Case("max_4096x4096", 4096, 4096, 1024, 1024, "bound", 1, False),   # all 255 in the top half, random below; one picture; the 2^32 bound
)
BY_NAME = {c.name: c for c in CASES}
FORMATS = {"i420": I420, "nv12": NV12, "rgba": RGBA}


def _noise(seed, n):
    return np.random.RandomState(seed).randint(0, 256, n).astype(np.uint8)


def to_rgba(f, w, h, seed):
    """an RGBA picture made from an I420 one (any will do); alpha is noise"""
    y, u, v = (p.astype(np.int32) for p in planes_i420(f, w, h))
    u, v = u.repeat(2, 0).repeat(2, 1), v.repeat(2, 0).repeat(2, 1)
    r = np.clip(y + ((359 * (v - 128)) >> 8), 0, 255)
    g = np.clip(y - ((88 * (u - 128) + 183 * (v - 128)) >> 8), 0, 255)
    b = np.clip(y + ((454 * (u - 128)) >> 8), 0, 255)
    a = np.random.RandomState(seed).randint(0, 256, (h, w))
    return np.stack([r, g, b, a], axis=2).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def source_i420(name):
    """the case's source pictures as tight I420 of the source size (read-only)"""
    c = BY_NAME[name]
    n = c.sw * c.sh * 3 // 2
    seed = 1000 + 17 * CASES.index(c)
    if c.content == "pan":
        out = [np.ascontiguousarray(f) for f in synth.sequence("s1", c.sw, c.sh, c.pictures, start=5)]
    elif c.content == "bound":
        f = _noise(seed, n)
        f[: c.sw * c.sh // 2] = 255
        out = [f]
    else:
        out = [_noise(seed + i, n) for i in range(c.pictures)]
        if c.content == "constant":
            out[0] = np.full(n, 201, np.uint8)
    for f in out:
        f.setflags(write=False)
    return tuple(out)


@functools.lru_cache(maxsize=None)
def pictures(name, fmt):
    """(what the stream is handed: flat uint8 pictures of the source size in layout fmt, the restated I420 pictures of the coded size)"""
    c = BY_NAME[name]
    src = source_i420(name)
    if fmt == I420:
        pics = src
    elif fmt == NV12:
        pics = tuple(to_nv12(f, c.sw, c.sh) for f in src)
    else:
        if c.content == "pan":
            pics = tuple(to_rgba(f, c.sw, c.sh, i).ravel() for i, f in enumerate(src))
        else:   # every channel its own noise (a constant picture stays one)
            pics = tuple(np.full(c.sw * c.sh * 4, 201, np.uint8) if (c.content == "constant" and i == 0) else _noise(5000 + 31 * CASES.index(c) + i, c.sw * c.sh * 4)
                         for i in range(c.pictures))
    want = tuple(restate(fmt, p, c.sw, c.sh, c.w, c.h) for p in pics)
    for a in pics + want:
        a.setflags(write=False)
    return pics, want


def plane_shapes(c):
    """[(SW, SH, W, H)] of the planes that are resampled: luma and chroma"""
    return [(c.sw, c.sh, c.w, c.h), (c.sw // 2, c.sh // 2, c.w // 2, c.h // 2)]
