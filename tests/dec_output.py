"""Decoder output in four layouts (include/mi355x_h264_dec.h: mi355x_h264_dec_read, _dec_group_read_all, _set_output, _output;
media_amd/csrc/k_dec_out.h): the case list and the restatement in Python that tests/test_dec_output_oracle.py (CPU: what the list
holds, the restatement against known answers) and tests/test_gpu_dec_output.py (GPU) share.

The restatement is the specification once more, from the header's words alone: pictures in stream order, each at an offset
rounded up to 256 bytes; a luma row, an NV12 / NV21 chroma row and an RGBA row have stride align_up(row bytes, row_align), an I420
chroma row align_up(width / 2, row_align); plane heights are tight.  RGBA is integer BT.601 studio swing with the chroma sample of
a 2x2 block serving its four pixels.  The expected samples are the oracle decoder's cropped I420 pictures
(dec_group.stream_pictures)."""
import numpy as np

import dec_group as dg
from dec_group import R, E, Case, N, PS, QP, CQ, IDC, SUB, OH

I420, NV12, NV21, RGBA = 0, 1, 2, 3
LAYOUTS = (I420, NV12, NV21, RGBA)
LAYOUT_NAMES = {I420: "i420", NV12: "nv12", NV21: "nv21", RGBA: "rgba"}

# names key dec_group's cache: new ones.  Coded 64x48 with two cropped sizes, two of them cropped left and top as well (PS: parameter
# sets by id, with frame cropping on the left and top); widths 46, 50, 14, 18 are no multiples of 4
CASES = [
    Case("out_50x34", 50, 34, 4, [R(100, 0, 2, PS | QP | CQ | SUB, 3, 71), R(66, 2, 1, QP | IDC, 4, 72), E(66, 0, 1, "s1", 3, 28), R(77, 0, 3, N | PS | OH | QP, 4, 73)]),
    Case("out_18x18", 18, 18, 3, [R(66, 0, 1, PS | QP, 3, 81), R(100, 0, 1, QP, 3, 82)]),
    dg.BY_NAME["twelve_96x80"],
    dg.BY_NAME["forty_32x32"],
    dg.BY_NAME["five_64x48"],
    # the position table at its limit: 64 copies of one stream
    Case("sixtyfour_32x32", 32, 32, 3, [dg.FORTY[0]] * 64),
]
BY_NAME = {c.name: c for c in CASES}


def pictures(case, k):
    """dec_group.stream_pictures; the 64 copies are one stream, made once"""
    return dg.stream_pictures(case, 0 if case.name == "sixtyfour_32x32" else k)


def facts(case, k):
    return dg.stream_facts(case, 0 if case.name == "sixtyfour_32x32" else k)


def align_up(v, a):
    return (v + a - 1) // a * a


def geometry(w, h, layout, row_align):
    """(stride, chroma stride, bytes) of one picture"""
    if layout == RGBA:
        s = align_up(4 * w, row_align)
        return s, 0, s * h
    s = align_up(w, row_align)
    if layout == I420:
        c = align_up(w // 2, row_align)
        return s, c, s * h + 2 * c * (h // 2)
    return s, s, s * h + s * (h // 2)


def layout(sizes, lay, row_align):
    """sizes: (width, height) per stream, None for a stream without a picture.  Returns ([descriptor per stream], total bytes);
    a descriptor has offset (-1: no picture), width, height, stride, chroma_stride"""
    assert row_align in (1, 2, 4, 8, 16, 32, 64, 128, 256)
    out, total = [], 0
    for size in sizes:
        if size is None:
            out.append({"offset": -1, "width": 0, "height": 0, "stride": 0, "chroma_stride": 0})
            continue
        w, h = size
        s, c, n = geometry(w, h, lay, row_align)
        off = align_up(total, 256)
        out.append({"offset": off, "width": w, "height": h, "stride": s, "chroma_stride": c})
        total = off + n
    return out, total


def rgba_from_yuv(y, u, v):
    """(R, G, B) of samples (arrays or numbers) by the stated formula; the shift is arithmetic"""
    y, u, v = (np.asarray(a).astype(np.int32) for a in (y, u, v))
    c, d, e = 298 * (y - 16), u - 128, v - 128
    clip = lambda a: np.clip(a, 0, 255).astype(np.uint8)
    return clip((c + 409 * e + 128) >> 8), clip((c - 100 * d - 208 * e + 128) >> 8), clip((c + 516 * d + 128) >> 8)


def planes_of(i420, size):
    w, h = size
    y = i420[:w * h].reshape(h, w)
    u = i420[w * h:w * h + (w // 2) * (h // 2)].reshape(h // 2, w // 2)
    v = i420[w * h + (w // 2) * (h // 2):].reshape(h // 2, w // 2)
    return y, u, v


def rows_of(i420, size, lay):
    """the picture as the list of its destination rows: (which stride: 0 luma / 1 chroma, bytes of the row)"""
    y, u, v = planes_of(i420, size)
    if lay == RGBA:
        up = lambda p: np.repeat(np.repeat(p, 2, axis=0), 2, axis=1)
        r, g, b = rgba_from_yuv(y, up(u), up(v))
        px = np.stack([r, g, b, np.full_like(r, 255)], axis=-1).reshape(y.shape[0], -1)
        return [(0, row) for row in px]
    rows = [(0, row) for row in y]
    if lay == I420:
        return rows + [(1, row) for row in u] + [(1, row) for row in v]
    a, b = (u, v) if lay == NV12 else (v, u)
    return rows + [(1, np.stack([ra, rb], axis=-1).ravel()) for ra, rb in zip(a, b)]


def pack(pics, lay, row_align, size=None, fill=0xA5):
    """pics: (cropped I420, (width, height)) per stream or None.  Returns (buffer, written, descriptors, total): the expected
    output inside a buffer of `size` bytes (default: total) pre-filled with `fill`, and which of its bytes the output defines"""
    desc, total = layout([None if p is None else p[1] for p in pics], lay, row_align)
    buf = np.full(total if size is None else size, fill, np.uint8)
    written = np.zeros(buf.size, bool)
    for p, d in zip(pics, desc):
        if p is None:
            continue
        at = d["offset"]
        for kind, row in rows_of(p[0], p[1], lay):
            buf[at:at + row.size] = row
            written[at:at + row.size] = True
            at += d["chroma_stride"] if kind else d["stride"]
    return buf, written, desc, total


# which streams take part in call t (the others sit it out): the schedule of test_streams_that_sit_out_and_empty_units for the five
# streams (stream 0 has non-reference pictures), and one for the cropped case (stream 3 has them)
SCHEDULES = {
    "five_64x48": lambda t, k: (t * 7 + k * 3) % 5 < 2 or (t % 6 == 5 and k == 2) or t > 30,
    "out_50x34": lambda t, k: (t + k) % 3 != 0 or t > 12,
}
