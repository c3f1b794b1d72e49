"""Decoder output at a requested size (include/mi355x_h264_dec.h, "output size"; media_amd/csrc/k_dec_out_scale.h): the case list
and the expected output that tests/test_dec_scale_oracle.py (CPU: what the list holds) and tests/test_gpu_dec_scale.py (GPU) share.

No arithmetic is stated here.  The expected output of a call is dec_output.pack() of the oracle decoder's cropped pictures
(dec_output.pictures), each resampled by scale.scale_i420() to the size its stream is given: the packing restated in
tests/dec_output.py, the resampling restated in tests/scale.py.  Streams are the cached cases of tests/dec_output.py."""
import functools
from collections import namedtuple

import dec_output as do
import scale

# target: the output size of a stream by its cropped size (the streams of a case differ in their crops); every target can be made
# from its source (W <= w <= 4 W, H <= h <= 4 H: scale.numerators asserts it)
Case = namedtuple("Case", "name source target note")
CASES = (
    Case("50_to_26x18", "out_50x34", {(50, 34): (26, 18), (46, 30): (26, 18)}, "ratios just below 2; crops on the left and top"),
    Case("50_to_14x10", "out_50x34", {(50, 34): (14, 10), (46, 30): (14, 8)}, "five taps in both dimensions, luma and chroma; W % 4 == 2; chroma 7x5"),
    Case("50_w_identity", "out_50x34", {(50, 34): (50, 18), (46, 30): (46, 16)}, "one identity dimension, for the 46-wide streams too"),
    Case("18_to_6x6", "out_18x18", {(18, 18): (6, 6), (14, 16): (6, 6)}, "chroma 9 -> 3, 7 -> 3"),
    Case("18_to_16x10", "out_18x18", {(18, 18): (16, 10), (14, 16): (12, 10)}, "ratios just above 1"),
    Case("18_identity", "out_18x18", {(18, 18): (18, 18), (14, 16): (14, 16)}, "identity: the new kernel gives k_dec_out's bytes"),
    Case("96_to_48x40", "twelve_96x80", {(96, 80): (48, 40), (94, 78): (48, 40), (92, 76): (48, 40)}, "2 : 1 ties"),
    Case("96_to_64x60", "twelve_96x80", {(96, 80): (64, 60), (94, 78): (64, 60), (92, 76): (64, 60)}, "3 : 2 and 4 : 3"),
    Case("96_to_24x20", "twelve_96x80", {(96, 80): (24, 20), (94, 78): (24, 20), (92, 76): (24, 20)}, "exactly 4 : 1, the limit"),
    Case("32_to_8x8", "forty_32x32", {(32, 32): (8, 8)}, "40 positions, 4 : 1"),
)
BY_NAME = {c.name: c for c in CASES}
TIES, FIVE, IDENTITY_DIM, IDENTITY = "96_to_48x40", "50_to_14x10", "50_w_identity", "18_identity"
ROW_ALIGNS = (1, 16, 256)
STEPS = 3   # pictures of a case the GPU tests walk through (an IDR picture and what follows it)

# the mixed group: five_64x48 with streams at the native size (None) and at three other sizes
MIXED = ("five_64x48", (None, (32, 24), (48, 36), None, (16, 12)))


def source(case):
    return do.BY_NAME[case.source]


def size_of(case, k):
    """the cropped size of stream k (every picture of a stream has it)"""
    return do.pictures(source(case), k)[0][3]


def target_of(case, k):
    return case.target[size_of(case, k)]


@functools.lru_cache(maxsize=None)
def scaled(source_name, k, t, W, H):
    """picture t of stream k of a dec_output case as tight I420 of W x H (read-only)"""
    _, _, i420, (w, h) = do.pictures(do.BY_NAME[source_name], k)[t]
    out = scale.scale_i420(i420, w, h, W, H)
    out.setflags(write=False)
    return out


def expected_pics(source_name, targets, last, only=None):
    """what dec_output.pack() takes: per stream None or (I420 at the size delivered, that size).  targets[k]: the stream's output
    size or None (native); last[k]: the index of its last decoded picture or None; only: the streams of the call"""
    case = do.BY_NAME[source_name]
    out = []
    for k in range(len(case.streams)):
        if last[k] is None or (only is not None and k not in only):
            out.append(None)
        elif targets[k] is None:
            out.append((do.pictures(case, k)[last[k]][2], do.pictures(case, k)[last[k]][3]))
        else:
            out.append((scaled(source_name, k, last[k], *targets[k]), tuple(targets[k])))
    return out


def targets(case):
    return [target_of(case, k) for k in range(len(source(case).streams))]


def plane_shapes(case, k):
    """[(SW, SH, W, H)] of the planes that are resampled for stream k: luma and chroma"""
    (w, h), (W, H) = size_of(case, k), target_of(case, k)
    return [(w, h, W, H), (w // 2, h // 2, W // 2, H // 2)]
