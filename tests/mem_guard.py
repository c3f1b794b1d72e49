"""The guarded runs' list and plumbing (tests/test_gpu_mem_guard.py): the guard mode of the library's own memory
(include/mi355x_h264.h, mi355x_h264_debug_mem_guard) switched on around the existing small case lists.

GUARD is a condition, not a measurement: it holds one whole macroblock row of the largest per-macroblock array at the widest
tested picture (2048x16: 128 macroblocks of 832 bytes of levels = 104 KiB) and 16 luma rows there (32 KiB).  A store that is off by
one macroblock, one row of macroblocks or one sample row therefore lands in a guard.  NOT claimed: a store that is off by a whole
item or plane stride can fly over any guard, and a read out of bounds is never seen this way.

guarded() is the one way in: it sets the switch (poison on), and - because the existing runners create and close their owners
themselves - wraps the close() of the four binding classes so that every owner is checked just before it goes.  It restores
everything in a finally.  clean() then asserts what the issue asks of every guarded run."""
import contextlib
import gc

import numpy as np

import stream_matrix as sm
from media_amd import capi, h264dec, synth

GUARD = 262144

# Floors of the regions one check must have examined, counted from the allocations in the source (two regions per block, one per
# plane, item and ring slot of the zeroed ring slack):
#   encoder: picture store 12 blocks + engine 14 + 3 access-unit slots of 4 = 38 blocks, ring slack 3 planes x 1 item x 2 slots
#   stream:  hub 2 + at least 2 step contexts of 2 = 6 blocks, its engine 12 + 14 + 1 slot of 4 = 30; slack 3 x 32 items x 2 slots
#   decoder / group: store 12 blocks + 16 pinned arrays + 5 device arrays + 3 tables + 3 lists of large levels = 39; slack 3 x 1 x 4
FLOOR = {"encoder": 2 * 38 + 6, "stream": 2 * 36 + 192, "decoder": 2 * 39 + 12, "group": 2 * 39 + 12}

DIRECT_SIZES = tuple(s for s in sm.FIXED_SIZES[:7])   # stream_matrix.FIXED_SIZES without the adversarial size
assert DIRECT_SIZES == ((16, 16), (32, 16), (16, 48), (18, 18), (50, 34), (130, 98), (2048, 16))


def direct_cases():
    """(name, kind, w, h, qp, profile, search, slices, refs, door): the fixed sizes with profile, search, slices and reference
    count in turn, host I420 with padded rows in half of them and NV12 from an odd device address in the others; then a noise
    picture at QP 10 (I_PCM, unfiltered) and a `cut` sequence (intra macroblocks in P pictures) at 50x34"""
    out = []
    for c, (w, h) in enumerate(DIRECT_SIZES):
        slices = 3 if (w, h) in ((130, 98), (16, 48)) else 0      # (16x48 has too few rows for three: the clamp to one slice)
        out.append(("%dx%d" % (w, h), "s1", w, h, 26, (66, 77, 100)[c % 3], c & 1, slices, 3 if c % 2 else 1, "nv12_device" if c % 2 else "host_padded"))
    out.append(("noise_50x34", "noise", 50, 34, 10, 66, 1, 0, 1, "host_padded"))
    out.append(("cut_50x34", "cut", 50, 34, 28, 100, 1, 0, 3, "nv12_device"))
    return out


def direct_frames(kind, w, h, n=4):
    if kind == "noise":
        return [sm._noise(w, h, i) for i in range(n)]
    return synth.sequence(kind, w, h, n)


class Checks(list):
    """what the wrapped close() calls saw: (kind, damaged regions, regions examined, report lines)"""
    tally_before = 0


@contextlib.contextmanager
def guarded(guard=GUARD, poison=True):
    was = capi.mem_guard(guard, poison)
    seen = Checks()
    seen.tally_before = capi.mem_tally()
    classes = ((capi.Encoder, "encoder"), (capi.Stream, "stream"), (h264dec.Decoder, "decoder"), (h264dec.DecoderGroup, "group"))
    originals = [(cls, cls.close) for cls, _ in classes]

    def wrap(cls, kind, orig):
        def close(self):
            if getattr(self, "h", None):
                try:
                    seen.append((kind,) + self.mem_check())
                except capi.EncoderError as e:
                    if e.rc != capi.E_ARG:   # (E_ARG: an owner from before the switch that happens to go now; it does not
                        raise                # count - clean() wants its number of guarded checks at their floor)
            orig(self)
        cls.close = close

    try:
        for (cls, kind), (_, orig) in zip(classes, originals):
            wrap(cls, kind, orig)
        yield seen
    finally:
        gc.collect()   # (owners left to their __del__ go through the wrapped close as well)
        for cls, orig in originals:
            cls.close = orig
        capi.mem_guard(*was)


def header(lines):
    """(blocks, ring slack regions) of a report's first line"""
    assert lines and lines[0].startswith("examined blocks="), lines[:1]
    a, b = lines[0].split()[1:3]
    return int(a.split("=")[1]), int(b.split("=")[1])


def clean(seen, checks=1, kinds=None):
    """every check found nothing and examined two regions per block plus the ring slack; at least `checks` of them reach the
    floor of their kind (an owner that never made its arrays - a decoder that refused its only unit - examines nothing and does
    not count); nothing was found while freeing either"""
    for kind, damaged, regions, lines in seen:
        assert damaged == 0, "%s: %d damaged regions: %s" % (kind, damaged, lines)
        blocks, slack = header(lines)
        assert regions == 2 * blocks + slack, (kind, regions, lines[0])
    full = [k for k, _, regions, _ in seen if regions >= FLOOR[k]]
    print("guarded: %d checks, regions %s" % (len(seen), [(k, r) for k, _, r, _ in seen]))
    assert len(full) >= checks, "only %d of %d checks reached their floor: %s" % (len(full), len(seen), [(k, r) for k, _, r, _ in seen])
    if kinds:
        assert set(kinds) <= set(full), (kinds, full)
    assert capi.mem_tally() == seen.tally_before, "damage was found while blocks were freed (MI355X_H264_MEM_GUARD_LOG=<file> names it)"


def luma_sse(recon_y, frame, w, h):
    src = np.asarray(frame[: w * h], np.int64).reshape(h, w)
    return int(((recon_y[:h, :w].astype(np.int64) - src) ** 2).sum())
