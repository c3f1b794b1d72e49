"""Adversarial I420 content for the saturating paths of the codec: hard 0/255 edges moving by fractional samples, Nyquist
checkerboards, ramps that run into 0 and 255 plateaus, whole-picture flips, contrast-stretched texture under large global
motion and saturated chroma bars.  Deterministic and integer-only (the only non-integer step is the sine table of
media_amd/synth.py that `contrast` starts from); any even size.

Every generator is frame(width, height, index) -> contiguous uint8 I420 of width * height * 3 / 2 bytes.

The content is meant to reach what smooth sinusoids never do: 6-tap intermediates outside 0..255 before the clip (8.4.2.2.1),
Intra16x16 / chroma plane predictions that clamp (8.3.3.4, 8.3.4.4), the largest DC and chroma DC levels (level_prefix 15),
blocks with TotalCoeff 16, I_PCM macroblocks, motion vectors that reach outside the picture, and loop-filter edges both below
and above alpha.  tests/test_saturation_oracle.py pins how much of each it does reach.
"""
import numpy as np
from media_amd import synth


def _hash(seed, a, b=0):
    """integer hash of (seed, a, b) -> uint32 array (a, b integer arrays of one shape)"""
    a = np.asarray(a, dtype=np.uint64)
    b = np.asarray(b, dtype=np.uint64)
    x = a * np.uint64(0x9E3779B97F4A7C15) + b * np.uint64(0xC2B2AE3D27D4EB4F) + np.uint64(seed * 0x165667B19E3779F9 & 0xFFFFFFFFFFFFFFFF)
    x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    x = x ^ (x >> np.uint64(31))
    return (x >> np.uint64(32)).astype(np.uint32)


def _pack(y, u, v):
    return np.concatenate([np.clip(p, 0, 255).astype(np.uint8).ravel() for p in (y, u, v)])


def _glyph_mask(w, h, fx, fy, seed):
    """binary "UI / text" on a grid four times finer than the samples: (fx, fy) is the fine-grid position of sample (0, 0),
    one sample = 4 fine units.  Cells of 32 x 32 samples each hold a rectangle with fine-unit (sub-sample) corners, one
    horizontal and one vertical line one sample thick, and a row of 'characters': 1-sample strokes two samples apart."""
    X = np.arange(w, dtype=np.int64)[None, :] * 4 + fx
    Y = np.arange(h, dtype=np.int64)[:, None] * 4 + fy
    cx, cy = X // 128, Y // 128
    lx, ly = X % 128, Y % 128
    r = _hash(seed, cx, cy)
    r2 = _hash(seed + 1, cx, cy)
    rx0 = (r & 31).astype(np.int64) + 4
    ry0 = ((r >> 5) & 31).astype(np.int64) + 4
    rw = ((r >> 10) & 63).astype(np.int64) + 16
    rh = ((r >> 16) & 63).astype(np.int64) + 16
    rect = (lx >= rx0) & (lx < rx0 + rw) & (ly >= ry0) & (ly < ry0 + rh)
    hl = ((r2 & 127).astype(np.int64) // 4) * 4 + 2        # line rows / columns start half a sample off the grid
    vl = (((r2 >> 7) & 127).astype(np.int64) // 4) * 4 + 1
    hline = (ly >= hl) & (ly < hl + 4)
    vline = (lx >= vl) & (lx < vl + 4)
    ty = ((r2 >> 14) & 63).astype(np.int64) + 40           # text row: 6 samples high
    text = (ly >= ty) & (ly < ty + 24) & ((lx // 8) % 2 == 0) & (_hash(seed + 2, X // 24, cy) & 3 != 0) & (lx > 8) & (lx < 120)
    inv = (r2 >> 24) & 1 == 1                              # half the cells: light text on dark, the others the reverse
    m = rect ^ hline ^ vline ^ text
    return np.where(inv, ~m, m)


# step height of each quarter of the picture width (deblocking: below and above alpha, 0/255 is never filtered at QP 51)
GLYPH_STEPS = (40, 90, 160, 255)


def frame_glyphs(width, height, index):
    """binary UI / text content scrolling by (+5, +3) quarter samples per picture (integer and fractional positions in turn);
    the four vertical quarters of the picture draw it with steps of 40, 90, 160 and 255 around mid-grey (0/255 in the last)"""
    def plane(w, h, div, seed):
        m = _glyph_mask(w, h, (5 * index) // div, (3 * index) // div + 64, seed)
        q = np.minimum(np.arange(w) * 4 // w, 3)
        step = np.array(GLYPH_STEPS)[q][None, :]
        lo = np.where(step == 255, 0, 128 - step // 2)
        return np.where(m, lo + step, lo)
    y = plane(width, height, 1, 11)
    u = plane(width // 2, height // 2, 2, 12)
    v = 255 - plane(width // 2, height // 2, 2, 13)
    return _pack(y, u, v)


def frame_checker(width, height, index):
    """Nyquist checkerboard (0 / 255 alternating every sample) in luma and chroma, its phase flipping every picture, inside
    8x8 patches chosen by a hash; the other patches flat 0 or 255, the layout drifting one sample right per picture.
    Edges between the checker and a flat area give the largest 6-tap overshoots."""
    def plane(w, h, seed, shift):
        x = np.arange(w, dtype=np.int64)[None, :] - shift
        y = np.arange(h, dtype=np.int64)[:, None]
        r = _hash(seed, x // 8, y // 8)
        chk = ((x + y + index) & 1) * 255
        flat = np.where(r & 2, 255, 0)
        return np.where(r & 1 == 1, chk, flat)
    return _pack(plane(width, height, 21, index), plane(width // 2, height // 2, 22, index // 2),
                 plane(width // 2, height // 2, 23, index // 2))


def frame_gradient(width, height, index):
    """a global ramp, slope 4..12 per sample (changing with the picture), saturating into 0 and 255 plateaus: Intra16x16 and
    chroma plane prediction across the knees extrapolate past 0..255.  The ramp's centre moves by a few samples per picture."""
    sx = 4 + (index * 3) % 9
    sy = 12 - (index * 5) % 9
    if index & 1:
        sy = -sy

    def plane(w, h, div, sgn):
        x = np.arange(w, dtype=np.int64)[None, :] - (w // 2 + (7 * index) // div)
        y = np.arange(h, dtype=np.int64)[:, None] - (h // 2 - (3 * index) // div)
        # a second, gentler fold: the ramp reverses every 48 samples along x, so the picture holds several knees
        xf = np.abs(((x + 24 * 64) % 96) - 48) - 24
        return 128 + sgn * (sx * xf + sy * y)
    return _pack(plane(width, height, 1, 1), plane(width // 2, height // 2, 2, 1), plane(width // 2, height // 2, 2, -1))


FLAT_CYCLE = ((0, 0, 255), (255, 255, 0), (0, 0, 0), (128, 128, 128))


def frame_flat_flip(width, height, index):
    """whole pictures of luma 0 / 255 / 0 / 128 in turn, chroma 0/255 swapping: the largest DC and chroma DC levels"""
    yv, uv, vv = FLAT_CYCLE[index % 4]
    n = width * height
    return np.concatenate([np.full(n, yv, np.uint8), np.full(n // 4, uv, np.uint8), np.full(n // 4, vv, np.uint8)])


def frame_contrast(width, height, index):
    """synth's s1 texture contrast-stretched x4 around 128 and clipped, under large global motion (+13, -9) per picture: the
    vectors point outside the picture, onto saturated borders"""
    f = synth.frame_s1(width, height, index, noise=2, motion=(13, -9)).astype(np.int64)
    return _pack((f[: width * height] - 128) * 4 + 128, (f[width * height: width * height * 5 // 4] - 128) * 4 + 128,
                 (f[width * height * 5 // 4:] - 128) * 4 + 128)


# (Y, U, V) of the bars: every chroma sample at 0 or 255
BARS = ((255, 0, 0), (0, 255, 255), (76, 0, 255), (150, 255, 0), (29, 255, 0), (226, 0, 255), (0, 0, 0), (255, 255, 255))


def frame_bars(width, height, index):
    """saturated colour bars 20 samples wide scrolling right by 9 quarter samples per picture (fine grid 4x), the lower
    half of the picture holding them 5 quarter samples further on"""
    tab = np.array(BARS, dtype=np.int64)

    def plane(w, h, div, comp):
        X = np.arange(w, dtype=np.int64)[None, :] * 4 * div - (9 * index)
        X = X + np.where(np.arange(h)[:, None] * 2 >= h, 5, 0)
        k = (X // 80) % len(BARS)
        return tab[k, comp]
    return _pack(plane(width, height, 1, 0), plane(width // 2, height // 2, 2, 1), plane(width // 2, height // 2, 2, 2))


GENERATORS = {"glyphs": frame_glyphs, "checker": frame_checker, "gradient": frame_gradient, "flat_flip": frame_flat_flip,
              "contrast": frame_contrast, "bars": frame_bars}


def sequence(kind, width, height, count, start=0):
    fn = GENERATORS[kind]
    return [fn(width, height, start + i) for i in range(count)]


# ---------------------------------------------------------------- the test matrix (tests/test_saturation_oracle.py, test_gpu_saturation.py)

SIZE = (176, 144)
PICTURES = 6
GOP = 30
QPS = (10, 11, 12, 49, 50, 51)          # both ends of the QP range: every qp % 6 class at each end, QPc saturating at 51
# (profile_idc, refs): Baseline and High with one and with three reference pictures at every QP; Main (which codes the same
# macroblock layer as Baseline here) only at the two extreme QPs
CONFIGS = ((66, 0), (66, 3), (100, 0), (100, 3))
MAIN_CONFIGS = ((77, 3),)
MAIN_QPS = (10, 51)


def matrix(kind):
    """(qp, profile_idc, refs) of the streams of one content"""
    out = [(qp, prof, refs) for qp in QPS for (prof, refs) in CONFIGS]
    out += [(qp, prof, refs) for qp in MAIN_QPS for (prof, refs) in MAIN_CONFIGS]
    return out


def slice_rows(mb_rows, slices):
    """macroblock rows per slice: bands of ceil(rows / n) rows, at least two rows each (mi355x_h264_config.slices)"""
    most = max(mb_rows // 2, 1)
    n = min(max(slices, 1), most)
    return -(-mb_rows // n)


COVERAGE = ("lp15_qp10_12", "lp15_qp49_51", "tc16", "i16_plane_mbs", "mc_clipped_qp49_51")


def tally(cov, qp, mbinfo, max_level_prefix, counters_before, counters_after):
    """coverage of one picture beyond spec_pred's counters: pictures whose coded (non-I_PCM) macroblocks reached
    level_prefix 15, 4x4 blocks of coded macroblocks with TotalCoeff 16, Intra16x16 plane-mode macroblocks, and the
    clamped 6-tap intermediates of the QP 49..51 pictures"""
    for k in COVERAGE:
        cov.setdefault(k, 0)
    coded = mbinfo["type"] != 3
    if max_level_prefix >= 15:
        cov["lp15_qp10_12" if qp <= 12 else "lp15_qp49_51"] += 1
    cov["tc16"] += int((mbinfo["tc"][coded] == 16).sum())
    cov["i16_plane_mbs"] += int(((mbinfo["type"] == 0) & (mbinfo["i16_mode"] == 3)).sum())
    if qp >= 49:
        cov["mc_clipped_qp49_51"] += counters_after["mc_clipped"] - counters_before.get("mc_clipped", 0)
