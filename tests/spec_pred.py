"""Prediction restated from the text of ITU-T H.264 in NumPy int64, independent of oracle/ and of media_amd/:

  8.4.2.2.1  luma sample interpolation (all 16 quarter-sample positions, reference sample coordinates clipped to the picture)
  8.4.2.2.2  chroma sample interpolation (4:2:0, eighth-sample)
  8.3.1.2    Intra4x4 prediction (9 modes, with the substitution of the top-right samples)
  8.3.3      Intra16x16 prediction (4 modes, the plane mode clipped)
  8.3.4      chroma intra prediction (4 modes, DC per 4x4 block, the plane mode clipped)
  6.4.x      neighbour availability, slices being bands of whole macroblock rows

check_picture() asserts that every PREDICTION-ONLY region of a coded picture equals its prediction, computed here from the
picture's own pre-filter reconstruction (intra) or from the previous pictures' post-filter reconstructions (inter):

  * an inter 8x8 quadrant whose coded_block_pattern bit is clear, and every quadrant of a P_Skip macroblock;
  * an Intra16x16 macroblock with luma cbp 0 and all sixteen DC levels zero;
  * an Intra4x4 8x8 quadrant whose cbp bit is clear;
  * the chroma of a macroblock with cbp >> 4 == 0;
  * an I_PCM macroblock, which must equal the source samples.

It returns counters of what it checked, so that a test can pin how much of the saturating arithmetic the content reached.

Side information follows the layout the oracle and the HIP encoder share (tests/oracle_lib.py MBINFO_DTYPE): type
0 I16, 1 P16x16, 2 P_Skip, 3 I_PCM, 4 I4, 5 P16x8, 6 P8x16, 7 P8x8; for inter macroblocks chroma_mode is ref_idx_l0; mvq holds
the vectors of the four 8x8 quadrants; mbaux the sixteen Intra4x4PredModes in blkIdx order; levels 416 int16 per macroblock,
the first 16 the Intra16x16 DC levels.
"""
import numpy as np

MB_I16, MB_P16, MB_PSKIP, MB_IPCM, MB_I4, MB_P16X8, MB_P8X16, MB_P8X8 = range(8)
INTER_TYPES = (MB_P16, MB_PSKIP, MB_P16X8, MB_P8X16, MB_P8X8)

COUNTERS = ("inter_quadrants", "frac_x", "frac_y", "frac_xy", "j_pos", "mc_clipped", "mv_outside", "chroma_mc_blocks",
            "i16_checked", "i16_plane", "i16_plane_clamped", "i4_blocks", "chroma_intra_checked", "chroma_plane_clamped", "pcm")

_TAP = np.array([1, -5, 20, 20, -5, 1], dtype=np.int64)


def _clip1(v):
    return np.clip(v, 0, 255)


def _tap6(a, axis):
    """six-tap sums along `axis` of every run of six samples: output length = input length - 5"""
    n = a.shape[axis] - 5
    out = 0
    for k in range(6):
        out = out + _TAP[k] * np.take(a, np.arange(k, k + n), axis=axis)
    return out


def luma_mc(ref, x0, y0, mvx, mvy, bw=8, bh=8):
    """8.4.2.2.1 for N blocks at once.  ref: (H, W) uint8 reference picture; x0, y0: block positions (full samples); mvx,
    mvy: quarter-sample vectors.  Returns (pred (N, bh, bw) int64, out_of_range (N,) bool: an intermediate the selected
    position uses lay outside 0..255 before its Clip1, outside (N,) bool: the block's integer samples leave the picture)"""
    H, W = ref.shape
    x0, y0, mvx, mvy = (np.asarray(a, dtype=np.int64) for a in (x0, y0, mvx, mvy))
    xi, yi, xf, yf = x0 + (mvx >> 2), y0 + (mvy >> 2), mvx & 3, mvy & 3
    o_x, o_y = np.arange(-2, bw + 4), np.arange(-2, bh + 4)          # 8.4.2.2.1 eq. 8-228 / 8-229: xZL, yZL of -2 .. +3
    cols = np.clip(xi[:, None] + o_x[None, :], 0, W - 1)
    rows = np.clip(yi[:, None] + o_y[None, :], 0, H - 1)
    win = ref.astype(np.int64)[rows[:, :, None], cols[:, None, :]]    # (N, bh + 6, bw + 6); sample (dx, dy) at [2 + dy, 2 + dx]
    b1 = _tap6(win, 2)[:, :, : bw + 1]     # b1 between columns dx and dx + 1, every window row      (N, bh + 6, bw + 1)
    h1 = _tap6(win, 1)[:, : bh + 1, :]     # h1 between rows dy and dy + 1, every window column      (N, bh + 1, bw + 6)
    j1 = _tap6(b1, 1)[:, :bh, :bw]         # j1 from the b1 column (8-241)                           (N, bh, bw)
    braw = (b1[:, 2: bh + 3, :bw] + 16) >> 5    # rows dy = 0 .. bh: b, and s one row below
    hraw = (h1[:, :bh, 2: bw + 3] + 16) >> 5    # cols dx = 0 .. bw: h, and m one column right
    jraw = (j1 + 512) >> 10
    B, Hh, J = _clip1(braw), _clip1(hraw), _clip1(jraw)
    inter = {"b": (B[:, :bh], braw[:, :bh]), "s": (B[:, 1:], braw[:, 1:]), "h": (Hh[:, :, :bw], hraw[:, :, :bw]),
             "m": (Hh[:, :, 1:], hraw[:, :, 1:]), "j": (J, jraw)}
    G = win[:, 2: bh + 2, 2: bw + 2]
    Hs = win[:, 2: bh + 2, 3: bw + 3]       # H: the sample right of G
    Ms = win[:, 3: bh + 3, 2: bw + 2]       # M: the sample below G
    b, s, h, m, j = (inter[k][0] for k in "bshmj")
    # Table 8-12: (xFrac, yFrac) -> sample, with the intermediates it is built from
    table = {(0, 0): (G, ""), (1, 0): ((G + b + 1) >> 1, "b"), (2, 0): (b, "b"), (3, 0): ((Hs + b + 1) >> 1, "b"),
             (0, 1): ((G + h + 1) >> 1, "h"), (0, 2): (h, "h"), (0, 3): ((Ms + h + 1) >> 1, "h"),
             (1, 1): ((b + h + 1) >> 1, "bh"), (3, 1): ((b + m + 1) >> 1, "bm"), (1, 3): ((h + s + 1) >> 1, "hs"),
             (3, 3): ((m + s + 1) >> 1, "ms"), (2, 1): ((b + j + 1) >> 1, "bj"), (2, 2): (j, "j"),
             (2, 3): ((j + s + 1) >> 1, "js"), (1, 2): ((h + j + 1) >> 1, "hj"), (3, 2): ((j + m + 1) >> 1, "jm")}
    n = len(x0)
    pred = np.zeros((n, bh, bw), np.int64)
    oor = np.zeros(n, bool)
    for (fx, fy), (val, used) in table.items():
        sel = (xf == fx) & (yf == fy)
        if not sel.any():
            continue
        pred[sel] = val[sel]
        for k in used:
            raw = inter[k][1][sel]
            oor[sel] |= ((raw < 0) | (raw > 255)).reshape(raw.shape[0], -1).any(axis=1)
    outside = (xi < 0) | (yi < 0) | (xi + bw - 1 >= W) | (yi + bh - 1 >= H)
    return pred, oor, outside


def chroma_mc(ref, x0, y0, mvx, mvy, bw=4, bh=4):
    """8.4.2.2.2 (4:2:0 frame: the chroma vector is the luma vector in eighth chroma samples) for N blocks; x0, y0 in chroma
    samples.  Returns (N, bh, bw) int64."""
    H, W = ref.shape
    x0, y0, mvx, mvy = (np.asarray(a, dtype=np.int64) for a in (x0, y0, mvx, mvy))
    xi, yi, xf, yf = x0 + (mvx >> 3), y0 + (mvy >> 3), (mvx & 7)[:, None, None], (mvy & 7)[:, None, None]
    cols = np.clip(xi[:, None] + np.arange(bw + 1)[None, :], 0, W - 1)
    rows = np.clip(yi[:, None] + np.arange(bh + 1)[None, :], 0, H - 1)
    win = ref.astype(np.int64)[rows[:, :, None], cols[:, None, :]]
    A, Bs, C, D = win[:, :bh, :bw], win[:, :bh, 1:], win[:, 1:, :bw], win[:, 1:, 1:]
    return ((8 - xf) * (8 - yf) * A + xf * (8 - yf) * Bs + (8 - xf) * yf * C + xf * yf * D + 32) >> 6


# ---------------------------------------------------------------- intra

def pred16x16(top, left, topleft, mode):
    """8.3.3: top = p[0..15, -1] or None, left = p[-1, 0..15] or None, topleft = p[-1, -1] or None.
    Returns (pred (16, 16) int64 or None when the mode needs unavailable samples, clamped: the plane mode left 0..255)"""
    if mode == 0:
        return (None, False) if top is None else (np.tile(top, (16, 1)), False)
    if mode == 1:
        return (None, False) if left is None else (np.tile(left[:, None], (1, 16)), False)
    if mode == 2:
        if top is not None and left is not None:
            dc = (top.sum() + left.sum() + 16) >> 5
        elif left is not None:
            dc = (left.sum() + 8) >> 4
        elif top is not None:
            dc = (top.sum() + 8) >> 4
        else:
            dc = 128
        return np.full((16, 16), dc, np.int64), False
    if top is None or left is None or topleft is None:
        return None, False
    pt = np.concatenate([[topleft], top])     # pt[1 + x] = p[x, -1], pt[0] = p[-1, -1]
    pl = np.concatenate([[topleft], left])
    xp = np.arange(8)
    Hs = int(((xp + 1) * (pt[1 + 8 + xp] - pt[1 + 6 - xp])).sum())
    Vs = int(((xp + 1) * (pl[1 + 8 + xp] - pl[1 + 6 - xp])).sum())
    a = 16 * (int(left[15]) + int(top[15]))
    b = (5 * Hs + 32) >> 6
    c = (5 * Vs + 32) >> 6
    x = np.arange(16)[None, :]
    y = np.arange(16)[:, None]
    raw = (a + b * (x - 7) + c * (y - 7) + 16) >> 5
    return _clip1(raw), bool(((raw < 0) | (raw > 255)).any())


def pred_chroma8x8(top, left, topleft, mode):
    """8.3.4 for one 8x8 chroma block (4:2:0); mode 0 DC, 1 horizontal, 2 vertical, 3 plane.  Same return as pred16x16."""
    if mode == 0:
        out = np.zeros((8, 8), np.int64)
        for yo in (0, 4):
            for xo in (0, 4):
                t = None if top is None else top[xo: xo + 4]
                l = None if left is None else left[yo: yo + 4]
                if (xo, yo) in ((0, 0), (4, 4)):               # 8.3.4.1 / 8.3.4.3
                    if t is not None and l is not None:
                        dc = (t.sum() + l.sum() + 4) >> 3
                    elif l is not None:
                        dc = (l.sum() + 2) >> 2
                    elif t is not None:
                        dc = (t.sum() + 2) >> 2
                    else:
                        dc = 128
                elif xo == 4:                                   # 8.3.4.2 first branch (xO > 0, yO == 0): top first
                    dc = (t.sum() + 2) >> 2 if t is not None else (l.sum() + 2) >> 2 if l is not None else 128
                else:                                           # xO == 0, yO > 0: left first
                    dc = (l.sum() + 2) >> 2 if l is not None else (t.sum() + 2) >> 2 if t is not None else 128
                out[yo: yo + 4, xo: xo + 4] = dc
        return out, False
    if mode == 1:
        return (None, False) if left is None else (np.tile(left[:, None], (1, 8)), False)
    if mode == 2:
        return (None, False) if top is None else (np.tile(top, (8, 1)), False)
    if top is None or left is None or topleft is None:
        return None, False
    pt = np.concatenate([[topleft], top])
    pl = np.concatenate([[topleft], left])
    xp = np.arange(4)
    Hs = int(((xp + 1) * (pt[1 + 4 + xp] - pt[1 + 2 - xp])).sum())
    Vs = int(((xp + 1) * (pl[1 + 4 + xp] - pl[1 + 2 - xp])).sum())
    a = 16 * (int(left[7]) + int(top[7]))
    b = (34 * Hs + 32) >> 6
    c = (34 * Vs + 32) >> 6
    x = np.arange(8)[None, :]
    y = np.arange(8)[:, None]
    raw = (a + b * (x - 3) + c * (y - 3) + 16) >> 5
    return _clip1(raw), bool(((raw < 0) | (raw > 255)).any())


def pred4x4(top8, left, topleft, mode):
    """8.3.1.2: top8 = p[0..7, -1] (p[4..7, -1] already substituted when not available) or None, left = p[-1, 0..3] or None,
    topleft = p[-1, -1] or None.  Returns (4, 4) int64, or None when the mode needs unavailable samples."""
    if mode == 0:
        return None if top8 is None else np.tile(top8[:4], (4, 1))
    if mode == 1:
        return None if left is None else np.tile(left[:, None], (1, 4))
    if mode == 2:
        if top8 is not None and left is not None:
            dc = (top8[:4].sum() + left.sum() + 4) >> 3
        elif left is not None:
            dc = (left.sum() + 2) >> 2
        elif top8 is not None:
            dc = (top8[:4].sum() + 2) >> 2
        else:
            dc = 128
        return np.full((4, 4), dc, np.int64)
    out = np.zeros((4, 4), np.int64)
    if mode in (3, 7):
        if top8 is None:
            return None
        T = [int(v) for v in top8]
        for y in range(4):
            for x in range(4):
                if mode == 3:                                    # 8.3.1.2.4 Diagonal_Down_Left
                    out[y, x] = (T[6] + 3 * T[7] + 2) >> 2 if (x == 3 and y == 3) else (T[x + y] + 2 * T[x + y + 1] + T[x + y + 2] + 2) >> 2
                elif y % 2 == 0:                                 # 8.3.1.2.8 Vertical_Left
                    out[y, x] = (T[x + (y >> 1)] + T[x + (y >> 1) + 1] + 1) >> 1
                else:
                    out[y, x] = (T[x + (y >> 1)] + 2 * T[x + (y >> 1) + 1] + T[x + (y >> 1) + 2] + 2) >> 2
        return out
    if mode == 8:                                                # 8.3.1.2.9 Horizontal_Up
        if left is None:
            return None
        L = [int(v) for v in left]
        for y in range(4):
            for x in range(4):
                z = x + 2 * y
                if z > 5:
                    out[y, x] = L[3]
                elif z == 5:
                    out[y, x] = (L[2] + 3 * L[3] + 2) >> 2
                elif z % 2 == 0:
                    out[y, x] = (L[y + (x >> 1)] + L[y + (x >> 1) + 1] + 1) >> 1
                else:
                    out[y, x] = (L[y + (x >> 1)] + 2 * L[y + (x >> 1) + 1] + L[y + (x >> 1) + 2] + 2) >> 2
        return out
    # modes 4, 5, 6 need top, left and top-left
    if top8 is None or left is None or topleft is None:
        return None

    def p(x, y):   # p[x, y] with x == -1 or y == -1
        if y == -1:
            return int(topleft) if x == -1 else int(top8[x])
        return int(left[y])
    for y in range(4):
        for x in range(4):
            if mode == 4:                                        # 8.3.1.2.5 Diagonal_Down_Right
                if x > y:
                    v = (p(x - y - 2, -1) + 2 * p(x - y - 1, -1) + p(x - y, -1) + 2) >> 2
                elif x < y:
                    v = (p(-1, y - x - 2) + 2 * p(-1, y - x - 1) + p(-1, y - x) + 2) >> 2
                else:
                    v = (p(0, -1) + 2 * p(-1, -1) + p(-1, 0) + 2) >> 2
            elif mode == 5:                                      # 8.3.1.2.6 Vertical_Right
                z = 2 * x - y
                if z >= 0 and z % 2 == 0:
                    v = (p(x - (y >> 1) - 1, -1) + p(x - (y >> 1), -1) + 1) >> 1
                elif z > 0:
                    v = (p(x - (y >> 1) - 2, -1) + 2 * p(x - (y >> 1) - 1, -1) + p(x - (y >> 1), -1) + 2) >> 2
                elif z == -1:
                    v = (p(-1, 0) + 2 * p(-1, -1) + p(0, -1) + 2) >> 2
                else:
                    v = (p(-1, y - 1) + 2 * p(-1, y - 2) + p(-1, y - 3) + 2) >> 2
            else:                                                # 8.3.1.2.7 Horizontal_Down
                z = 2 * y - x
                if z >= 0 and z % 2 == 0:
                    v = (p(-1, y - (x >> 1) - 1) + p(-1, y - (x >> 1)) + 1) >> 1
                elif z > 0:
                    v = (p(-1, y - (x >> 1) - 2) + 2 * p(-1, y - (x >> 1) - 1) + p(-1, y - (x >> 1)) + 2) >> 2
                elif z == -1:
                    v = (p(-1, 0) + 2 * p(-1, -1) + p(0, -1) + 2) >> 2
                else:
                    v = (p(x - 1, -1) + 2 * p(x - 2, -1) + p(x - 3, -1) + 2) >> 2
            out[y, x] = v
    return out


def blk_xy(blk):
    """6.4.3: luma4x4BlkIdx -> (x, y) of the block in 4x4 units inside the macroblock"""
    return 2 * ((blk >> 2) & 1) + (blk & 1), 2 * (blk >> 3) + ((blk >> 1) & 1)


def blk_idx(bx, by):
    return 8 * (by >> 1) + 4 * (bx >> 1) + 2 * (by & 1) + (bx & 1)


class Availability:
    """6.4.x neighbour availability for macroblocks coded in raster order in slices of `slice_rows` whole macroblock rows"""

    def __init__(self, mbw, mbh, slice_rows):
        self.mbw, self.mbh, self.slice_rows = mbw, mbh, max(1, slice_rows)

    def mb(self, mx, my, nx, ny):
        """macroblock (nx, ny) is available to (mx, my): inside the picture, in the same slice, earlier in decoding order"""
        if not (0 <= nx < self.mbw and 0 <= ny < self.mbh):
            return False
        if ny // self.slice_rows != my // self.slice_rows:
            return False
        return ny * self.mbw + nx < my * self.mbw + mx


# ---------------------------------------------------------------- the check

def coded_planes(i420, width, height, cw, ch):
    """source I420 (display size) -> three planes of the coded size, the last column / row repeated (what I_PCM carries)"""
    f = np.asarray(i420, dtype=np.uint8).ravel()
    n = width * height
    planes = (f[:n].reshape(height, width), f[n: n * 5 // 4].reshape(height // 2, width // 2),
              f[n * 5 // 4: n * 3 // 2].reshape(height // 2, width // 2))
    out = []
    for p, (tw, th) in zip(planes, ((cw, ch), (cw // 2, ch // 2), (cw // 2, ch // 2))):
        out.append(np.pad(p, ((0, th - p.shape[0]), (0, tw - p.shape[1])), mode="edge"))
    return out


class PredictionMismatch(AssertionError):
    pass


def _first_diff(got, want):
    d = np.argwhere(np.asarray(got, np.int64) != np.asarray(want, np.int64))
    y, x = d[0]
    return "first at (%d, %d): %d != %d, %d samples differ" % (x, y, got[y, x], want[y, x], len(d))


def check_picture(pre, refs, src, mbinfo, mvq, mbaux, levels, slice_rows, tag="", counters=None, max_report=6):
    """pre: pre-filter (Y, U, V) of the coded picture; refs: post-filter (Y, U, V) of the previous pictures, refs[0] the
    newest (ref_idx_l0 0); src: the source as coded planes (coded_planes()); mbinfo / mvq / mbaux / levels: side
    information of the picture; slice_rows: macroblock rows per slice.  Adds to `counters` (a dict, created when None) and
    returns it; raises PredictionMismatch naming the picture (tag), macroblock, quadrant / block, mode, vector and ref_idx."""
    if counters is None:
        counters = {}
    for k in COUNTERS:
        counters.setdefault(k, 0)
    Y, U, V = (np.asarray(p) for p in pre)
    ch_, cw_ = Y.shape
    mbw, mbh = cw_ // 16, ch_ // 16
    av = Availability(mbw, mbh, slice_rows)
    types = mbinfo["type"].astype(np.int64)
    cbp = mbinfo["cbp"].astype(np.int64)
    errs = []

    def fail(msg):
        errs.append("%s: %s" % (tag, msg))

    # ---- inter: every quadrant of every inter macroblock, batched ----
    inter_mbs = np.nonzero(np.isin(types, INTER_TYPES))[0]
    if len(inter_mbs):
        mb_of = np.repeat(inter_mbs, 4)
        q = np.tile(np.arange(4), len(inter_mbs))
        skip = types[mb_of] == MB_PSKIP
        vx = np.where(skip, mbinfo["mvx"][mb_of], mvq[mb_of, 2 * q]).astype(np.int64)
        vy = np.where(skip, mbinfo["mvy"][mb_of], mvq[mb_of, 2 * q + 1]).astype(np.int64)
        ridx = np.where(skip, 0, mbinfo["chroma_mode"][mb_of]).astype(np.int64)
        mx, my = mb_of % mbw, mb_of // mbw
        lx, ly = 16 * mx + 8 * (q & 1), 16 * my + 8 * (q >> 1)
        cx, cy = 8 * mx + 4 * (q & 1), 8 * my + 4 * (q >> 1)
        luma_only = skip | ((cbp[mb_of] >> q) & 1 == 0)
        chroma_only = skip | (cbp[mb_of] >> 4 == 0)
        for r in np.unique(ridx):
            sel = ridx == r
            if r >= len(refs):
                for i in np.nonzero(sel)[0]:
                    fail("mb %d (%d, %d) quadrant %d: ref_idx %d but only %d reference pictures" % (mb_of[i], mx[i], my[i], q[i], r, len(refs)))
                continue
            ry, ru, rv = (np.asarray(p) for p in refs[r])
            ls = sel & luma_only
            if ls.any():
                pred, oor, outside = luma_mc(ry, lx[ls], ly[ls], vx[ls], vy[ls])
                idx = np.nonzero(ls)[0]
                got = Y[ly[ls][:, None, None] + np.arange(8)[None, :, None], lx[ls][:, None, None] + np.arange(8)[None, None, :]]
                bad = (got != pred).reshape(len(idx), -1).any(axis=1)
                for k in np.nonzero(bad)[0]:
                    i = idx[k]
                    fail("mb %d (%d, %d) type %d quadrant %d luma: vector (%d, %d) ref_idx %d: %s"
                         % (mb_of[i], mx[i], my[i], types[mb_of[i]], q[i], vx[i], vy[i], r, _first_diff(got[k], pred[k])))
                fx, fy = vx[ls] & 3, vy[ls] & 3
                counters["inter_quadrants"] += int(ls.sum())
                counters["frac_x"] += int(((fx != 0) & (fy == 0)).sum())
                counters["frac_y"] += int(((fx == 0) & (fy != 0)).sum())
                counters["frac_xy"] += int(((fx != 0) & (fy != 0)).sum())
                counters["j_pos"] += int(((fx == 2) & (fy == 2)).sum())
                counters["mc_clipped"] += int(oor.sum())
                counters["mv_outside"] += int(outside.sum())
            cs = sel & chroma_only
            if cs.any():
                idx = np.nonzero(cs)[0]
                for pl, (rp, cur) in enumerate(((ru, U), (rv, V))):
                    pred = chroma_mc(rp, cx[cs], cy[cs], vx[cs], vy[cs])
                    got = cur[cy[cs][:, None, None] + np.arange(4)[None, :, None], cx[cs][:, None, None] + np.arange(4)[None, None, :]]
                    bad = (got != pred).reshape(len(idx), -1).any(axis=1)
                    for k in np.nonzero(bad)[0]:
                        i = idx[k]
                        fail("mb %d (%d, %d) type %d quadrant %d chroma %s: vector (%d, %d) ref_idx %d: %s"
                             % (mb_of[i], mx[i], my[i], types[mb_of[i]], q[i], "UV"[pl], vx[i], vy[i], r, _first_diff(got[k], pred[k])))
                counters["chroma_mc_blocks"] += int(cs.sum())

    # ---- intra and I_PCM, macroblock by macroblock ----
    Yi, Ui, Vi = (p.astype(np.int64) for p in (Y, U, V))
    for a in np.nonzero(np.isin(types, (MB_I16, MB_I4, MB_IPCM)))[0]:
        t = types[a]
        mx, my = a % mbw, a // mbw
        x0, y0 = 16 * mx, 16 * my
        if t == MB_IPCM:
            counters["pcm"] += 1
            for pl, (cur, s, n) in enumerate(((Y, src[0], 16), (U, src[1], 8), (V, src[2], 8))):
                g, w = cur[n * my: n * my + n, n * mx: n * mx + n], s[n * my: n * my + n, n * mx: n * mx + n]
                if not np.array_equal(g, w):
                    fail("mb %d (%d, %d) I_PCM plane %d is not the source: %s" % (a, mx, my, pl, _first_diff(g, w)))
            continue
        A = av.mb(mx, my, mx - 1, my)
        B = av.mb(mx, my, mx, my - 1)
        D = av.mb(mx, my, mx - 1, my - 1)
        C = av.mb(mx, my, mx + 1, my - 1)
        if t == MB_I16 and cbp[a] & 15 == 0 and not np.any(levels[a, 0:16]):
            mode = int(mbinfo["i16_mode"][a])
            pred, clamped = pred16x16(Yi[y0 - 1, x0: x0 + 16] if B else None, Yi[y0: y0 + 16, x0 - 1] if A else None,
                                      Yi[y0 - 1, x0 - 1] if D else None, mode)
            if pred is None:
                fail("mb %d (%d, %d) Intra16x16 mode %d needs neighbours that are not available (left %d top %d)" % (a, mx, my, mode, A, B))
            else:
                got = Y[y0: y0 + 16, x0: x0 + 16]
                if not np.array_equal(got, pred):
                    fail("mb %d (%d, %d) Intra16x16 mode %d: %s" % (a, mx, my, mode, _first_diff(got, pred)))
                counters["i16_checked"] += 1
                counters["i16_plane"] += int(mode == 3)
                counters["i16_plane_clamped"] += int(clamped)
        if t == MB_I4:
            for blk in range(16):
                if (cbp[a] >> (blk >> 2)) & 1:
                    continue
                bx, by = blk_xy(blk)
                px, py = x0 + 4 * bx, y0 + 4 * by
                left_ok = bx > 0 or A
                top_ok = by > 0 or B
                tl_ok = (bx > 0 and by > 0) or (bx == 0 and by > 0 and A) or (bx > 0 and by == 0 and B) or (bx == 0 and by == 0 and D)
                if by == 0:
                    tr_ok = B if bx < 3 else C
                else:
                    tr_ok = bx < 3 and blk_idx(bx + 1, by - 1) < blk
                top8 = None
                if top_ok:
                    top8 = Yi[py - 1, px: px + 8].copy() if tr_ok else np.concatenate([Yi[py - 1, px: px + 4], np.repeat(Yi[py - 1, px + 3], 4)])
                mode = int(mbaux[a, blk])
                pred = pred4x4(top8, Yi[py: py + 4, px - 1] if left_ok else None, Yi[py - 1, px - 1] if tl_ok else None, mode)
                if pred is None:
                    fail("mb %d (%d, %d) Intra4x4 block %d mode %d needs neighbours that are not available" % (a, mx, my, blk, mode))
                    continue
                got = Y[py: py + 4, px: px + 4]
                if not np.array_equal(got, pred):
                    fail("mb %d (%d, %d) Intra4x4 block %d (%d, %d) mode %d: %s" % (a, mx, my, blk, bx, by, mode, _first_diff(got, pred)))
                counters["i4_blocks"] += 1
        if cbp[a] >> 4 == 0:
            mode = int(mbinfo["chroma_mode"][a])
            c0x, c0y = 8 * mx, 8 * my
            for pl, cur in ((0, Ui), (1, Vi)):
                pred, clamped = pred_chroma8x8(cur[c0y - 1, c0x: c0x + 8] if B else None, cur[c0y: c0y + 8, c0x - 1] if A else None,
                                               cur[c0y - 1, c0x - 1] if D else None, mode)
                if pred is None:
                    fail("mb %d (%d, %d) chroma mode %d needs neighbours that are not available (left %d top %d)" % (a, mx, my, mode, A, B))
                    break
                got = cur[c0y: c0y + 8, c0x: c0x + 8]
                if not np.array_equal(got, pred):
                    fail("mb %d (%d, %d) type %d chroma %s intra mode %d: %s" % (a, mx, my, t, "UV"[pl], mode, _first_diff(got, pred)))
                counters["chroma_plane_clamped"] += int(clamped)
            counters["chroma_intra_checked"] += 1
    if errs:
        more = "" if len(errs) <= max_report else "\n  ... %d more" % (len(errs) - max_report)
        raise PredictionMismatch("prediction-only regions differ from the prediction of the standard:\n  " + "\n  ".join(errs[:max_report]) + more)
    return counters
