"""SSIM in the quality report (include/mi355x_h264.h, "quality report: SSIM"): the definition restated in numpy from the header's
text, the case list, and the oracle's expected records - what tests/test_ssim_oracle.py (CPU: what the list holds) and
tests/test_gpu_ssim.py (GPU) share.

The definition.  src, rec, display samples and the plane order Y, U, V are those of the SSE (tests/quality.py).  A plane is W x H
display samples (chroma: width / 2 x height / 2).  A window is 8x8 samples at (4i, 4j) and counts when 4i + 8 <= W and
4j + 8 <= H: (W / 4 - 1) * (H / 4 - 1) windows.  A band instance counts the windows whose origin row lies in its own macroblock
rows and whose last row lies below its limit, min(H, 16 * (row0 + rows)) for luma, min(H / 2, 8 * (row0 + rows)) for chroma.
Per window, integers over its 64 samples: s1 = sum src, s2 = sum rec, ss = sum (src^2 + rec^2), s12 = sum src * rec,
vars = 64 ss - s1^2 - s2^2, covar = 64 s12 - s1 s2, C1 = 416, C2 = 235963,
l = floor(((2 s1 s2 + C1) << 16) / (s1^2 + s2^2 + C1)), c = floor(((2 covar + C2) << 16) / (vars + C2)), q = (l * c) >> 16.
Per picture: sum[3] of q, windows[3], and a luma map [rows][columns of macroblocks] of the q of the windows whose origin lies in
the macroblock, 0 outside the band.  The GPU's reconstruction equals the oracle's bit for bit and everything is an integer:
nothing here has a tolerance.

Everything is deterministic; what is computed is computed once per process, shared and never changed."""
import functools
from collections import namedtuple
import numpy as np
import quality as q

C1, C2 = 416, 235963

Record = namedtuple("Record", "sum windows map q sums")   # q, sums: per plane, int64 [window rows][window columns] of the windows that count
Sums = namedtuple("Sums", "s1 s2 ss s12")


def window_sums(src, rec):
    """Sums of every window at (4i, 4j) that lies wholly inside the two equally sized planes: int64 arrays [H / 4 - 1][W / 4 - 1]"""
    a, b = np.asarray(src, np.int64), np.asarray(rec, np.int64)
    assert a.shape == b.shape
    if a.shape[0] < 8 or a.shape[1] < 8:
        z = np.zeros((max(0, a.shape[0] // 4 - 1), max(0, a.shape[1] // 4 - 1)), np.int64)
        return Sums(z, z, z, z)

    def win(p):
        return np.lib.stride_tricks.sliding_window_view(p, (8, 8))[::4, ::4].sum(axis=(2, 3))
    return Sums(win(a), win(b), win(a * a + b * b), win(a * b))


def evaluate(s):
    """(l, c, q) of window sums, in int64 (numpy's // is floor division and >> is arithmetic on signed integers)"""
    s1, s2, ss, s12 = (np.asarray(v, np.int64) for v in s)
    vars_ = 64 * ss - s1 * s1 - s2 * s2
    covar = 64 * s12 - s1 * s2
    l = ((2 * s1 * s2 + C1) << 16) // (s1 * s1 + s2 * s2 + C1)
    c = ((2 * covar + C2) << 16) // (vars_ + C2)
    return l, c, (l * c) >> 16


def evaluate_py(s1, s2, ss, s12):
    """one window in Python integers (no width at all): (l, c, q) and the terms whose bounds the header states"""
    vars_ = 64 * ss - s1 * s1 - s2 * s2
    covar = 64 * s12 - s1 * s2
    ln, ld = (2 * s1 * s2 + C1) << 16, s1 * s1 + s2 * s2 + C1
    cn, cd = (2 * covar + C2) << 16, vars_ + C2
    l, c = ln // ld, cn // cd
    return l, c, (l * c) >> 16, {"vars": vars_, "covar": covar, "ln": ln, "ld": ld, "cn": cn, "cd": cd}


def float_ssim(s):
    """the same window in floating point (the usual formula on the window's sums, the constants as above)"""
    s1, s2, ss, s12 = (np.asarray(v, np.float64) for v in s)
    vars_ = 64.0 * ss - s1 * s1 - s2 * s2
    covar = 64.0 * s12 - s1 * s2
    return (2.0 * s1 * s2 + C1) * (2.0 * covar + C2) / ((s1 * s1 + s2 * s2 + C1) * (vars_ + C2))


def window_count(w, h):
    return max(0, w // 4 - 1) * max(0, h // 4 - 1)


def expected(src_planes, rec_planes, w, h, row0=0, rows=None):
    """Record of one picture.  src_planes: (Y, U, V) of the display size; rec_planes: (Y, U, V) of the coded size; row0, rows: the
    macroblock rows of a band instance (default: all)"""
    mbw, mbh = (w + 15) // 16, (h + 15) // 16
    rows = mbh - row0 if rows is None else rows
    sums, counts, qs, ws = [], [], [], []
    mp = np.zeros((mbh, mbw), np.int64)
    for p in range(3):
        pw, ph, b = (w, h, 16) if p == 0 else (w // 2, h // 2, 8)
        first, limit = b * row0, min(ph, b * (row0 + rows))
        # the band's display samples: its windows are those that lie wholly inside them (origin rows first, first + 4, ..)
        s, r = src_planes[p][first:limit, :pw], rec_planes[p][first:limit, :pw]
        ws.append(window_sums(s, r))
        qq = evaluate(ws[-1])[2]
        assert qq.shape == (max(0, (limit - first) // 4 - 1), max(0, pw // 4 - 1))
        qq.setflags(write=False)
        qs.append(qq)
        sums.append(int(qq.sum()))
        counts.append(int(qq.size))
        if p == 0:
            for j in range(qq.shape[0]):
                for i in range(qq.shape[1]):
                    mp[(first + 4 * j) // 16, (4 * i) // 16] += qq[j, i]
    assert int(mp.sum()) == sums[0] and (not mp.size or int(np.abs(mp).max()) <= 16 * 65536)
    m = mp.astype(np.int32)
    m.setflags(write=False)
    return Record(tuple(sums), tuple(counts), m, tuple(qs), tuple(ws))


def mean(rec):
    """mean SSIM per plane: sum / (65536 * windows)"""
    return [s / (65536.0 * n) if n else float("nan") for s, n in zip(rec.sum, rec.windows)]


# ---------------------------------------------------------------- the cases (tests/quality.py's, and three of this module's own)

TINY = q.case("tiny_16x16", "s1", 16, 16, 30, 4, 3)              # 9 luma windows, one per chroma plane
NOISE51 = q.case("noise51_64x48", "noise", 64, 48, 51, 4, 3)     # windows with q < 0
SINGLE = (TINY, q.CROP, NOISE51, q.PCM, q.NODEBLOCK, q.NV12, q.RGBA, q.REFS3, q.SLICES)
ALL = SINGLE + (q.BIG, q.BATCH4, q.PLUGIN) + q.HUB

Pic = namedtuple("Pic", "au idr rec sse")   # rec: the SSIM Record; sse: quality.Record of the same picture


def _pic(c, orc, src, au, idr, row0=0, rows=None):
    recon = tuple(orc.recon(p) for p in range(3))
    return Pic(au, idr, expected(src, recon, c.w, c.h, row0, rows), q.expected(src, recon, c.w, c.h, row0, rows))


@functools.lru_cache(maxsize=None)
def oracle_run(c):
    """the oracle's stream of the case: a tuple of Pic"""
    orc = q.oracle_for(c)
    out = []
    for f in q.frames(c):
        src, i420 = q.source_planes(c, f)
        au, idr = orc.encode(i420)
        out.append(_pic(c, orc, src, au, idr))
    orc.close()
    return tuple(out)


@functools.lru_cache(maxsize=None)
def oracle_bands(c, world=2):
    """`world` band instances of the oracle with halo swaps after every picture: per picture, (access unit put together, [Pic per band])"""
    parts = [q.oracle_for(c, band_index=r, band_count=world) for r in range(world)]
    buf = np.zeros(parts[0].halo_bytes(), np.uint8)
    out = []
    for f in q.frames(c):
        src, i420 = q.source_planes(c, f)
        coded = [p.encode(i420) for p in parts]
        pics = []
        for r, p in enumerate(parts):
            row0, rows = q.band_rows(c.h, c.slices, r, world)
            pics.append(_pic(c, p, src, coded[r][0], coded[r][1], row0, rows))
        for r in range(world):
            if r > 0:
                parts[r].halo_export(0, buf.ctypes.data)
                parts[r - 1].halo_import(1, buf.ctypes.data)
            if r < world - 1:
                parts[r].halo_export(1, buf.ctypes.data)
                parts[r + 1].halo_import(0, buf.ctypes.data)
        out.append((b"".join(a for a, _ in coded), tuple(pics)))
    for p in parts:
        p.close()
    return tuple(out)


@functools.lru_cache(maxsize=None)
def oracle_gops():
    """the lockstep batch of tests/quality.py (GOPS): one oracle codes the closed GOP of item 0, item 1, .."""
    orc = q.oracle_for(q.GOPS[0])
    out = []
    for c in q.GOPS:
        gop = []
        for i, f in enumerate(q.frames(c)):
            src, i420 = q.source_planes(c, f)
            au, idr = orc.encode(i420, force_idr=i == 0)
            gop.append(_pic(c, orc, src, au, idr))
        out.append(tuple(gop))
    orc.close()
    return tuple(out)


def plugin_replay(c, qps):
    """quality.plugin_replay with the SSIM record: picture i at QP qps[i], a scene cut coded again as an IDR picture"""
    orc = q.oracle_for(c)
    nmb = ((c.w + 15) // 16) * ((c.h + 15) // 16)
    out = []
    for i, f in enumerate(q.frames(c)):
        orc.set_qp(qps[i])
        src, i420 = q.source_planes(c, f)
        au, idr = orc.encode(i420)
        cut = not idr and orc.me_cost() > q.SCENE_CUT_COST_PER_MB * nmb
        if cut:
            au, idr = orc.encode(i420, force_idr=True)
        out.append((_pic(c, orc, src, au, idr), cut))
    orc.close()
    return tuple(out)
