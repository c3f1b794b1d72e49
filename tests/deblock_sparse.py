"""Inputs and conditions of tests/test_gpu_deblock_sparse.py: short sequences whose P pictures differ from the previous source in
chosen macroblocks only, so that the loop filter (media_amd/csrc/k_deblock.h) meets filtered and unfiltered top edges, dirty and
clean macroblocks in known places; the boundary strengths restated from the oracle's macroblock records (8.7.2.1, as k_bs computes
them); and what each case must contain, stated of the oracle alone."""
import functools
import numpy as np
from media_amd import synth
from oracle_lib import OracleEncoder

QP = 30
INTRA_TYPES = (0, 3, 4)   # MbInfo type: Intra16x16, I_PCM, Intra4x4
MB_P16, MB_P16X8 = 1, 5
AMP_Y, AMP_C = 14, 6   # what a changed macroblock's samples move by


def xy2blk(x, y):
    return (x & 1) | ((y & 1) << 1) | ((x & 2) << 1) | ((y & 2) << 2)


def slice_rows(mbh, slices):
    return mbh if slices <= 1 else -(-mbh // slices)


def strengths(mb, mvq, mbw, mbh, slices=0):
    """bS[my, mx, dir, edge, segment] of one picture from the oracle's mbinfo() / mvq(): dir 0 vertical edges, 1 horizontal"""
    rows = slice_rows(mbh, slices)
    bs = np.zeros((mbh, mbw, 2, 4, 4), np.uint8)
    typ, tc, i16, ref = mb["type"], mb["tc"], mb["i16_mode"], mb["chroma_mode"]
    intra = np.isin(typ, INTRA_TYPES)
    t8 = ((typ == MB_P16) | (typ >= MB_P16X8)) & (i16 == 1)
    for my in range(mbh):
        for mx in range(mbw):
            q = my * mbw + mx
            for d in range(2):
                for e in range(4):
                    if e == 0 and (mx == 0 if d == 0 else my % rows == 0):
                        continue
                    p = q if e else (q - 1 if d == 0 else q - mbw)
                    for k in range(4):
                        bq = xy2blk(e, k) if d == 0 else xy2blk(k, e)
                        bp = (xy2blk(3 if e == 0 else e - 1, k)) if d == 0 else xy2blk(k, 3 if e == 0 else e - 1)
                        if intra[p] or intra[q]:
                            s = 4 if e == 0 else 3
                        elif t8[q] and (e & 1):
                            s = 0
                        else:
                            nzq = tc[q][bq & ~3: (bq & ~3) + 4].any() if t8[q] else tc[q][bq] != 0
                            nzp = tc[p][bp & ~3: (bp & ~3) + 4].any() if t8[p] else tc[p][bp] != 0
                            vp, vq = mvq[p][2 * (bp >> 2): 2 * (bp >> 2) + 2].astype(int), mvq[q][2 * (bq >> 2): 2 * (bq >> 2) + 2].astype(int)
                            s = 2 if (nzp or nzq) else 1 if (ref[p] != ref[q] or abs(vp - vq).max() >= 4) else 0
                        bs[my, mx, d, e, k] = s
    return bs


def edge_maps(bs, slices=0):
    """per macroblock: top (its top edge is filtered), own (one of its eight edge groups is), dirty (own, or the left edge of the
    right neighbour), down (the row below takes its bottom rows: top of the macroblock below, inside the slice), last (no row below
    in its slice)"""
    mbh, mbw = bs.shape[:2]
    rows = slice_rows(mbh, slices)
    top = bs[:, :, 1, 0].any(axis=-1)
    own = bs.reshape(mbh, mbw, -1).any(axis=-1)
    left = bs[:, :, 0, 0].any(axis=-1)
    dirty = own.copy()
    dirty[:, :-1] |= left[:, 1:]
    down, last = np.zeros_like(top), np.zeros_like(top)
    down[:-1] = top[1:]
    for my in range(mbh):
        if my == mbh - 1 or (my + 1) % rows == 0:   # the last row of the picture or of a slice stores all sixteen sample rows
            down[my], last[my] = False, True
    return {"top": top, "own": own, "dirty": dirty, "clean": ~dirty, "down": down, "left": left, "last": last}


def mask(name, mbw, mbh):
    """macroblocks of a P picture that differ from the previous source.  A macroblock is clean when it, its left, right and upper
    neighbours are unchanged - so the checkerboard is a sparse, staggered one (every other row, every third column) and the column
    stripes are the two outer columns: a third of 6 x 5 macroblocks and more stay clean"""
    y, x = np.mgrid[0:mbh, 0:mbw]
    if name == "checker":
        return (y % 2 == 1) & (x % 3 == (1 + y // 2) % 3) if mbw > 1 else y % 2 == 1
    if name == "rows":     # rows 1, 2 of every four: changed and unchanged rows both even and odd
        return (y % 4 == 1) | (y % 4 == 2)
    if name == "columns":
        return (x == 0) | (x == mbw - 1)
    if name == "one_bottom":
        return (y == mbh - 1) & (x == mbw // 2)
    if name == "one_right":
        return (x == mbw - 1) & (y == mbh // 2)
    if name == "all":
        return y >= 0
    if name == "none":
        return y < 0
    raise KeyError(name)


MASKS = ("checker", "rows", "columns", "one_bottom", "one_right", "all", "none")


def frames_for(name, w, h, npic, cut=False):
    """IDR source, then P sources: the previous one with a pattern of 2x2 squares added to (odd pictures) or taken from (even ones)
    the masked macroblocks - found at vector 0 and coded with coefficients, bS 2 on their edges; every other macroblock is the
    previous source again and settles as P_Skip, bS 0.  cut: the last picture is other content everywhere (synth.frame_cut behind its cut), the search
    finds nothing and macroblocks go intra"""
    mbw, mbh = w // 16, h // 16
    out = [synth.frame_s1(w, h, 0).copy()]
    m = np.kron(mask(name, mbw, mbh).astype(np.int16), np.ones((16, 16), np.int16))
    yy, xx = np.mgrid[0:h, 0:w]
    pat = (((xx // 2 + yy // 2) % 2) * 2 - 1).astype(np.int16) * m
    for i in range(1, npic):
        if cut and i == npic - 1:
            out.append(synth.frame_cut(w, h, 5))
            continue
        nxt = out[-1].astype(np.int16)
        sgn = 1 if i % 2 else -1
        nxt[: w * h] += (sgn * AMP_Y * pat).ravel()
        for p in range(2):
            o = w * h + p * (w * h // 4)
            nxt[o: o + w * h // 4] += (sgn * AMP_C * pat[::2, ::2][: h // 2, : w // 2]).ravel()
        out.append(np.clip(nxt, 0, 255).astype(np.uint8))
    return out


@functools.lru_cache(maxsize=None)
def oracle(names, w, h, npic=4, slices=0, cut=False, disable_deblock=0):
    """names: one mask per GOP of npic pictures, coded one after the other by ONE encoder.  (frames, per picture dict(au, pre, post,
    maps, intra, changed ...)); computed once per configuration and shared, never modified.
    changed[my, mx]: the filter changed a sample of the macroblock; changed_bottom: one of its luma rows 12..15; changed_right: one
    of its luma columns 13..15"""
    frames = [f for n in names for f in frames_for(n, w, h, npic, cut)]
    orc = OracleEncoder(w, h, qp=QP, gop=npic, slices=slices, disable_deblock=disable_deblock)
    mbw, mbh = orc.cw // 16, orc.ch // 16
    out = []
    for f in frames:
        au = orc.encode(f)[0]
        post = tuple(orc.recon(p) for p in range(3))
        pre = tuple(orc.recon_pre(p) for p in range(3))
        for a in post + pre:
            a.setflags(write=False)
        mb = orc.mbinfo()
        diff = (post[0] != pre[0]).reshape(mbh, 16, mbw, 16)
        cdiff = sum((post[p] != pre[p]).reshape(mbh, 8, mbw, 8).any(axis=(1, 3)) for p in (1, 2)) > 0
        out.append({"au": au, "pre": pre, "post": post, "maps": edge_maps(strengths(mb, orc.mvq(), mbw, mbh, slices), slices),
                    "intra": int(np.isin(mb["type"], INTRA_TYPES).sum()), "changed": diff.any(axis=(1, 3)) | cdiff,
                    "changed_bottom": diff[:, 12:].any(axis=(1, 3)), "changed_right": diff[:, :, :, 13:].any(axis=(1, 3))})
    orc.close()
    return frames, out


def conditions(pic):
    """what a P picture contains of the situations the sparse hand-off distinguishes (names -> bool; clean_fraction a number)"""
    m = pic["maps"]
    top, dirty, clean, down, own, left, inner = m["top"], m["dirty"], m["clean"], m["down"], m["own"], m["left"], ~m["last"]
    mbh = top.shape[0]
    quiet_left = ~own
    quiet_left[:, :-1] &= left[:, 1:]
    quiet_left[:, -1] = False
    return {
        # the upper row stores its own bottom rows - and the filter changed them, so leaving them out shows
        "dirty_above_unfiltered_top": bool((dirty & inner & ~down & pic["changed_bottom"]).any()),
        # a publish of unchanged samples
        "clean_above_filtered_top": bool((clean & down).any()),
        # both halves of a pair (its upper row is even, its lower row odd) and the edge between pairs
        "mixed_tops_even_row": any(top[r].any() and not top[r].all() for r in range(2, mbh, 2)),
        "mixed_tops_odd_row": any(top[r].any() and not top[r].all() for r in range(1, mbh, 2)),
        "dirty_last_column": bool(dirty[:, -1].any()),
        "dirty_last_row": bool(dirty[-1].any()),
        # no own edge, but the right neighbour's left edge is filtered - and changes this macroblock's columns 13..15
        "quiet_left_of_filtered_edge": bool((quiet_left & pic["changed_right"]).any()),
        "filter_changes_a_sample": bool(pic["changed"].any()),
        "clean_fraction": float(clean.mean()),
    }
