#!/usr/bin/env python3
"""How much of a picture the loop filter has to touch (media_amd/csrc/k_deblock.h: db_hands_down, db_dirty), from the CPU oracle.
usage: db_sparsity.py [--content s1|s2|scroll] [--pictures 30] [--search seeded|exhaustive] [--width 1920 --height 1080 --qp 26]
       MI355X_H264_LIB=<a -DDB_AB_COUNT build> db_sparsity.py --gpu-counts ...      (needs the GPU)
Codes one closed GOP of the bench.py content with the oracle, restates the boundary strengths from its macroblock records
(8.7.2.1, as k_bs computes them) and prints per P picture the fractions of macroblocks
  top    whose top edge has a strength (the row below waits for the row above there, and nowhere else)
  quiet  none of whose own eight edge groups has one
  clean  quiet, and the right neighbour's left edge has none (nothing of it is stored, unless its bottom rows are handed down)
  idle   clean, and the top edge below has none (nothing to store, nothing to hand down)
the four counts of the -DDB_AB_COUNT build for the pair form (top_on, idle iterations, skipped, published), and the steps of the
path model of DESIGN.md section 11: pair p waits at mid-iteration, only where its upper row's top edge is filtered, for the publish
the pair above makes 0.3 into its iteration x + 2, hand-off latency 0.8 iterations (every macroblock coupled: 207.8 steps at
1080p); --quiet-cost is what an iteration with nothing to filter in either row costs (1 = as any other).
--gpu-counts encodes the same GOP on the GPU with the pair form forced, reads mi355x_h264_db_counts2() after every picture and
prints both; the last line says whether they are equal."""
import argparse
import ctypes
import json
import os
import sys
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
INTRA_TYPES, MB_P16, MB_P16X8 = (0, 3, 4), 1, 5


def edge_maps(mb, mvq, mbw, mbh):
    """per macroblock (one slice): top, left (that edge has a strength), own (any of its eight edge groups), dirty, down"""
    by, bx = np.mgrid[0:4, 0:4]
    blk = ((bx & 1) | ((by & 1) << 1) | ((bx & 2) << 1) | ((by & 2) << 2)).ravel()          # 4x4 block (by, bx) -> index into tc
    typ = mb["type"]
    t8 = ((typ == MB_P16) | (typ >= MB_P16X8)) & (mb["i16_mode"] == 1)
    tc = mb["tc"][:, :16] != 0
    q8 = np.repeat(tc.reshape(-1, 4, 4).any(axis=2), 4, axis=1)                              # transform 8x8: the quadrant's four lists
    nz = np.where(t8[:, None], q8, tc)[:, blk]                                              # [mb, by * 4 + bx]

    def grid(a):   # [mb, 16] -> [4 * mbh, 4 * mbw]
        return a.reshape(mbh, mbw, 4, 4).transpose(0, 2, 1, 3).reshape(4 * mbh, 4 * mbw)
    quad = (blk >> 2)
    NZ = grid(nz)
    MVX, MVY = grid(mvq[:, 2 * quad].astype(np.int32)), grid(mvq[:, 2 * quad + 1].astype(np.int32))
    per = lambda v: grid(np.repeat(v[:, None], 16, axis=1))
    INTRA, T8, REF = per(np.isin(typ, INTRA_TYPES)), per(t8), per(mb["chroma_mode"])

    def strengths(axis):   # edges between block line i - 1 and i along `axis`, i = 1 ..; returns [lines - 1, ...] moved to axis 0
        mv = lambda a: np.moveaxis(a, axis, 0)
        nzp, nzq = mv(NZ)[:-1], mv(NZ)[1:]
        s = np.where(nzp | nzq, 2, np.where((mv(REF)[:-1] != mv(REF)[1:]) | (abs(mv(MVX)[:-1] - mv(MVX)[1:]) >= 4) | (abs(mv(MVY)[:-1] - mv(MVY)[1:]) >= 4), 1, 0))
        i = np.arange(1, s.shape[0] + 1)[:, None]
        s = np.where(mv(T8)[1:] & (i % 2 == 1), 0, s)
        s = np.where(mv(INTRA)[:-1] | mv(INTRA)[1:], np.where(i % 4 == 0, 4, 3), s)
        return s
    v = strengths(1)   # [4 * mbw - 1, 4 * mbh]: vertical edge left of block column i
    h = strengths(0)   # [4 * mbh - 1, 4 * mbw]
    vfull = np.zeros((4 * mbw, 4 * mbh), np.uint8); vfull[1:] = v
    hfull = np.zeros((4 * mbh, 4 * mbw), np.uint8); hfull[1:] = h
    vany = vfull.reshape(mbw, 4, mbh, 4).any(axis=3).transpose(2, 0, 1)    # [my, mx, edge]
    hany = hfull.reshape(mbh, 4, mbw, 4).any(axis=3).transpose(0, 2, 1)
    top, left = hany[:, :, 0], vany[:, :, 0]
    own = vany.any(axis=2) | hany.any(axis=2)
    dirty = own.copy(); dirty[:, :-1] |= left[:, 1:]
    down = np.zeros_like(top); down[:-1] = top[1:]
    return {"top": top, "left": left, "own": own, "dirty": dirty, "down": down}


def pair_counts(m):
    """what a -DDB_AB_COUNT build counts on the picture in the pair form: top_on, idle iterations, skipped, published"""
    top, own, dirty, down = m["top"], m["own"], m["dirty"], m["down"]
    if not own.any():
        return [0, 0, 0, 0]   # (the picture-level early return: no wave counts)
    mbh, mbw = top.shape
    idle = 0
    for p in range((mbh + 1) // 2):
        busy = np.zeros(mbw + 2, bool)
        for half, r in enumerate((2 * p, 2 * p + 1)):
            if r >= mbh:
                continue
            cur = np.zeros(mbw + 2, bool); cur[half: half + mbw] = own[r]                      # iteration t holds macroblock t - half
            prev = np.zeros(mbw + 2, bool); prev[half + 1: half + 1 + mbw] = dirty[r] | down[r]    # and stores / hands down t - half - 1
            busy |= cur | prev
        idle += int((~busy).sum())
    return [int(top.sum()), idle, int((~dirty).sum()), int(down.sum())]


def path_steps(m, quiet_cost=1.0, sparse=True):
    """critical path of the pair form in iterations (the model in the header)"""
    top, own, dirty, down = m["top"], m["own"], m["dirty"], m["down"]
    mbh, mbw = top.shape
    n = mbw + 2
    above = None
    for p in range((mbh + 1) // 2):
        quiet = np.ones(n, bool)
        for half, r in enumerate((2 * p, 2 * p + 1)):
            if r < mbh:
                quiet[half: half + mbw] &= ~own[r]
                quiet[half + 1: half + 1 + mbw] &= ~(dirty[r] | down[r])
        start = np.zeros(n + 1)
        for t in range(n):
            cost = quiet_cost if (quiet[t] and sparse) else 1.0
            mid = start[t] + 0.5 * cost
            if above is not None and t < mbw and (top[2 * p, t] or not sparse):
                mid = max(mid, above[t + 2] + 0.3 + 0.8)
            start[t + 1] = mid + 0.5 * cost
        above = start
    return float(above[n])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--content", default="s1")
    ap.add_argument("--pictures", type=int, default=30)
    ap.add_argument("--search", default="seeded", choices=["seeded", "exhaustive"])
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--qp", type=int, default=26)
    ap.add_argument("--quiet-cost", type=float, nargs="*", default=[1.0, 0.5, 1 / 3])
    ap.add_argument("--gpu-counts", action="store_true")
    a = ap.parse_args()
    from media_amd import synth
    from oracle_lib import OracleEncoder
    frames = synth.sequence(a.content, a.width, a.height, a.pictures)
    search = 1 if a.search == "seeded" else 0
    orc = OracleEncoder(a.width, a.height, qp=a.qp, gop=a.pictures, search=search)
    mbw, mbh = orc.cw // 16, orc.ch // 16
    enc = lib = None
    if a.gpu_counts:
        os.environ["MI355X_H264_PAIR_FILTER"] = "1"
        from media_amd import capi
        enc, lib = capi.Encoder(a.width, a.height, qp=a.qp, gop=a.pictures, search=search), capi.lib()
        got = (ctypes.c_uint * 8)()
        assert lib.mi355x_h264_db_counts2(got, 1) == 0
    print("picture | top quiet clean idle | top_on idle_iterations skipped published%s | steps: every macroblock coupled, sparse at quiet cost %s"
          % (" (GPU: the same four)" if enc else "", ", ".join("%.2f" % q for q in a.quiet_cost)))
    equal, rows = True, []
    for i, f in enumerate(frames):
        au = orc.encode(f)[0]
        m = edge_maps(orc.mbinfo(), orc.mvq(), mbw, mbh)
        intra = int(np.isin(orc.mbinfo()["type"], INTRA_TYPES).sum())
        cnt = pair_counts(m)
        gpu = None
        if enc:
            assert enc.encode(f)[0] == au, "picture %d: the GPU's access unit differs from the oracle's" % i
            enc.debug_read(capi.DBG_RECON_Y)   # (the filter has finished)
            assert lib.mi355x_h264_db_counts2(got, 1) == 0
            gpu = list(got)[4:]
            equal &= gpu == cnt
        clean, idle = ~m["dirty"], ~m["dirty"] & ~m["down"]
        steps = [path_steps(m, 1.0, False)] + [path_steps(m, q) for q in a.quiet_cost]
        rows.append({"picture": i, "intra_mbs": intra, "top": float(m["top"].mean()), "quiet": float((~m["own"]).mean()), "clean": float(clean.mean()),
                     "idle": float(idle.mean()), "counts": cnt, "gpu_counts": gpu, "steps": steps})
        print("%7d | %.2f %.2f %.2f %.2f | %s%s | %s" % (i, m["top"].mean(), (~m["own"]).mean(), clean.mean(), idle.mean(), " ".join(map(str, cnt)),
                                                        " (GPU: %s)" % " ".join(map(str, gpu)) if gpu else "", " ".join("%.1f" % s for s in steps)))
    p = [r for r in rows if r["picture"]]
    mean = [float(np.mean([r["steps"][k] for r in p])) for k in range(len(a.quiet_cost) + 1)]
    print("P pictures, mean steps: " + " ".join("%.1f" % s for s in mean) + "  (relative: " + " ".join("%.3f" % (s / mean[0]) for s in mean) + ")")
    print(json.dumps({"db_sparsity": {"content": a.content, "search": a.search, "pictures": rows, "mean_steps_p": mean,
                                      "gpu_counts_equal": equal if enc else None}}))
    if enc:
        enc.close()
    orc.close()


if __name__ == "__main__":
    main()
