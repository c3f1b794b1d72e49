"""The decoder's prediction, cell by cell: the streams, the cells a stream list has to reach, and the floor.  Shared by
tests/test_pred_cells_oracle.py (CPU: the list reaches what it claims, from the oracle decoder's own account h264o_dec_pred) and
tests/test_gpu_pred_cells.py (GPU).  Nothing of the decoder under test is used here.

Two kinds of stream.

"rand": h264o_enc_random_picture - partitions down to 4x4 with a vector and a reference index each, slices cut anywhere,
constrained_intra_pred_flag, intra macroblocks among inter ones.  Feature 262144 ("prediction cells") draws every vector so that an
edge of the window 8.4.2.2.1 reads lies up to 5 samples inside or 8 outside an edge of the picture and makes four in ten
macroblocks of a P slice intra ones: what independent draws reach a few times in a thousand macroblocks.

"enc": access units of the oracle ENCODER on the content of tests/adversarial.py.  Random residual makes noisy reference pictures,
where Clip1 of the interpolation is active all the time but on no smooth ramp; the encoder's own pictures are the ones a motion
search has matched.

Everything is deterministic and computed once per process."""
import functools
from collections import namedtuple

import numpy as np

import adversarial
import range_ends
from media_amd import synth
from oracle_lib import OracleEncoder, OracleDecoder, Pred

FLOOR = 8            # times every legal cell is met, over the whole list (the floor tests/deblock_cells.py uses for a changed line)
BASE, RE = range_ends.BASE, range_ends.RE
CI, PC = OracleEncoder.RAND_CONSTRAINED_INTRA, OracleEncoder.RAND_PRED_CELLS
GOP = 6

Case = namedtuple("Case", "name kind w h prof slices refs content features pictures")


def _rand(w, h, prof, slices, refs, features, pictures=12, tag=""):
    name = "rand_%dx%d_%d_r%d%s%s%s%s" % (w, h, prof, refs, "_ci" if features & CI else "", "_ends" if features & RE else "", "_pc" if features & PC else "", tag)
    return Case(name, "rand", w, h, prof, slices, refs, None, features, pictures)


def _enc(w, h, prof, slices, refs, content, qp, pictures=6):
    return Case("enc_%dx%d_%d_r%d_%s_q%d" % (w, h, prof, refs, content, qp), "enc", w, h, prof, slices, refs, content, qp, pictures)


CASES = [
    # the generator as the older lists use it: with and without constrained_intra_pred_flag, one to three references
    _rand(16, 16, 66, 0, 1, BASE), _rand(32, 16, 77, 0, 2, BASE | CI), _rand(16, 48, 100, 0, 3, BASE), _rand(48, 48, 66, 0, 2, BASE | RE),
    _rand(64, 48, 77, 0, 3, BASE | CI), _rand(96, 80, 77, 2, 2, BASE | RE | CI, 6), _rand(112, 64, 100, 0, 3, BASE, 6),
    # windows at the picture's edges, four in ten macroblocks of a P slice intra
    _rand(16, 16, 66, 0, 1, BASE | PC), _rand(16, 16, 77, 0, 3, BASE | PC | CI), _rand(32, 16, 77, 0, 2, BASE | PC), _rand(32, 16, 66, 0, 3, BASE | PC | CI),
    _rand(16, 48, 100, 0, 3, BASE | PC | CI), _rand(16, 48, 66, 0, 1, BASE | PC), _rand(48, 48, 66, 0, 2, BASE | PC | CI), _rand(48, 48, 77, 0, 3, BASE | PC),
    _rand(64, 48, 100, 0, 3, BASE | PC), _rand(64, 48, 66, 0, 1, BASE | PC | CI), _rand(64, 48, 77, 0, 2, BASE | PC | CI), _rand(64, 48, 77, 0, 3, BASE | PC | CI, tag="_b"),
    _rand(64, 48, 66, 0, 2, BASE | PC, tag="_b"), _rand(64, 48, 100, 0, 1, BASE | PC | CI),
    _rand(96, 80, 77, 0, 2, BASE | PC | CI, 6), _rand(96, 80, 66, 3, 3, BASE | PC, 6), _rand(112, 64, 100, 0, 3, BASE | PC | CI, 6),
    _rand(16, 16, 100, 0, 2, BASE | PC, tag="_b"), _rand(16, 16, 66, 0, 2, BASE | PC | CI, tag="_b"), _rand(16, 16, 77, 0, 1, BASE | PC, tag="_c"),
    _rand(32, 16, 100, 0, 1, BASE | PC, tag="_b"), _rand(32, 16, 66, 0, 2, BASE | PC | CI, tag="_b"), _rand(16, 48, 77, 0, 2, BASE | PC, tag="_b"),
    _rand(16, 48, 66, 0, 3, BASE | PC | CI, tag="_b"), _rand(48, 48, 100, 0, 1, BASE | PC | CI, tag="_b"), _rand(48, 48, 66, 0, 3, BASE | PC, tag="_b"),
    _rand(96, 80, 66, 0, 1, BASE | PC, 12, tag="_b"), _rand(96, 80, 100, 0, 3, BASE | PC | CI, 12, tag="_b"), _rand(96, 80, 77, 0, 2, BASE | PC, 12, tag="_c"),
    _rand(112, 64, 100, 0, 3, BASE | PC | CI, 12, tag="_b"), _rand(112, 64, 100, 2, 3, BASE | PC, 12, tag="_c"), _rand(96, 80, 77, 0, 3, BASE | PC | CI, 12, tag="_d"),
    # the rare ones: a 16-sample partition with a fraction in a picture 16 wide or high (the window crosses both edges), P_Skip with a
    # fractional vector, Intra4x4 / Intra16x16 beside one inter neighbour under constrained_intra_pred_flag
] + [_rand(w, h, (66, 77, 100)[k % 3], 0, 1 + (k + n) % 3, BASE | PC | (CI if k % 2 else 0), tag="_%c" % (100 + k))
     for n, (w, h, count) in enumerate(((16, 16, 8), (32, 16, 6), (16, 48, 4))) for k in range(count)] + [
    _rand(96, 80, (77, 100, 66)[k % 3], 0, 1 + k % 3, BASE | PC | CI, 12, tag="_%c" % (101 + k)) for k in range(16)] + [
    _rand(64, 48, (100, 66, 77)[k % 3], 0, 1 + k % 3, BASE | PC, 12, tag="_%c" % (101 + k)) for k in range(6)] + [
    # the encoder's own pictures
    _enc(64, 48, 66, 0, 1, "gradient", 24), _enc(64, 48, 100, 0, 3, "contrast", 30), _enc(96, 80, 77, 2, 1, "glyphs", 28), _enc(48, 48, 66, 0, 2, "bars", 26),
]
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)

Picture = namedtuple("Picture", "au idr planes pred stats kinds mv4 i4_hits constrained avail modes")


def frame(content, w, h, i):
    if content in adversarial.GENERATORS:
        return adversarial.GENERATORS[content](w, h, i)
    return synth.sequence(content, w, h, 1, start=i)[0]


def blocks_of(dec, n_mb):
    """(x, y, ref_idx_l0) of every 4x4 block of every macroblock, raster order inside the macroblock (meaningful for inter ones)"""
    return np.array([[dec.mb_mv(a, b) for b in range(16)] for a in range(n_mb)], np.int32)


@functools.lru_cache(maxsize=None)
def stream(case):
    """the case's pictures: the access unit, is_idr, the oracle decoder's three coded planes, its prediction account (Pred), its
    statistics, its macroblock kinds, its vector and reference index per 4x4 block, the writer's Intra4x4PredMode counts ([blkIdx][mode];
    random cases), whether constrained_intra_pred_flag is set, the neighbour availability per macroblock (OracleDecoder.mb_avail), the intra prediction modes per macroblock (OracleDecoder.mb_intra_modes)"""
    enc = OracleEncoder(case.w, case.h, qp=case.features if case.kind == "enc" else 30, gop=1000 if case.kind == "enc" else GOP,
                        profile_idc=case.prof, slices=case.slices, refs=case.refs)
    dec = OracleDecoder()
    out = []
    assert 6 <= case.pictures <= 12
    for i in range(case.pictures):
        enc.hits_reset()
        if case.kind == "enc":
            au, idr = enc.encode(frame(case.content, case.w, case.h, i))
            hits = None
        else:
            au, idr, _ = enc.random_picture(range_ends.seed(case, i) + 104729 * (1 + sum(case.name.encode())), features=case.features)
            hits = enc.hits()["i4_mode"].astype(np.int64)
        assert dec.decode(au) == 1, "%s picture %d: the independent decoder decodes every picture" % (case.name, i)
        planes = tuple(dec.plane(p) for p in range(3))
        for a in planes:
            a.setflags(write=False)
        kinds = dec.mb_kinds()
        out.append(Picture(au, idr, planes, dec.pred(), dec.stats(), kinds, blocks_of(dec, len(kinds)), hits, bool(case.kind == "rand" and case.features & CI), dec.mb_avail(), dec.mb_intra_modes()))
    enc.close(); dec.close()
    return tuple(out)


def account(cases):
    """the sum of the prediction accounts of every picture of the cases"""
    total = Pred()
    for c in cases:
        for p in stream(c):
            total = total + p.pred
    return total


def account_of(aus):
    """the prediction account of a list of access units, decoded by a decoder of their own"""
    dec, total = OracleDecoder(), Pred()
    for au in aus:
        if dec.decode(au) == 1:
            total = total + dec.pred()
    dec.close()
    return total


# ---------------------------------------------------------------- the cells a list has to reach
# Every cell of a section is legal unless a rule below excludes it; the rules are the standard's, restated here and nowhere taken
# from the account.
INSIDE, CROSS_LOW, CROSS_HIGH, BEYOND_LOW, BEYOND_HIGH, CROSS_BOTH = range(6)
LEFT, TOP, TOPLEFT, TOPRIGHT = 1, 2, 4, 8


def blk_xy(k):
    """6.4.3: the 4x4 luma block blkIdx lies at (x, y), in units of four samples"""
    return (k & 1) + 2 * ((k >> 2) & 1), ((k >> 1) & 1) + 2 * (k >> 3)


BLK_AT = {blk_xy(k): k for k in range(16)}
# 8.3.1.2: the neighbouring samples each Intra4x4PredMode needs to be "available for Intra_4x4 prediction"
I4_NEEDS = {0: TOP, 1: LEFT, 2: 0, 3: TOP, 4: LEFT | TOP | TOPLEFT, 5: LEFT | TOP | TOPLEFT, 6: LEFT | TOP | TOPLEFT, 7: TOP, 8: LEFT}
# 8.3.3 / 8.3.4: the same for Intra16x16PredMode (vertical, horizontal, DC, plane) and intra_chroma_pred_mode (DC, horizontal, vertical, plane)
I16_NEEDS = {0: TOP, 1: LEFT, 2: 0, 3: LEFT | TOP | TOPLEFT}
IC_NEEDS = {0: 0, 1: LEFT, 2: TOP, 3: LEFT | TOP | TOPLEFT}


def tr_not_yet_decoded(k):
    """6.4.11.4 with 6.4.3: the block above and to the right of blkIdx k lies in this macroblock with a greater blkIdx, or in the
    macroblock to the right"""
    x, y = blk_xy(k)
    return y > 0 and (x == 3 or BLK_AT[(x + 1, y - 1)] > k)


def i4_availabilities():
    """every (left | top << 1 | top-left << 2 | top-right << 3) a block can have: per blkIdx, from every combination of the four
    neighbouring macroblocks A, B, C, D being available or not (6.4.11.4; with constrained_intra_pred_flag any of them may be an
    inter macroblock on its own, so all sixteen combinations occur)"""
    out = set()
    for k in range(16):
        x, y = blk_xy(k)
        for a in (0, 1):
            for b in (0, 1):
                for c in (0, 1):
                    for d in (0, 1):
                        left = 1 if x > 0 else a
                        top = 1 if y > 0 else b
                        tl = 1 if (x > 0 and y > 0) else b if x > 0 else a if y > 0 else d
                        tr = (b if x < 3 else c) if y == 0 else 0 if tr_not_yet_decoded(k) else 1
                        out.add(left | top << 1 | tl << 2 | tr << 3)
    return out


def legal_cells():
    """{section: boolean array, True where a stream can reach the cell}"""
    legal = {name: np.ones(shape, bool) for name, shape in Pred.SECTIONS}
    # 8.4.2.2.1 reads at most 16 columns (rows) with a fraction of 0, and a picture is at least 16 wide (high): 7.4.2.1.1, PicWidthInMbs >= 1
    legal["l_rel"][:, 0, CROSS_BOTH] = False
    # 8.4.2.2.2 reads at most 8 + 1 chroma columns (rows); a window across both edges of a plane of at least 8 needs 10
    legal["c_rel"][:, :, CROSS_BOTH] = False
    # Table 8-12: the intermediates of each position (0 b-type, 1 h-type, 2 j); G itself is not clipped
    uses = {1: (0,), 2: (0,), 3: (0,), 4: (1,), 8: (1,), 12: (1,), 5: (0, 1), 7: (0, 1), 13: (0, 1), 15: (0, 1), 10: (2,), 6: (0, 2), 14: (0, 2), 9: (1, 2), 11: (1, 2)}
    legal["l_clip"][:] = False
    for pos, kinds in uses.items():
        legal["l_clip"][pos, list(kinds)] = True
    legal["i4"][:] = False
    for avail in i4_availabilities():
        for mode, needs in I4_NEEDS.items():
            legal["i4"][mode, avail] = needs & avail == needs
    # 6.4.11.4: "not yet decoded" is the fate of a top-right neighbour alone (left, top and top-left precede the block in decoding order)
    legal["i4_nb"][:3, Pred.REASONS.index("not_yet_decoded")] = False
    legal["i4_tr_nyd"][:] = [tr_not_yet_decoded(k) for k in range(16)]
    for name, needs in (("i16", I16_NEEDS), ("ic", IC_NEEDS)):
        for mode in range(4):
            for avail in range(8):
                legal[name][mode, avail] = needs[mode] & avail == needs[mode]
    return legal


LEGAL = legal_cells()
# cells no stream can reach beyond what LEGAL excludes, each with the subclause that forbids it (failing to find a stream is no argument)
UNREACHABLE = {}


def thin(pred, floor=FLOOR):
    """[(section, index, count)] of the legal cells met fewer than `floor` times, thinnest first"""
    out = []
    for name, _ in Pred.SECTIONS:
        a = pred[name]
        for idx in zip(*np.nonzero(LEGAL[name] & (a < floor))):
            if (name, tuple(int(i) for i in idx)) not in UNREACHABLE:
                out.append((name, tuple(int(i) for i in idx), int(a[idx])))
    return sorted(out, key=lambda t: t[2])


def coverage(pred):
    """the summary of an account that DESIGN.md tabulates: per family the legal cells never met / met fewer than FLOOR times"""
    fam = {"inter luma": ("l_shape", "l_ref", "l_rel", "l_cross", "l_corner"), "luma 4x4": ("b_ref", "b_align", "b_rdist"), "luma clip": ("l_clip",),
           "inter chroma": ("c_frac", "c_rel", "c_cross", "c_rdist", "c_pair", "c_pair_mixed"), "intra 4x4": ("i4", "i4_nb", "i4_tr_nyd", "i4_tr"),
           "intra 16x16 / chroma": ("i16", "ic", "ic_dc", "plane_clip"), "intra beside inter": ("ibi",)}
    out = {}
    for f, names in fam.items():
        cells = sum(int(LEGAL[n].sum()) for n in names)
        never = sum(int((LEGAL[n] & (pred[n] == 0)).sum()) for n in names)
        below = sum(int((LEGAL[n] & (pred[n] < FLOOR)).sum()) for n in names)
        out[f] = (cells, never, below)
    return out


def relation(lo, hi, n):
    """Pred.RELATIONS of the window lo .. hi against 0 .. n - 1"""
    return Pred.RELATIONS[BEYOND_LOW if hi < 0 else BEYOND_HIGH if lo > n - 1 else CROSS_BOTH if lo < 0 and hi > n - 1 else CROSS_LOW if lo < 0 else CROSS_HIGH if hi > n - 1 else INSIDE]


def describe(pic, w, h, plane, x, y):
    """what the independent decoder's side information says about the sample (x, y) of a plane of a w x h picture (coded size): its
    macroblock and kind; inter: the vector, fractions and reference index of its 4x4 luma block and where the window of that block lies
    against the picture; intra: the prediction mode and the neighbour availability"""
    s = 1 if plane == 0 else 2
    lx, ly = x * s, y * s
    mbw = w // 16
    mb = (ly // 16) * mbw + lx // 16
    kind = int(pic.kinds[mb])
    name = {1: "Intra4x4", 2: "Intra16x16", 3: "I_PCM", 4: "inter", 5: "P_Skip"}.get(kind, "kind %d" % kind)
    bx, by = (lx % 16) // 4, (ly % 16) // 4
    out = "macroblock %d (%d, %d) %s" % (mb, lx // 16, ly // 16, name)
    if kind in (4, 5):
        vx, vy, ref = (int(v) for v in pic.mv4[mb, 4 * by + bx])
        if plane == 0:
            fx, fy = vx & 3, vy & 3
            x0, y0 = 4 * (lx // 4) + (vx >> 2), 4 * (ly // 4) + (vy >> 2)
            rel = (relation(x0 - (2 if fx else 0), x0 + 3 + (3 if fx else 0), w), relation(y0 - (2 if fy else 0), y0 + 3 + (3 if fy else 0), h))
        else:
            fx, fy = vx & 7, vy & 7
            x0, y0 = 2 * (lx // 4) + (vx >> 3), 2 * (ly // 4) + (vy >> 3)
            rel = (relation(x0, x0 + 1 + (1 if fx else 0), w // 2), relation(y0, y0 + 1 + (1 if fy else 0), h // 2))
        out += ", 4x4 block (%d, %d): vector (%d, %d), fraction (%d, %d), ref_idx_l0 %d, window from (%d, %d) %s horizontally / %s vertically" % (
            bx, by, vx, vy, fx, fy, ref, x0, y0, rel[0], rel[1])
    elif kind in (1, 2):
        a = int(pic.avail[mb]) >> 4
        avail = "left %d top %d top-right %d top-left %d%s" % (a & 1, a >> 1 & 1, a >> 2 & 1, a >> 3 & 1, " (constrained_intra_pred_flag)" if pic.constrained else "")
        if plane:
            out += ", intra_chroma_pred_mode %d, available: %s" % (pic.modes[mb, 17], avail)
        elif kind == 2:
            out += ", Intra16x16PredMode %d, available: %s" % (pic.modes[mb, 16], avail)
        else:
            out += ", 4x4 block (%d, %d) blkIdx %d Intra4x4PredMode %d, macroblocks available: %s" % (bx, by, BLK_AT[(bx, by)], pic.modes[mb, 4 * by + bx], avail)
    return out
