"""k_cavlc's one residual-block coder on waves whose lanes hold every block kind at once.

k_cavlc keeps lane = (macroblock, slot), two macroblocks per wave, and code_slot reaches cavlc_block from ONE call site with
a run-time maxc (4, 15, 16) and nC (-1: chroma DC).  The pictures here are built by hand (64x48: 12 macroblocks, 6 waves) so
that the lanes of a wave hold an Intra16x16 DC, Intra16x16 AC, luma, chroma DC and chroma AC block side by side, and so that
every edge of the run-time maxc and every nC table threshold is met; they go into mi355x_h264_debug_code_syntax and the
access unit must be the oracle's, byte for byte.

The oracle codes whole pictures only from its own random draws, so the expected access unit of a hand-built picture is put
together from the oracle's parts: its parameter sets and slice header (taken from a picture the oracle writes at the same
place of the sequence), its residual block coder (h264o_cavlc_block), its Exp-Golomb codes and its emulation prevention; the
macroblock layer between them (7.3.5, write_mb of oracle/h264_enc.c) is restated in `write_mb` below.  The CPU half proves
that restatement on the oracle's own random pictures (byte for byte), checks that the hand-built pictures hold what they
are meant to hold, and round-trips them through the oracle's decoder: a malformed case shows there and not on the GPU."""
import ctypes as C

import numpy as np
import pytest

import annexb
from oracle_lib import LV_CHROMA_AC, LV_CHROMA_DC, LV_LUMA, LV_LUMA_DC, LV_STRIDE, MBINFO_DTYPE, OracleDecoder, _ptr, lib
from test_entropy_random_oracle import DENSE, SHAPED, SLICE_GUARD_BITS, SLICE_TAIL_BITS, Case, oracle_for, share_bits, slice_geometry

MB_I16, MB_P16, MB_PSKIP, MB_I4 = 0, 1, 2, 4   # media_amd/csrc/dev_common.h
W, H, MBW, MBH, NMB = 64, 48, 4, 3, 12
GOP = 4   # the sequence is I P P P I P P P
CASE = Case(W, H, 66, 0, 0, 0, 20, SHAPED, GOP, 8, 0)
BLK_X = [(b & 1) | ((b >> 1) & 2) for b in range(16)]
BLK_Y = [((b >> 1) & 1) | ((b >> 2) & 2) for b in range(16)]
CBP_INTRA = [47, 31, 15, 0, 23, 27, 29, 30, 7, 11, 13, 14, 39, 43, 45, 46, 16, 3, 5, 10, 12, 19, 21, 26, 28, 35, 37, 42, 44, 1, 2, 4,
             8, 17, 18, 20, 24, 6, 9, 22, 25, 32, 33, 34, 36, 40, 38, 41]   # Table 9-4, codeNum -> coded_block_pattern
CBP_INTER = [0, 16, 1, 2, 4, 8, 32, 3, 5, 10, 12, 15, 47, 7, 11, 13, 14, 6, 9, 31, 35, 37, 42, 44, 33, 34, 36, 40, 39, 43, 45, 46,
             17, 18, 20, 24, 19, 21, 26, 28, 23, 27, 29, 30, 22, 25, 38, 41]


def xy2blk(x, y):
    return (x & 1) | ((y & 1) << 1) | ((x & 2) << 1) | ((y & 2) << 2)


# ---- the oracle's parts ----
class Bits:
    def __init__(self):
        self.v, self.n = 0, 0

    def put(self, n, v):
        self.v, self.n = (self.v << n) | (int(v) & ((1 << n) - 1)), self.n + n

    def ue(self, v):
        code = C.c_uint32()
        self.put(lib().h264o_ue_bits(int(v), C.byref(code)), code.value)

    def se(self, v):
        code = C.c_uint32()
        self.put(lib().h264o_se_bits(int(v), C.byref(code)), code.value)

    def block(self, lv, maxc, nC):
        """residual_block_cavlc by the oracle's coder; returns the bits it took"""
        a, buf = np.zeros(16, np.int16), np.zeros(64, np.uint8)
        a[:maxc] = lv[:maxc]
        n = lib().h264o_cavlc_block(_ptr(a), maxc, nC, _ptr(buf))
        self.put(n, int.from_bytes(bytes(buf), "big") >> (512 - n))
        return n

    def rbsp(self):
        """with rbsp_trailing_bits"""
        self.put(1, 1)
        pad = -self.n % 8
        return (self.v << pad).to_bytes((self.n + pad) // 8, "big")


def unescape(payload):
    out, zeros = bytearray(), 0
    for b in payload:
        if zeros >= 2 and b == 3:
            zeros = 0
            continue
        out.append(b)
        zeros = zeros + 1 if b == 0 else 0
    return bytes(out)


def escape(rbsp):
    a, out = np.frombuffer(rbsp, np.uint8), np.zeros(2 * len(rbsp) + 4, np.uint8)
    return bytes(out[:lib().h264o_nal_escape(_ptr(a), len(rbsp), _ptr(out))])


# ---- the macroblock layer, restated (one slice, Baseline, one reference picture, every vector zero) ----
def n_c(mb, i, idx_in_a, idx_out_a, a_in, idx_in_b, idx_out_b, b_in):
    """9.2.1: (nC, where nA came from, where nB came from) - 'in' this macroblock, the neighbouring 'mb', or 'none'"""
    mx, my = i % MBW, i // MBW
    nA = nB = -1
    sa = sb = "none"
    if a_in:
        nA, sa = int(mb["tc"][i][idx_in_a]), "in"
    elif mx > 0:
        nA, sa = int(mb["tc"][i - 1][idx_out_a]), "mb"
    if b_in:
        nB, sb = int(mb["tc"][i][idx_in_b]), "in"
    elif my > 0:
        nB, sb = int(mb["tc"][i - MBW][idx_out_b]), "mb"
    n = (nA + nB + 1) >> 1 if nA >= 0 and nB >= 0 else (nA if nA >= 0 else (nB if nB >= 0 else 0))
    return n, sa, sb


def nc_luma(mb, i, b):
    x, y = BLK_X[b], BLK_Y[b]
    return n_c(mb, i, xy2blk(x - 1, y), xy2blk(3, y), x > 0, xy2blk(x, y - 1), xy2blk(x, 3), y > 0)


def nc_chroma(mb, i, pl, b):
    x, y, base = b & 1, b >> 1, 16 + 4 * pl
    return n_c(mb, i, base + 2 * y, base + 2 * y + 1, x > 0, base + x, base + 2 + x, y > 0)


def write_mb(bw, mb, lv, aux, i, p_slice, log):
    m, l = mb[i], lv[i]
    t, cbp = int(m["type"]), int(m["cbp"])
    cbpl, cbpc = cbp & 15, cbp >> 4
    mx, my = i % MBW, i // MBW

    def block(kind, at, maxc, nc):
        n = bw.block(l[at:at + maxc], maxc, nc[0])
        log.append(dict(mb=i, kind=kind, maxc=maxc, nC=nc[0], src=nc[1:], tc=int(np.count_nonzero(l[at:at + maxc])), bits=n,
                        last_only=bool(l[at + maxc - 1] != 0 and np.count_nonzero(l[at:at + maxc]) == 1)))

    if t == MB_I4:
        bw.ue(5 if p_slice else 0)
        for k in range(16):
            x, y = BLK_X[k], BLK_Y[k]
            dc_only = False
            if x > 0:
                mA = aux[i][xy2blk(x - 1, y)]
            elif mx == 0:
                dc_only, mA = True, 2
            else:
                mA = aux[i - 1][xy2blk(3, y)] if mb[i - 1]["type"] == MB_I4 else 2
            if y > 0:
                mB = aux[i][xy2blk(x, y - 1)]
            elif my == 0:
                dc_only, mB = True, 2
            else:
                mB = aux[i - MBW][xy2blk(x, 3)] if mb[i - MBW]["type"] == MB_I4 else 2
            pm, mode = 2 if dc_only else min(int(mA), int(mB)), int(aux[i][k])
            if mode == pm:
                bw.put(1, 1)
            else:
                bw.put(4, mode if mode < pm else mode - 1)
        bw.ue(m["chroma_mode"])
        bw.ue(CBP_INTRA.index(cbp))
        if cbp:
            bw.se(0)
    elif t == MB_I16:
        bw.ue((5 if p_slice else 0) + 1 + int(m["i16_mode"]) + 4 * cbpc + (12 if cbpl else 0))
        bw.ue(m["chroma_mode"])
        bw.se(0)
        block("dc16", LV_LUMA_DC, 16, nc_luma(mb, i, 0))
    else:
        assert t == MB_P16 and p_slice and not m["mvx"] and not m["mvy"]
        bw.ue(0)
        bw.se(0)   # mvd_l0: every vector of these pictures is zero, and so is every predictor
        bw.se(0)
        bw.ue(CBP_INTER.index(cbp))
        if cbp:
            bw.se(0)
    for b in range(16):
        if cbpl & (1 << (b >> 2)):
            if t == MB_I16:
                block("ac", LV_LUMA + 16 * b + 1, 15, nc_luma(mb, i, b))
            else:
                block("luma", LV_LUMA + 16 * b, 16, nc_luma(mb, i, b))
    if cbpc:
        block("cdc", LV_CHROMA_DC, 4, (-1, "none", "none"))
        block("cdc", LV_CHROMA_DC + 4, 4, (-1, "none", "none"))
    if cbpc == 2:
        for k in range(8):
            block("cac", LV_CHROMA_AC + 16 * k + 1, 15, nc_chroma(mb, i, k >> 2, k & 3))


def write_access_unit(oracle_au, header_bits, idr, mb, lv, aux):
    """the oracle's access unit with its slice data replaced by the given macroblocks': (access unit, block log, slice bits)"""
    cut = oracle_au.rindex(b"\x00\x00\x01") + 4   # parameter sets, start code and NAL header byte of the (only) slice
    old = unescape(annexb.split_nal_units(oracle_au)[-1][2])
    bw, log, run = Bits(), [], 0
    bw.put(header_bits, int.from_bytes(old, "big") >> (8 * len(old) - header_bits))
    for i in range(NMB):
        if not idr:
            if mb[i]["type"] == MB_PSKIP:
                run += 1
                continue
            bw.ue(run)
            run = 0
        write_mb(bw, mb, lv, aux, i, not idr, log)
    if run:
        bw.ue(run)
    bits = bw.n + 1
    return oracle_au[:cut] + escape(bw.rbsp()), log, bits


# ---- the hand-built pictures ----
class Pic:
    def __init__(self, name, idr):
        self.name, self.idr = name, idr
        self.mb = np.zeros(NMB, MBINFO_DTYPE)
        self.lv = np.zeros((NMB, LV_STRIDE), np.int16)
        self.aux = np.full((NMB, 16), 2, np.uint8)   # Intra4x4 DC everywhere: legal at every picture edge
        self.mvq = np.zeros((NMB, 8), np.int16)
        if idr:
            for i in range(NMB):
                self.i16(i, 0)
        else:
            self.mb["type"] = MB_PSKIP

    def i16(self, i, cbp):
        self.mb[i] = (0, 0, MB_I16, 2, 0, cbp, [0] * 24)   # Intra16x16 DC prediction, chroma DC prediction
        self.lv[i, LV_LUMA:LV_LUMA + 256:16] = 5   # scan position 0 of the AC lists: never coded (the DC list holds it), never to be read

    def i4(self, i, cbp):
        self.mb[i] = (0, 0, MB_I4, 0, 0, cbp, [0] * 24)

    def p16(self, i, cbp):
        assert not self.idr and cbp   # (without coefficients and with the predicted vector it would be P_Skip)
        self.mb[i] = (0, 0, MB_P16, 0, 0, cbp, [0] * 24)

    def put(self, i, at, values):
        self.lv[i, at:at + len(values)] = values

    def luma(self, i, b, values):
        """16 scan positions of luma block b; an Intra16x16 macroblock takes positions 1..15 of them as its AC list"""
        first = 1 if self.mb[i]["type"] == MB_I16 else 0
        self.lv[i, LV_LUMA + 16 * b + first:LV_LUMA + 16 * b + 16] = values[first:]

    def scatter(self, rng, i, density=0.25):
        """small random levels in every list the macroblock's coded_block_pattern codes"""
        def draw(n):
            v = rng.integers(-3, 4, n) * (rng.random(n) < density)
            big = rng.random(n) < 0.03
            return np.where(big, rng.integers(-40, 41, n), v).astype(np.int16)
        m = self.mb[i]
        if m["type"] == MB_PSKIP:
            return
        if m["type"] == MB_I16:
            self.put(i, LV_LUMA_DC, draw(16))
        for b in range(16):
            if m["cbp"] & (1 << (b >> 2)):
                self.luma(i, b, draw(16))
        if m["cbp"] >> 4:
            self.put(i, LV_CHROMA_DC, draw(8))
        if m["cbp"] >> 4 == 2:
            for k in range(8):
                self.put(i, LV_CHROMA_AC + 16 * k + 1, draw(15))

    def finish(self):
        """tc consistent with levels, as the decision kernels leave it: TotalCoeff of the coded luma and chroma AC lists"""
        for i in range(NMB):
            m, l = self.mb[i], self.lv[i]
            first = 1 if m["type"] == MB_I16 else 0
            for b in range(16):
                if m["type"] != MB_PSKIP and m["cbp"] & (1 << (b >> 2)):
                    m["tc"][b] = np.count_nonzero(l[LV_LUMA + 16 * b + first:LV_LUMA + 16 * b + 16])
            if m["type"] != MB_PSKIP and m["cbp"] >> 4 == 2:
                for k in range(8):
                    m["tc"][16 + k] = np.count_nonzero(l[LV_CHROMA_AC + 16 * k + 1:LV_CHROMA_AC + 16 * k + 16])
        return self

    def arrays(self):
        return self.mb, self.lv, self.mvq, self.aux, np.zeros(W * H * 3 // 2, np.uint8)


BIG = np.array([300, -310, 320, -330, 340, -350, 360, -370, 380, -390, 400, -410, 420, -430, 440, -450], np.int16)   # escape codes: 28 bits each
FULL = np.array([2, -1, 3, 1, -2, 1, 1, -1, 4, 1, -1, 2, 1, -1, 1, -1], np.int16)   # a list without a zero: no total_zeros
LAST = np.array([0] * 15 + [1], np.int16)   # the only coefficient at the last scan position


def _edges(p, inter_or_i4, i16):
    """the edges of the run-time maxc, in macroblock `inter_or_i4` (maxc 16, 4, 15) and the Intra16x16 macroblock `i16`"""
    a, b = inter_or_i4, i16
    p.luma(a, 0, LAST)                     # a luma block whose only coefficient is at scan position 15
    p.luma(a, 1, FULL)                     # tc == maxc == 16
    p.luma(a, 2, [7] + [0] * 15)           # only scan position 0
    p.put(a, LV_CHROMA_DC, [1, -2, 3, -1, 9, 0, 0, 0])   # Cb DC: tc == maxc == 4, followed by a non-zero entry (Cr DC) that is no fifth coefficient
    p.put(a, LV_CHROMA_AC + 1, FULL[1:])   # chroma AC: tc == maxc == 15
    p.put(a, LV_CHROMA_AC + 16, [6, 0])    # (scan position 0 of the next AC list: never coded, lies where a sixteenth entry would)
    p.put(a, LV_CHROMA_AC + 16 + 1, LAST[1:])   # chroma AC: the only coefficient at its last position
    p.put(b, LV_LUMA_DC, FULL)             # Intra16x16 DC: tc == maxc == 16
    p.luma(b, 0, LAST)                     # Intra16x16 AC: the only coefficient at its last position (lv[15] of the block)
    p.luma(b, 1, FULL)                     # tc == maxc == 15
    p.put(b, LV_CHROMA_DC, [0, 0, 0, 0, -1, 2, -3, 1])   # Cr DC: 4 levels, followed by position 0 of the first AC list
    p.put(b, LV_CHROMA_AC, [9])            # never coded


def _nc_picture(name, left, above):
    """luma block 0 of macroblocks 1..3 has nC = left[k] from the macroblock to its left alone (nothing above the first row);
    of macroblocks 4 and 8, nC = above[k] from the macroblock above alone (nothing left of the first column); the macroblocks
    5..7 and 9..11 average both neighbours; macroblock 0 has neither"""
    p = Pic(name, False)
    for i in range(NMB):
        p.p16(i, 0x0F)
        p.luma(i, 0, [1] + [0] * 15)
    for k, n in enumerate(left):
        p.luma(k, 5, [1] * n + [0] * (16 - n))        # block 5 = (3, 0): the left neighbour of the next macroblock's block 0
    for k, n in enumerate(above):
        p.luma(4 * k, 10, [-1] * n + [0] * (16 - n))  # block 10 = (0, 3): above block 0 of the macroblock below
    for i in (4, 5, 6, 9, 10):
        p.luma(i, 5, [2] * (i - 2) + [0] * (18 - i))
    for i in (1, 2, 3, 6, 7):
        p.luma(i, 10, [1, -1] * (i // 2 + 1) + [0] * (14 - 2 * (i // 2)))
    p.luma(5, 10, [-1] + [0] * 15)   # block 0 of macroblock 9: nA 0, nB 1
    return p.finish()


def build_pictures():
    rng = np.random.default_rng(20)
    pics = []
    # 0 (IDR): Intra16x16 with DC, AC, chroma DC and chroma AC beside Intra4x4 in one wave; chroma DC alone; everything mixed
    p = Pic("mixed_idr", True)
    for i, (kind, cbp) in enumerate([("i16", 0x2F), ("i4", 0x2F), ("i4", 0x10), ("i16", 0x10), ("i4", 0x25), ("i16", 0x0F), ("i16", 0x00),
                                     ("i4", 0x1A), ("i16", 0x2F), ("i16", 0x20), ("i4", 0x00), ("i4", 0x2F)]):
        getattr(p, kind)(i, cbp)
        p.scatter(rng, i, 0.3)
    p.put(2, LV_CHROMA_AC, [3, -3, 1])   # macroblock 2 codes chroma DC alone (cbp chroma 1): AC levels left behind are not its business
    pics.append(p.finish())
    # 1 (P): the Intra16x16 macroblock with everything beside P16x16 with luma only, then beside Intra4x4; chroma DC alone; skip runs
    p = Pic("mixed_p", False)
    for i, (kind, cbp) in enumerate([("i16", 0x2F), ("p16", 0x0F), ("i16", 0x2F), ("i4", 0x2F), ("p16", 0x10), (None, 0), ("p16", 0x2F),
                                     ("i4", 0x10), (None, 0), (None, 0), ("p16", 0x03), (None, 0)]):
        if kind:
            getattr(p, kind)(i, cbp)
            p.scatter(rng, i, 0.3)
    p.put(4, LV_CHROMA_DC, [1, 2, -1, 1, 0, 0, 0, -2])
    pics.append(p.finish())
    # 2 (P): the edges of maxc
    p = Pic("edges_p", False)
    p.p16(0, 0x2F)
    p.i16(1, 0x2F)
    _edges(p, 0, 1)
    p.i4(6, 0x2F)
    p.scatter(rng, 6)
    pics.append(p.finish())
    # 3 (P): one slot over 64 bits of each block kind (the count pass and the write pass both code these)
    p = Pic("long_slots_p", False)
    p.i16(0, 0x2F)
    p.put(0, LV_LUMA_DC, BIG)
    p.luma(0, 0, BIG)
    p.put(0, LV_CHROMA_DC, BIG[:8])
    p.put(0, LV_CHROMA_AC + 1, BIG[1:])
    p.p16(1, 0x2F)
    p.scatter(rng, 1)
    p.luma(1, 3, -BIG)
    p.put(1, LV_CHROMA_AC + 16 * 7 + 1, BIG[:15])   # the last list of the levels row
    p.i4(5, 0x08)
    p.luma(5, 15, BIG)
    pics.append(p.finish())
    # 4 (IDR): the edges of maxc once more, Intra4x4 in place of P16x16; a long slot of each kind in an IDR picture
    p = Pic("edges_idr", True)
    p.i4(0, 0x2F)
    p.i16(1, 0x2F)
    _edges(p, 0, 1)
    p.i16(6, 0x2F)
    p.put(6, LV_LUMA_DC, -BIG)
    p.luma(6, 9, BIG)
    p.put(6, LV_CHROMA_DC, -BIG[:8])
    p.put(6, LV_CHROMA_AC + 16 * 5 + 1, BIG[1:])
    p.i4(7, 0x01)
    p.luma(7, 0, BIG)
    pics.append(p.finish())
    # 5, 6 (P): nC at both sides of the table thresholds 2, 4 and 8, and 0 / 1
    pics.append(_nc_picture("nc_1_2_3", (1, 2, 3), (1, 2)))
    pics.append(_nc_picture("nc_4_7_8", (4, 7, 8), (4, 8)))
    # 7 (P): everything mixed
    p = Pic("mixed_p2", False)
    for i in range(NMB):
        kind = ("i16", "p16", "i4", None)[int(rng.integers(0, 4))]
        cbp = int(rng.integers(1, 16)) | (int(rng.integers(0, 3)) << 4)
        if kind:
            getattr(p, kind)(i, (cbp & 0x30) | (15 if cbp & 8 else 0) if kind == "i16" else cbp)
            p.scatter(rng, i, 0.4)
    pics.append(p.finish())
    assert [q.idr for q in pics] == [k % GOP == 0 for k in range(len(pics))]
    return pics


def expected_sequence(pics, idr_id=0, idr_step=1):
    """the oracle's access units for the pictures coded one after the other: [(access unit, block log, slice bits)]"""
    o, out = oracle_for(CASE), []
    o.set_idr_id(idr_id, idr_step)
    try:
        for k, p in enumerate(pics):
            au, idr, _ = o.random_picture(1 + k, features=CASE.features)   # the headers of picture k of the sequence
            assert idr == p.idr
            out.append(write_access_unit(au, int(o.mb_bitpos()[0]), idr, p.mb, p.lv, p.aux))
    finally:
        o.close()
    return out


@pytest.fixture(scope="module")
def pictures():
    return build_pictures()


@pytest.fixture(scope="module")
def expected(pictures):
    return expected_sequence(pictures)


# ---- CPU half ----
def test_macroblock_layer_restatement_equals_the_oracle():
    """write_access_unit on the arrays of the oracle's own random IDR pictures (Intra16x16 and Intra4x4 macroblocks with random
    modes, patterns and dense levels) gives the oracle's access unit, byte for byte"""
    c = CASE._replace(features=SHAPED | DENSE)
    o = oracle_for(c)
    try:
        for k in range(6):
            au, idr, _ = o.random_picture(300 + k, force_idr=True, features=c.features)
            got, log, bits = write_access_unit(au, int(o.mb_bitpos()[0]), idr, o.mbinfo(), o.levels(), o.mbaux())
            assert got == au, "picture %d" % k
            assert bits == o.slice_bits()[0]
            assert {e["kind"] for e in log} >= {"dc16", "luma", "cdc", "cac"}
    finally:
        o.close()


def test_pictures_decode_and_fit(pictures, expected):
    mbw, rows = slice_geometry(CASE)
    kinds = {MB_I16: OracleDecoder.KIND_I16, MB_I4: OracleDecoder.KIND_I4, MB_P16: OracleDecoder.KIND_INTER, MB_PSKIP: OracleDecoder.KIND_SKIP}
    dec = OracleDecoder()
    try:
        for p, (au, _, bits) in zip(pictures, expected):
            assert dec.decode(au) == 1, p.name
            assert dec.max_level_prefix <= 15, p.name
            assert list(dec.mb_kinds()) == [kinds[int(t)] for t in p.mb["type"]], p.name
            assert all(dec.mb_mv(i) == (0, 0, 0) for i in range(NMB) if p.mb["type"][i] in (MB_P16, MB_PSKIP)), p.name
            assert bits <= share_bits(mbw, rows[0]) - (SLICE_GUARD_BITS + SLICE_TAIL_BITS), (p.name, bits)   # no I_PCM fallback on this path
    finally:
        dec.close()


def test_pictures_hold_what_they_are_built_for(pictures, expected):
    logs = {p.name: log for p, (_, log, _) in zip(pictures, expected)}

    def wave_kinds(name, wave):
        return {e["kind"] for e in logs[name] if e["mb"] // 2 == wave}
    # every block kind in one wave: Intra16x16 with everything beside P16x16 with luma only, beside Intra4x4; chroma DC alone
    assert wave_kinds("mixed_p", 0) == {"dc16", "ac", "luma", "cdc", "cac"} and pictures[1].mb["cbp"][1] == 0x0F
    assert wave_kinds("mixed_p", 1) == {"dc16", "ac", "luma", "cdc", "cac"} and pictures[1].mb["type"][3] == MB_I4
    assert wave_kinds("mixed_idr", 0) == {"dc16", "ac", "luma", "cdc", "cac"}
    assert {e["kind"] for e in logs["mixed_p"] if e["mb"] == 4} == {"cdc"} and {e["kind"] for e in logs["mixed_idr"] if e["mb"] == 2} == {"cdc"}
    for name in ("edges_p", "edges_idr"):
        log = logs[name]
        assert {(e["kind"], e["maxc"]) for e in log if e["tc"] == e["maxc"]} >= {("dc16", 16), ("luma", 16), ("ac", 15), ("cac", 15), ("cdc", 4)}, name
        assert {e["kind"] for e in log if e["last_only"]} >= {"luma", "ac", "cac"}, name
        assert pictures[2].lv[0, LV_CHROMA_DC + 4] != 0 and pictures[2].lv[1, LV_CHROMA_AC] != 0   # what follows the full chroma DC lists
    # one slot over 64 bits of each kind, in a P and in an IDR picture
    for name in ("long_slots_p", "edges_idr"):
        assert {e["kind"] for e in logs[name] if e["bits"] > 64} == {"dc16", "ac", "luma", "cdc", "cac"}, name
    # nC: both sides of every threshold, from the left macroblock alone, from the macroblock above alone, and without a neighbour
    nc = [e for name in ("nc_1_2_3", "nc_4_7_8") for e in logs[name] if e["kind"] == "luma"]
    assert {e["nC"] for e in nc if e["src"] == ("mb", "none")} >= {1, 2, 3, 4, 7, 8}
    assert {e["nC"] for e in nc if e["src"] == ("none", "mb")} >= {1, 2, 4, 8}
    assert {e["nC"] for e in nc if e["src"] == ("none", "none")} == {0}
    both = {e["nC"] for e in nc if e["src"] == ("mb", "mb")}
    assert both & {0, 1} and both & {2, 3} and both & {4, 5, 6, 7} and both & set(range(8, 17)), both
    assert {e["nC"] for e in logs["mixed_p"] + logs["mixed_idr"] if e["kind"] == "cac"} >= {0, 1, 2}


# ---- GPU half ----
def _encoder(batch=1):
    from media_amd import capi
    return capi, capi.Encoder(W, H, qp=CASE.qp, gop=GOP, profile_idc=CASE.profile, batch=batch)


@pytest.mark.gpu
def test_mixed_slot_pictures_code_to_the_oracles_bytes(pictures, expected):
    capi, enc = _encoder()
    try:
        for p, (want, _, _) in zip(pictures, expected):
            rc, (got,), ft = enc.code_syntax(*p.arrays())
            assert rc == 0, "%s: rc %d (%s)" % (p.name, rc, enc.last_error())
            assert ft == (capi.FRAME_IDR if p.idr else capi.FRAME_P), p.name
            assert got == want, "%s: first difference at byte %d of %d (oracle: %d)" % (
                p.name, next((i for i, (a, b) in enumerate(zip(got, want)) if a != b), min(len(got), len(want))), len(got), len(want))
    finally:
        enc.close()


@pytest.mark.gpu
def test_mixed_slot_pictures_as_a_lockstep_batch_of_two(pictures, expected):
    """item 1 codes the same pictures four places on (the picture types of a lockstep step are the same for every item)"""
    other = pictures[GOP:] + pictures[:GOP]
    want1 = expected_sequence(other, 1, 2)
    want0 = expected_sequence(pictures, 0, 2)
    capi, enc = _encoder(2)
    try:
        for k, (a, b) in enumerate(zip(pictures, other)):
            rc, got, _ = enc.code_syntax(*[np.concatenate([np.ascontiguousarray(x).reshape(-1).view(np.uint8), np.ascontiguousarray(y).reshape(-1).view(np.uint8)])
                                           for x, y in zip(a.arrays(), b.arrays())])
            assert rc == 0, "step %d: rc %d (%s)" % (k, rc, enc.last_error())
            assert got[0] == want0[k][0], "step %d item 0 (%s)" % (k, a.name)
            assert got[1] == want1[k][0], "step %d item 1 (%s)" % (k, b.name)
    finally:
        enc.close()
