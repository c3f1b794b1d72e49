"""Sequences and comparisons for the sparse stores of k_tq / k_tq8 (media_amd/csrc/k_tq.h): the kernels store the levels of an
8x8 luma quadrant, of the chroma DC and of the chroma AC part only where coded_block_pattern says that the part is coded, and a
block's reconstructed samples and TotalCoeff byte only where the block has a level (chroma: or a non-zero scaled DC term).
Everything else in `levels` is left from an EARLIER picture.  The failure this invites: a stage reads levels, samples or TotalCoeff
bytes that were last written for another picture.  So the sequences here put dense pictures in front of sparse ones: one GOP
whose picture QP jumps up and down, so that parts coded in one picture are empty - with the old levels still lying there - in
the next.

tests/test_tq_sparse_oracle.py proves on the CPU oracle alone that the sequence holds what it is meant to hold;
tests/test_gpu_tq_sparse.py runs it on the GPU, through the single encoder, a lockstep batch, a hub stream and the High profile,
and compares every picture with the oracle.  Everything is deterministic."""
import functools
from collections import namedtuple
import numpy as np
from media_amd import synth

SIZE = (176, 144)    # 99 macroblocks: a row of 11 straddles the waves of 8, the last wave holds 3 (k_tq8: waves of 16, the last holds 3)
SMALL = (48, 32)     # 6 macroblocks: fewer than one wave's 8
KIND = "s1"
QPS = (20, 18, 40, 22, 36, 26, 30, 16, 44, 26)   # one GOP; a dense picture in front of every sparse one
INTER = (1, 2, 5, 6, 7)                          # MbInfo.type: P_L0_16x16, P_Skip, 16x8, 8x16, 8x8

# the lockstep batch: every call is a step of closed GOPs at ONE QP (the direct kernels, IND = false, know one QP per launch), so the
# dense-then-sparse order runs over the calls; the items start at different pictures of the sequence, so that the macroblocks
# of one wave differ from item to item
BATCH_G, BATCH_GOP = 8, 4
BATCH_QPS = (18, 40, 22, 44)


def frames(w, h, n=len(QPS), start=0):
    return synth.sequence(KIND, w, h, n, start=start)


def batch_frames(w, h, call, g):
    return frames(w, h, BATCH_GOP, start=5 * g + 3 * call)


def read_mask(mbinfo):
    """which of the 416 levels of every macroblock some stage reads (7.3.5.3: by macroblock type and coded_block_pattern): the
    Intra16x16 DC list, the 64 levels of a luma quadrant whose bit is set, chroma DC at cbp >> 4 >= 1, chroma AC at cbp >> 4 == 2;
    nothing of an I_PCM macroblock.  What the mask leaves out is unspecified on the GPU"""
    read = np.zeros((len(mbinfo), 416), dtype=bool)
    cbp = mbinfo["cbp"].astype(np.int32)
    read[mbinfo["type"] == 0, 0:16] = True
    for q in range(4):
        read[(cbp >> q) & 1 == 1, 16 + 64 * q: 16 + 64 * (q + 1)] = True
    read[(cbp >> 4) >= 1, 272:280] = True
    read[(cbp >> 4) == 2, 280:408] = True
    read[mbinfo["type"] == 3, :] = False
    return read


Stages = namedtuple("Stages", "mbinfo levels mvq mbaux pre recon")
Pic = namedtuple("Pic", "au idr qp stages")


def stages_of(orc):
    return Stages(orc.mbinfo(), orc.levels(), orc.mvq(), orc.mbaux(), [orc.recon_pre(p) for p in range(3)], [orc.recon(p) for p in range(3)])


@functools.lru_cache(maxsize=None)
def expected(w, h, prof=66):
    """the oracle's pictures of the sequence at (w, h): access unit, picture type, QP and every stage.  Computed once per
    process, shared by the tests that need it; nobody changes it"""
    from oracle_lib import OracleEncoder
    orc = OracleEncoder(w, h, qp=QPS[0], gop=len(QPS), profile_idc=prof)
    out = []
    for i, f in enumerate(frames(w, h)):
        if i:
            orc.set_qp(QPS[i])
        au, idr = orc.encode(f)
        out.append(Pic(au, idr, QPS[i], stages_of(orc)))
    orc.close()
    return tuple(out)


@functools.lru_cache(maxsize=None)
def expected_batch(w, h, prof=66):
    """the oracle's serial stream of the lockstep case: call 0 item 0, item 1, .. then call 1 .. (idr_pic_id runs on, as the
    engine's does).  [call][item] = (list of access units, stages of the item's last picture)"""
    from oracle_lib import OracleEncoder
    orc = OracleEncoder(w, h, qp=BATCH_QPS[0], gop=BATCH_GOP, profile_idc=prof)
    out = []
    for call, qp in enumerate(BATCH_QPS):
        orc.set_qp(qp)
        items = []
        for g in range(BATCH_G):
            aus = []
            for i, f in enumerate(batch_frames(w, h, call, g)):
                au, idr = orc.encode(f)
                assert idr == (i == 0), "closed GOPs"
                aus.append(au)
            items.append((aus, stages_of(orc)))
        out.append(items)
    orc.close()
    return out


def compare(got, want, tag):
    """got: an object with debug_read (capi.Encoder, capi.Stream) that has just coded the picture; want: the oracle's Stages"""
    from media_amd import capi
    mb, omb = got.debug_read(capi.DBG_MBINFO), want.mbinfo
    for f in ("mvx", "mvy", "type", "i16_mode", "chroma_mode", "cbp", "tc"):
        assert np.array_equal(mb[f], omb[f]), "%s: mbinfo.%s" % (tag, f)
    inter = np.isin(omb["type"], INTER)
    if inter.any():
        assert np.array_equal(got.debug_read(capi.DBG_MVQ)[inter], want.mvq[inter]), tag + ": quadrant vectors"
    i4 = omb["type"] == 4
    if i4.any():
        assert np.array_equal(got.debug_read(capi.DBG_MBAUX)[i4], want.mbaux[i4]), tag + ": Intra4x4 modes"
    read = read_mask(omb)
    assert np.array_equal(np.where(read, got.debug_read(capi.DBG_LEVELS), 0), np.where(read, want.levels, 0)), tag + ": levels where read"
    for p in range(3):
        assert np.array_equal(got.debug_read(capi.DBG_PRE_Y + p), want.pre[p]), "%s: pre-filter plane %d" % (tag, p)
        assert np.array_equal(got.debug_read(capi.DBG_RECON_Y + p), want.recon[p]), "%s: final plane %d" % (tag, p)


def coverage(pics):
    """what the sequence holds, from the oracle's mbinfo and levels alone.  A part is STALE in picture i when an inter macroblock
    leaves it uncoded although picture i - 1 left non-zero levels there that were read (so the GPU wrote them too)"""
    cov = {"luma_patterns": set(), "chroma_cbp": set(), "types": set(), "stale_quadrants": 0, "stale_chroma_ac": 0}
    prev = None
    for pic in pics:
        mb, lv = pic.stages.mbinfo, pic.stages.levels
        inter = np.isin(mb["type"], INTER)
        coded = inter & (mb["type"] != 2)
        cbp = mb["cbp"].astype(np.int32)
        cov["types"] |= set(int(t) for t in mb["type"])
        cov["luma_patterns"] |= set(int(c) & 15 for c in cbp[coded])
        cov["chroma_cbp"] |= set(int(c) >> 4 for c in cbp[coded])
        had = np.where(read_mask(mb), lv, 0) != 0
        if prev is not None:
            for q in range(4):
                cov["stale_quadrants"] += int((inter & ((cbp >> q) & 1 == 0) & prev[:, 16 + 64 * q: 16 + 64 * (q + 1)].any(axis=1)).sum())
            cov["stale_chroma_ac"] += int((inter & ((cbp >> 4) != 2) & prev[:, 280:408].any(axis=1)).sum())
        prev = had
    return cov
