"""The device entropy coder at the shapes where up-front loads can go wrong.

k_cavlc's code_slot requests what a slot needs - the word of the macroblock's MbInfo, two neighbour bytes at clamped
addresses, on slot 0 the modes of three macroblocks - before it looks at any of it, then its aligned block of levels where
type and pattern leave it one.  The scan
kernels split a picture over 256 threads.  The case list of tests/test_entropy_random_oracle.py has no picture with a half-dead last wave, none with more
macroblocks than the scan kernels have threads and no slice that starts at an odd macroblock below another slice; the
cases here do.  Every access unit must be the oracle's, byte for byte: injected random syntax
(mi355x_h264_debug_code_syntax) first, then a real sequence whose skip runs cover a whole slice, end at the last and at the
first macroblock and cross the share of one scan thread.

The CPU-only tests (no gpu mark) prove on the oracle alone that these inputs hold what the GPU tests rely on."""
import numpy as np
import pytest

from oracle_lib import OracleEncoder
from test_entropy_random_oracle import (BIG, DENSE, PCM, SHAPED, SLICE_GUARD_BITS, SLICE_TAIL_BITS, Case, batch_pictures, case_id, oracle_for,
                                        pictures, share_bits, slice_geometry)

MB_PSKIP, MB_IPCM, MB_I4 = 2, 3, 4   # media_amd/csrc/dev_common.h


def _c(i, w, h, profile, slices, qp, feat):
    return Case(w, h, profile, 0, slices, 0, qp, SHAPED | feat, 5, 8, 9100 + 100 * i)


# 48x48: 9 macroblocks, the last wave's upper half is dead.  272x256: 272 macroblocks on 256 scan threads (two per thread,
# a ragged last share, empty threads).  48x80 in 2 slices: slice 1 starts at macroblock 9 - an odd start, and the
# macroblocks above its first row belong to the other slice: what the clamped neighbour loads bring must not be used.  272x256 in 3 slices: starts at 0, 102, 204.
# Levels of 128 and more (BIG) go with QP 10 only, as in the case list this one extends.
CASES = [_c(i, *t) for i, t in enumerate([
    (48, 48, 66, 0, 26, PCM | DENSE), (48, 48, 100, 0, 10, PCM | BIG),
    (272, 256, 100, 0, 26, PCM | DENSE), (272, 256, 66, 0, 10, PCM | BIG),
    (48, 80, 66, 2, 26, PCM | DENSE), (48, 80, 100, 2, 10, PCM | BIG),
    (272, 256, 66, 3, 26, PCM | DENSE), (272, 256, 100, 3, 10, PCM | BIG | DENSE),
])]
BATCH_CASE, BATCH = CASES[6], 3

# the real sequence: 272x256, a flat picture (IDR), the same again, then a 16x16 patch of noise in every picture
SEQ_W, SEQ_H, SEQ_MBW = 272, 256, 17
SEQ_PATCHES = [None, None, 271, 0, 32]   # macroblock that gets its patch in picture k


def sequence_pictures():
    """the five pictures.  A patch of noise does not reconstruct exactly, so a picture that kept the SOURCE of an earlier patch
    would code that macroblock again: every picture is the oracle's reconstruction of the one before it plus its own patch"""
    if not _SEQ:
        rng = np.random.default_rng(77)
        o = sequence_oracle()
        planes = [np.full((SEQ_H >> (p > 0), SEQ_W >> (p > 0)), 128, np.uint8) for p in range(3)]
        for mb in SEQ_PATCHES:
            if mb is not None:
                my, mx = divmod(mb, SEQ_MBW)
                planes[0][16 * my: 16 * my + 16, 16 * mx: 16 * mx + 16] = rng.integers(0, 256, (16, 16), dtype=np.uint8)
            _SEQ.append(np.concatenate([p.ravel() for p in planes]))
            o.encode(_SEQ[-1])
            planes = [o.recon(p)[: SEQ_H >> (p > 0), : SEQ_W >> (p > 0)].copy() for p in range(3)]
        o.close()
    return _SEQ


_SEQ = []


def sequence_oracle():
    return OracleEncoder(SEQ_W, SEQ_H, qp=26, gop=30)


# ---- what the inputs hold: the oracle alone ----

def _i4_between_other_types(o, c):
    """I_NxN macroblocks whose left and upper macroblocks exist (the upper one in the same slice) and are both not I_NxN"""
    mbw, rows = slice_geometry(c)
    t = o.mbinfo()["type"].reshape(-1, mbw)
    first_rows = set(np.cumsum([0] + rows[:-1]).tolist())
    n = 0
    for my in range(t.shape[0]):
        for mx in range(1, mbw):
            if my not in first_rows and t[my, mx] == MB_I4 and t[my, mx - 1] != MB_I4 and t[my - 1, mx] != MB_I4:
                n += 1
    return n


def test_inputs_hold_what_the_gpu_tests_rely_on():
    assert {(c.width, c.height, c.slices) for c in CASES} == {(48, 48, 0), (272, 256, 0), (48, 80, 2), (272, 256, 3)}
    assert slice_geometry(CASES[4]) == (3, [3, 2]) and slice_geometry(CASES[6]) == (17, [6, 6, 4])   # slice 1 of 48x80 starts at macroblock 9
    long_res = long_hdr = pcm = i4 = tc16 = 0
    for c in CASES:
        mbw, rows = slice_geometry(c)
        idrs = 0
        for o, au, idr in pictures(c):
            for b, r in zip(o.slice_bits(), rows):   # the injected path has no I_PCM fallback: every slice inside its share
                assert b <= share_bits(mbw, r) - (SLICE_GUARD_BITS + SLICE_TAIL_BITS), (case_id(c), o.slice_bits(), rows)
            idrs += idr
            pcm += int((o.mbinfo()["type"] == MB_IPCM).sum())
            i4 += _i4_between_other_types(o, c)
        assert 2 <= idrs < c.pictures, case_id(c)   # IDR and P pictures
        h = o.hits()
        long_res += int(h["long_residual_slots"])
        long_hdr += int(h["long_header_slots"])
        tc16 += int(h["coeff_token"][:, 16, :].sum())
        o.close()
    print("residual slots over 64 bits %d, header slots over 64 bits %d, I_PCM %d, I_NxN between other types %d, coeff_token with tc 16: %d"
          % (long_res, long_hdr, pcm, i4, tc16))
    assert long_res >= 1 and long_hdr >= 1 and pcm >= 1 and i4 >= 1 and tc16 >= 1


def test_batch_items_differ():
    for oracles, aus, _ in batch_pictures(BATCH_CASE, BATCH):
        assert len(set(aus)) == BATCH


def test_sequence_codes_nothing_then_one_macroblock_per_picture():
    o = sequence_oracle()
    try:
        for k, pic in enumerate(sequence_pictures()):
            _, idr = o.encode(pic)
            assert idr == (k == 0)
            coded = np.flatnonzero(o.mbinfo()["type"] != MB_PSKIP)
            if k == 1:
                assert coded.size == 0   # the whole slice is the closing skip run
            elif k >= 2:
                assert coded.tolist() == [SEQ_PATCHES[k]], (k, coded)
    finally:
        o.close()


# ---- the device ----

gpu = pytest.mark.gpu


def _gpu():
    from media_amd import capi
    import test_gpu_entropy_random as ger
    return capi, ger


@gpu
@pytest.mark.parametrize("c", CASES, ids=case_id)
def test_injected_syntax_codes_to_the_oracles_bytes(c):
    capi, ger = _gpu()
    enc, o = ger.encoder_for(c), oracle_for(c)
    try:
        for k in range(c.pictures):
            want, idr, _ = o.random_picture(c.seed + k, features=c.features)
            rc, (got,), ft = enc.code_syntax(*ger.arrays(o))
            tag = "%s picture %d" % (case_id(c), k)
            assert rc == 0, "%s: rc %d (%s)" % (tag, rc, enc.last_error())
            assert ft == (capi.FRAME_IDR if idr else capi.FRAME_P), tag
            assert got == want, "%s: %s" % (tag, ger.locate(got, want, o, c))
    finally:
        enc.close()
        o.close()


@gpu
def test_three_slices_in_a_lockstep_batch_of_three():
    capi, ger = _gpu()
    c = BATCH_CASE
    enc = ger.encoder_for(c, BATCH)
    try:
        for k, (oracles, want, idr) in enumerate(batch_pictures(c, BATCH)):
            rc, got, ft = enc.code_syntax(*ger._stack(oracles))
            assert rc == 0, "picture %d: rc %d (%s)" % (k, rc, enc.last_error())
            assert ft == (capi.FRAME_IDR if idr else capi.FRAME_P)
            for g, o in enumerate(oracles):
                assert got[g] == want[g], "picture %d item %d: %s" % (k, g, ger.locate(got[g], want[g], o, c))
    finally:
        enc.close()


@gpu
def test_skip_runs_of_a_real_sequence():
    """all P_Skip; one coded macroblock at the end, at the start, and where a scan thread's share begins
    (test_sequence_codes_nothing_then_one_macroblock_per_picture)"""
    capi, _ = _gpu()
    enc, o = capi.Encoder(SEQ_W, SEQ_H, qp=26, gop=30), sequence_oracle()
    try:
        for k, pic in enumerate(sequence_pictures()):
            want, idr = o.encode(pic)
            got, ft = enc.encode(pic)
            assert ft == (capi.FRAME_IDR if idr else capi.FRAME_P), k
            assert got == want, "picture %d: %d bytes, oracle %d" % (k, len(got), len(want))
    finally:
        enc.close()
        o.close()
