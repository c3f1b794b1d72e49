"""The device entropy coder on syntax its own decision kernels never choose.

Every picture of tests/test_entropy_random_oracle.py's case list (random macroblock types, modes, vectors, patterns and
levels - that file shows what they cover) goes into mi355x_h264_debug_code_syntax as the arrays the decision kernels would
have left, and the access unit that k_bs, k_mvpred, k_skip_scan, k_cavlc, k_bit_scan, k_pack and the host's finishing make
of them must be the oracle's, byte for byte.  Then lockstep batches, and once the refusal of a slice that outgrows its
payload share (MI355X_H264_E_OVERFLOW)."""
import numpy as np
import pytest

import annexb
from media_amd import capi
from test_entropy_random_oracle import BATCH_CASES, CASES, REFUSAL_CASE, batch_pictures, case_id, oracle_for, refusal_sequence, slice_geometry

pytestmark = pytest.mark.gpu


def encoder_for(c, batch=1):
    return capi.Encoder(c.width, c.height, qp=c.qp, gop=c.gop, profile_idc=c.profile, disable_deblock=c.disable_deblock,
                        slices=c.slices, refs=c.refs, batch=batch)


def arrays(o):
    return o.mbinfo(), o.levels(), o.mvq(), o.mbaux(), o.source_i420()


def _rbsp(payload):
    out, zeros = bytearray(), 0
    for b in payload:
        if zeros >= 2 and b == 3:
            zeros = 0
            continue
        out.append(b)
        zeros = zeros + 1 if b == 0 else 0
    return bytes(out)


def locate(got, want, o, c):
    """the first differing byte of two access units and the macroblock of the oracle's picture it falls in"""
    n = next((i for i, (a, b) in enumerate(zip(got, want)) if a != b), min(len(got), len(want)))
    text = "first difference at byte %d of %d (oracle: %d bytes)" % (n, len(got), len(want))
    mbw, rows = slice_geometry(c)
    pos = o.mb_bitpos()
    sl = 0
    for (_, tg, pg), (_, tw, pw) in zip(annexb.split_nal_units(got), annexb.split_nal_units(want)):
        if tw not in (1, 5):
            if pg != pw:
                return text + ": in a parameter set"
            continue
        if pg != pw:
            rg, rw = _rbsp(pg), _rbsp(pw)
            k = next((i for i, (a, b) in enumerate(zip(rg, rw)) if a != b), min(len(rg), len(rw)))
            first = sum(rows[:sl]) * mbw
            mbs = [first + i for i in range(rows[sl] * mbw) if pos[first + i] <= 8 * k + 7]
            mb = mbs[-1] if mbs else first
            return text + ": slice %d, byte %d of its RBSP, macroblock %d (x %d, y %d, type %d), which starts at bit %d" % (
                sl, k, mb, mb % mbw, mb // mbw, int(o.mbinfo()["type"][mb]), int(pos[mb]))
        sl += 1
    return text


def check_mbinfo(enc, o, tag):
    got, want = enc.debug_read(capi.DBG_MBINFO), o.mbinfo()
    for f in ("type", "cbp", "tc"):
        assert np.array_equal(got[f], want[f]), "%s: MbInfo.%s read back differs at macroblocks %s" % (
            tag, f, np.flatnonzero((got[f] != want[f]).reshape(len(want), -1).any(axis=1))[:8])


@pytest.mark.parametrize("c", CASES, ids=case_id)
def test_injected_syntax_codes_to_the_oracles_bytes(c):
    enc, o = encoder_for(c), oracle_for(c)
    try:
        for k in range(c.pictures):
            want, idr, _ = o.random_picture(c.seed + k, features=c.features)
            rc, (got,), ft = enc.code_syntax(*arrays(o))
            tag = "%s picture %d" % (case_id(c), k)
            assert rc == 0, "%s: rc %d (%s)" % (tag, rc, enc.last_error())
            assert ft == (capi.FRAME_IDR if idr else capi.FRAME_P), tag
            assert got == want, "%s: %s" % (tag, locate(got, want, o, c))
            check_mbinfo(enc, o, tag)
    finally:
        enc.close()
        o.close()


@pytest.mark.parametrize("c,batch", BATCH_CASES, ids=lambda v: case_id(v) if isinstance(v, tuple) else "G%d" % v)
def test_lockstep_batches_of_different_pictures(c, batch):
    """every item its own seeds: the items' pictures differ in length and in whether they hold an I_PCM macroblock
    (test_entropy_random_oracle.test_batch_items_differ_in_length_and_in_ipcm_presence)"""
    enc = encoder_for(c, batch)
    try:
        for k, (oracles, want, idr) in enumerate(batch_pictures(c, batch)):
            rc, got, ft = enc.code_syntax(*_stack(oracles))
            assert rc == 0, "picture %d: rc %d (%s)" % (k, rc, enc.last_error())
            assert ft == (capi.FRAME_IDR if idr else capi.FRAME_P)
            for g, o in enumerate(oracles):
                assert got[g] == want[g], "picture %d item %d: %s" % (k, g, locate(got[g], want[g], o, c))
            check_mbinfo(enc, oracles[0], "picture %d item 0" % k)
    finally:
        enc.close()


def _stack(oracles):
    """the items' arrays one after the other, as mi355x_h264_debug_code_syntax takes a batch"""
    return [np.concatenate([np.ascontiguousarray(a).reshape(-1).view(np.uint8) for a in x]) for x in zip(*[arrays(o) for o in oracles])]


@pytest.mark.parametrize("batch", [1, 2])
def test_first_slice_over_its_share_is_refused_and_nothing_else_is_touched(batch):
    """Item 0's first slice codes to more than its payload share (test_entropy_random_oracle proves that of this very sequence):
    the call returns MI355X_H264_E_OVERFLOW, a second item is delivered untouched, and the next picture - which fits - is an IDR
    equal to the oracle's after a forced IDR, all three slices of it: nothing was left behind in the shares that follow the first"""
    c = REFUSAL_CASE
    enc = encoder_for(c, batch)
    try:
        for step, oracles, want in refusal_sequence(batch):
            rc, got, ft = enc.code_syntax(*_stack(oracles))
            if step == "refused":
                assert rc == capi.E_OVERFLOW, "rc %d (%s)" % (rc, enc.last_error())
                assert got[0] is None
            else:
                assert rc == 0, "%s: rc %d (%s)" % (step, rc, enc.last_error())
                assert ft == capi.FRAME_IDR   # "after": because of the refusal, not of the GOP length (5)
            for g in range(1 if step == "refused" else 0, batch):
                assert got[g] == want[g], "%s, item %d: %s" % (step, g, locate(got[g], want[g], oracles[g], c))
    finally:
        enc.close()


def test_a_real_picture_after_an_injected_one_is_an_idr():
    c = CASES[12]
    enc, o, ref = encoder_for(c), oracle_for(c), oracle_for(c)
    try:
        for k in range(2):
            want, _, _ = o.random_picture(c.seed + k, features=c.features)
            rc, (got,), ft = enc.code_syntax(*arrays(o))
            assert rc == 0 and got == want
        assert ft == capi.FRAME_P
        rng = np.random.default_rng(5)
        pic = rng.integers(0, 256, c.width * c.height * 3 // 2, dtype=np.uint8)
        ref.random_picture(1, features=0)   # (one IDR done: the next idr_pic_id is 1, as the encoder's)
        want, idr = ref.encode(pic, force_idr=True)
        got, ft = enc.encode(pic)
        assert ft == capi.FRAME_IDR and idr
        assert got == want
    finally:
        enc.close()
        o.close()
        ref.close()
