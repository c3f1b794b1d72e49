"""The chain of a P step of the encoder's own lockstep batches between the motion search and the loop filter
(media_amd/csrc/engine.h submit_step): the intra pass is ONE launch (k_intra.h k_pintra_rows<false, false, true>) whose row waves
choose Intra4x4-or-16x16 and the block modes of a marked macroblock themselves, just before they code it, and ask a flag of the
whole step before they look at any picture's own; the motion-search lock goes back with the first wave of k_tq / k_tq8
(k_tq.h tq_turn_release) instead of a launch of its own.

Every access unit of every item equals the oracle's, and so do the planes before and after the loop filter - of every picture with
one picture in flight, of item 0's last picture in a lockstep batch (tests/pstep_chain.py gives item 0 another kind in every call;
a wrong reconstruction of an earlier picture changes the bytes of the next).  Shapes: one macroblock, two beside each other, one
column of three rows, 3 x 5 and 11 x 9 macroblocks; batches of 8 (the pair form of the filter) and 2 (the row form), a batch-1
encoder, three slices, and two engines of 16 items side by side on two threads (the batch size from which the searches take turns).

The CPU part states of the oracle alone that the cases hold what they are for.

Mutations of the committed kernels in scratch builds (profiles/pstep_chain_headline.json): the step flag never set (k_me's store
left out) fails all 24 GPU tests, first on the bytes of the items with a cut; the modes chosen by the row wave but not stored for
the entropy coder fails all 24; the lock never given back leaves the outputs right and shows in the measurement build's counter."""
import threading
import numpy as np
import pytest
from media_amd import capi
import pstep_chain as pc

gpu = pytest.mark.gpu
SIZE_IDS = ["%dx%d" % s for s in pc.SIZES]
CALLS = len(pc.PATTERN)          # item 0 takes every kind once
BIG, ODD = (176, 144), (48, 80)
MIX = ("cut2", "cut3")           # a step of pictures with and without marked macroblocks, the other way round in the next


def _p_pictures(w, h, G, calls, **kw):
    for call, per_item in enumerate(pc.expected(w, h, G, calls, **kw)):
        for g, pics in enumerate(per_item):
            for i, p in enumerate(pics[1:], 1):
                yield pc.kinds_of(call, G, kw.get("pattern", pc.PATTERN))[g][0], call, g, i, p


# ---- conditions, stated of the oracle alone (no GPU needed)

def test_oracle_p_pictures_hold_both_intra_types_and_none():
    for w, h in (ODD, BIG):
        seen = {"i4": 0, "i16": 0}
        for kind, call, g, i, p in _p_pictures(w, h, 8, CALLS):
            seen["i4"] += int((p["types"] == pc.MB_I4).sum())
            seen["i16"] += int((p["types"] == pc.MB_I16).sum())
            if kind in ("s1", "s2", "split"):
                assert pc.intra_mbs(p) == 0, "%dx%d %s call %d picture %d: an intra macroblock" % (w, h, kind, call, i)
        assert seen["i4"] and seen["i16"], seen
        # the batch of 2: steps none of whose pictures has an intra macroblock (one load per wave), and steps with some
        ex2 = pc.expected(w, h, 2, CALLS)
        per_step = [sum(pc.intra_mbs(ex2[c][g][i]) for g in range(2)) for c in range(CALLS) for i in range(1, pc.GOP)]
        assert 0 in per_step and any(per_step), per_step


def test_oracle_every_size_has_a_p_picture_with_an_intra_macroblock():
    for w, h in pc.SIZES:
        for G in (8, 2, 1):
            assert any(pc.intra_mbs(p) for _, _, _, _, p in _p_pictures(w, h, G, CALLS)), (w, h, G)


def test_oracle_mixed_steps_and_their_reverse():
    """step 2 holds pictures with intra macroblocks (cut2 items) beside pictures without (cut3 items: the step's flag is up, theirs is
    not); in step 3 pictures that had some have none and the other way round - in a batch of 8 and in a batch of 2"""
    for w, h in (ODD, BIG):
        for G in (8, 2):
            ex = pc.expected(w, h, G, 2, pattern=MIX)
            n = [(pc.intra_mbs(ex[c][g][2]), pc.intra_mbs(ex[c][g][3])) for c in range(2) for g in range(G)]
            steps = [n[c * G:(c + 1) * G] for c in range(2)]
            assert any(any(a > 0 and b == 0 for a, b in s) and any(a == 0 and b > 0 for a, b in s) for s in steps), (w, h, G, steps)


def test_oracle_a_still_picture_is_all_skip():
    for kind, call, g, i, p in _p_pictures(BIG[0], BIG[1], 8, CALLS):
        if kind == "s2" and i >= 2:   # (picture 1 still codes the IDR picture's quantisation error here and there)
            assert (p["types"] == 2).all(), (call, g, i)


# ---- the GPU cases

@gpu
@pytest.mark.parametrize("G", [8, 2])
@pytest.mark.parametrize("size", pc.SIZES, ids=SIZE_IDS)
def test_lockstep_batch(size, G):
    """8: the pair form of the filter behind the chain, 2: the row form.  An item codes a still picture (s2) in the call after one
    with motion, on the same arrays"""
    pc.run_batch(size[0], size[1], G, CALLS)


@gpu
@pytest.mark.parametrize("size", pc.SIZES, ids=SIZE_IDS)
def test_one_picture_in_flight(size):
    """a batch-1 encoder, GOP after GOP of every kind; the planes before and after the filter compared after every picture"""
    w, h = size
    want = pc.expected(w, h, 1, CALLS)
    enc = capi.Encoder(w, h, qp=pc.QP, gop=pc.GOP)
    try:
        enc.keep_pre()
        for call in range(CALLS):
            kind = pc.kinds_of(call, 1)[0][0]
            for i, (f, o) in enumerate(zip(pc.frames(w, h, call, 1)[0], want[call][0])):
                assert enc.encode(f)[0] == o["au"], "%s picture %d: access unit" % (kind, i)
                for p in range(3):
                    pc.same(enc.debug_read(capi.DBG_PRE_Y + p), o["pre"][p], "%s picture %d plane %d before the filter" % (kind, i, p))
                    pc.same(enc.debug_read(capi.DBG_RECON_Y + p), o["post"][p], "%s picture %d plane %d" % (kind, i, p))
    finally:
        enc.close()


@gpu
@pytest.mark.parametrize("G", [8, 2])
@pytest.mark.parametrize("size", [ODD, BIG], ids=["48x80", "176x144"])
def test_three_slices(size, G):
    """slices of two rows (the last of 48x80: one): a slice's first row has no macroblock above, for the intra pass and the filter"""
    pc.run_batch(size[0], size[1], G, 4, slices=3)


@gpu
@pytest.mark.parametrize("G", [8, 2])
@pytest.mark.parametrize("size", [ODD, BIG], ids=["48x80", "176x144"])
def test_steps_that_mix_pictures_with_and_without_intra_macroblocks(size, G):
    """step 2: the step's flag is up, every other picture's own flag is down; step 3: the other half"""
    pc.run_batch(size[0], size[1], G, 2, pattern=MIX)


@gpu
def test_two_engines_of_16_items_side_by_side():
    """two engines whose motion searches take turns at the GPU's lock, one thread each, two calls: both code what the oracle codes.
    (A lock that is not given back lets the other engine's acquire run into its time-out: the output is still right, so the
    time-outs are counted by a measurement build - media_amd/csrc/Makefile, TURN_AB_COUNT - and tools/turn_timeouts.py.)"""
    w, h = ODD
    pc.expected(w, h, 16, 2)   # (once, before the threads ask for it)
    encs = [capi.Encoder(w, h, qp=pc.QP, gop=pc.GOP, batch=16) for _ in range(2)]
    errs = [None, None]
    go = threading.Barrier(2)

    def work(k):
        try:
            go.wait()
            pc.run_batch(w, h, 16, 2, enc=encs[k])
        except BaseException as e:   # noqa: BLE001 (handed to the test's thread)
            errs[k] = e

    try:
        ths = [threading.Thread(target=work, args=(k,)) for k in range(2)]
        for t in ths:
            t.start()
        for t in ths:
            t.join()
    finally:
        for e in encs:
            e.close()
    for k, e in enumerate(errs):
        if e is not None:
            raise AssertionError("engine %d: %s" % (k, e)) from e
