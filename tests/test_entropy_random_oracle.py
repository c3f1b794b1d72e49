"""Random syntax for the device entropy coder (k_mvpred, k_skip_scan, k_cavlc, k_bit_scan, k_pack): the case list, and the
proof - on the oracle alone, no GPU - that those inputs are worth running.

tests/test_gpu_entropy_random.py hands every picture of CASES to mi355x_h264_debug_code_syntax and asks for the oracle's
bytes.  Here the oracle's own hit counters (h264o_hits) say what those pictures exercise: every macroblock type, every
Intra4x4 mode at every block, every coded_block_pattern, every legal entry of Tables 9-5, 9-7, 9-8, 9-9 and 9-10, every
suffixLength with both escape prefixes, slots longer than 64 bits, long vectors differences and skip runs.  Nothing is
excused: an entry that is not reached is a reason to extend the generator (oracle/h264_enc.c, features 2048 / 4096).
The injected entropy path has no I_PCM fallback, so every slice must also stay inside its payload share."""
import collections

import numpy as np
import pytest

import annexb
from oracle_lib import OracleDecoder, OracleEncoder

SHAPED, DENSE, PCM, BIG = OracleEncoder.RAND_ENCODER_SHAPED, OracleEncoder.RAND_DENSE, OracleEncoder.RAND_PCM, OracleEncoder.RAND_BIG_LEVELS
SLICE_GUARD_BITS, SLICE_TAIL_BITS = 1024, 64   # media_amd/csrc/k_cavlc.h

Case = collections.namedtuple("Case", "width height profile refs slices disable_deblock qp features gop pictures seed")


def _c(i, w, h, profile, refs, slices, nofilter, qp, feat):
    return Case(w, h, profile, refs, slices, nofilter, qp, SHAPED | feat, 5, 8, 7000 + 100 * i)


# every size, profile, refs, slices, filter switch and QP of the issue's table, each feature set with each profile; I_PCM is
# left out of the one-macroblock picture (an I_PCM macroblock alone is more than that picture's payload share) and levels of
# 128 and more (BIG) go with QP <= 14 only
CASES = [_c(i, *t) for i, t in enumerate([
    (16, 16, 66, 0, 0, 0, 26, 0), (16, 16, 100, 2, 0, 1, 10, DENSE), (16, 16, 77, 3, 0, 0, 51, 0),
    (256, 16, 66, 0, 0, 0, 14, PCM | BIG), (256, 16, 100, 3, 0, 1, 26, PCM | DENSE), (256, 16, 77, 2, 0, 0, 10, DENSE),
    (16, 64, 66, 2, 2, 0, 26, PCM), (16, 64, 100, 0, 0, 0, 14, DENSE), (16, 64, 77, 3, 2, 1, 51, 0),
    (50, 34, 66, 0, 0, 0, 26, PCM | DENSE), (50, 34, 100, 2, 0, 0, 10, PCM | BIG), (50, 34, 77, 3, 0, 1, 14, DENSE),
    (178, 98, 66, 3, 2, 0, 26, PCM), (178, 98, 100, 0, 3, 0, 10, PCM | DENSE), (178, 98, 77, 2, 0, 1, 51, PCM),
    (178, 98, 100, 3, 2, 0, 14, PCM | BIG),
    (352, 288, 66, 0, 0, 0, 26, PCM | DENSE), (352, 288, 100, 3, 4, 0, 10, DENSE), (352, 288, 77, 2, 3, 1, 14, PCM | BIG),
    (352, 288, 66, 2, 2, 0, 51, PCM), (352, 288, 100, 0, 4, 0, 26, PCM | DENSE),
    (640, 368, 66, 0, 0, 0, 26, PCM), (640, 368, 100, 3, 4, 0, 14, PCM | DENSE), (640, 368, 77, 2, 3, 1, 10, DENSE),
    (640, 368, 100, 0, 2, 0, 51, 0), (640, 368, 66, 3, 0, 1, 10, PCM | BIG),
    (352, 288, 77, 0, 0, 0, 26, 0), (178, 98, 66, 2, 3, 1, 26, DENSE), (50, 34, 100, 0, 0, 0, 51, PCM), (256, 16, 66, 0, 0, 0, 51, PCM),
])]
BATCH_CASES = [(CASES[13], 2), (CASES[9], 3), (CASES[18], 8)]   # lockstep batches of the GPU test: (case, batch)
# the refusal path: three slices, the first of every picture of seed REFUSAL_SEED outgrows its share (feature 8192)
REFUSAL_CASE = Case(352, 288, 66, 0, 3, 0, 10, SHAPED | PCM | OracleEncoder.RAND_SATURATE_FIRST_SLICE, 5, 1, 4242)


def case_id(c):
    return "%dx%d-p%d-r%d-s%d-d%d-qp%d-f%d" % c[:8]


def oracle_for(c):
    return OracleEncoder(c.width, c.height, qp=c.qp, gop=c.gop, profile_idc=c.profile, disable_deblock=c.disable_deblock,
                         slices=c.slices, refs=c.refs)


def slice_geometry(c):
    """(macroblocks per row, [macroblock rows of every slice]) as mi355x_h264_create and the oracle lay a picture out"""
    mbw, mbh = (c.width + 15) // 16, (c.height + 15) // 16
    n = min(max(c.slices, 1), max(1, mbh // 2))
    rows = (mbh + n - 1) // n
    return mbw, [min(rows, mbh - r) for r in range(0, mbh, rows)]


def share_bits(mbw, rows):
    """payload share of a slice of `rows` macroblock rows: twice its luma bytes"""
    return 8 * 2 * 256 * mbw * rows


def pictures(c, seed_offset=0):
    """the pictures of a case: (oracle, access unit, is_idr) one after the other; the oracle holds the picture's arrays"""
    o = oracle_for(c)
    for k in range(c.pictures):
        au, idr, _ = o.random_picture(c.seed + seed_offset + k, features=c.features)
        yield o, au, idr


def batch_pictures(c, batch):
    """the steps of a lockstep batch of a case, every item with seeds of its own: yields (oracles, access units, is_idr)"""
    oracles = [oracle_for(c) for _ in range(batch)]
    for g, o in enumerate(oracles):   # consecutive idr_pic_ids, as a lockstep batch numbers its items' IDR pictures
        o.set_idr_id(g, batch)
    for k in range(c.pictures):
        res = [o.random_picture(c.seed + 1000 * (g + 1) + k, features=c.features) for g, o in enumerate(oracles)]
        yield oracles, [r[0] for r in res], res[0][1]


def refusal_sequence(batch):
    """the three steps of the refusal test, for `batch` lockstep items: a picture that fits (IDR), the picture whose FIRST slice
    outgrows its share in item 0 only (a P picture), a picture that fits after a forced IDR.  Yields (step, oracles, access units)
    with the oracles holding the step's arrays"""
    c = REFUSAL_CASE
    fits = c.features & ~OracleEncoder.RAND_SATURATE_FIRST_SLICE
    oracles = [oracle_for(c) for _ in range(batch)]
    for g, o in enumerate(oracles):   # consecutive idr_pic_ids, as a lockstep batch numbers its items' IDR pictures
        o.set_idr_id(g, batch)
    yield "before", oracles, [o.random_picture(c.seed - 1 - g, features=fits)[0] for g, o in enumerate(oracles)]
    yield "refused", oracles, [o.random_picture(c.seed + g, features=c.features if g == 0 else fits)[0] for g, o in enumerate(oracles)]
    yield "after", oracles, [o.random_picture(c.seed + 50 + g, force_idr=True, features=fits)[0] for g, o in enumerate(oracles)]


def has_emulation_prevention(au):
    return any(b"\x00\x00\x03" in payload for _, t, payload in annexb.split_nal_units(au) if t in (1, 5))


@pytest.fixture(scope="module")
def run():
    """every picture of every case, once: decoded, its slices measured, the hit counters summed"""
    total, per_case, epb, wide_skip = None, {}, 0, 0
    for c in CASES:
        dec = OracleDecoder()
        mbw, rows = slice_geometry(c)
        idrs, worst = 0, 0.0
        for o, au, idr in pictures(c):
            assert dec.decode(au) == 1, case_id(c)
            assert dec.max_level_prefix <= 15, case_id(c)
            bits = o.slice_bits()
            assert len(bits) == len(rows), (case_id(c), bits)
            for b, r in zip(bits, rows):   # a condition on the inputs: the injected path has no I_PCM fallback
                assert b <= share_bits(mbw, r) - (SLICE_GUARD_BITS + SLICE_TAIL_BITS), (case_id(c), bits, rows)
                worst = max(worst, b / share_bits(mbw, r))
            idrs += idr
            epb += has_emulation_prevention(au)
        h = o.hits()
        dec.close()
        assert idrs >= 2 and idrs < c.pictures, case_id(c)   # the GOP length crosses an IDR
        if mbw >= 4:
            wide_skip += int(h["skip_runs_over_a_row"])
        per_case[case_id(c)] = (c.pictures, worst)
        if total is None:
            total = h
        else:
            total = {k: (np.maximum(total[k], v) if k in ("max_mvd", "max_skip_run") else total[k] + v) for k, v in h.items()}
    print("\npictures per case and the fullest slice (share of its payload):")
    for k, (n, wst) in per_case.items():
        print("  %-36s %d pictures, %.2f" % (k, n, wst))
    print("hit counters over all cases:")
    for k, v in total.items():
        print("  %s: sum %d, entries hit %d of %d, least non-zero %d" % (k, int(v.sum()), int((v > 0).sum()), v.size, int(v[v > 0].min()) if (v > 0).any() else 0))
    print("  access units with an emulation prevention byte: %d; skip runs over a row in pictures 4+ macroblocks wide: %d" % (epb, wide_skip))
    return total, epb, wide_skip


def test_case_list_spans_the_issue_table():
    assert 28 <= len(CASES) <= 32
    assert {(c.width, c.height) for c in CASES} == {(16, 16), (256, 16), (16, 64), (50, 34), (178, 98), (352, 288), (640, 368)}
    assert {c.profile for c in CASES} == {66, 77, 100} and {c.refs for c in CASES} == {0, 2, 3}
    assert {c.slices for c in CASES} == {0, 2, 3, 4} and {c.disable_deblock for c in CASES} == {0, 1}
    assert {c.qp for c in CASES} == {10, 14, 26, 51}
    assert {c.features for c in CASES} == {SHAPED | f for f in (0, PCM, PCM | BIG, DENSE, PCM | DENSE)}
    assert all(c.qp <= 14 for c in CASES if c.features & BIG)
    assert all(c.pictures >= 8 and c.gop < c.pictures for c in CASES)


def _missing(arr, legal):
    return [ix for ix in legal if arr[ix] == 0]


def test_macroblock_layer_coverage(run):
    h, _, _ = run
    assert (h["mb_kind"] > 0).all(), h["mb_kind"]
    assert not _missing(h["mb_type"], [(0, t) for t in range(26)] + [(1, t) for t in range(31) if t != 4])   # (4 = P_8x8ref0: code_slot has no way to write it)
    assert not _missing(h["cbp_intra"], range(48)) and not _missing(h["cbp_inter"], range(48))
    # every Intra4x4 mode at every block, modes 3 and 7 at the blocks whose above-right samples are substituted included
    assert not _missing(h["i4_mode"], [(k, m) for k in range(16) for m in range(9)])
    for k in (3, 7, 13, 15):
        assert h["i4_mode"][k][3] > 0 and h["i4_mode"][k][7] > 0


def test_residual_table_coverage(run):
    h, _, _ = run
    tokens = [(tc, t1) for tc in range(17) for t1 in range(min(tc, 3) + 1)]
    assert not _missing(h["coeff_token"], [(c,) + t for c in range(4) for t in tokens])                       # Table 9-5, 0 <= nC
    assert not _missing(h["cdc_token"], [(tc, t1) for tc in range(5) for t1 in range(min(tc, 3) + 1)])        # Table 9-5, nC = -1
    assert not _missing(h["total_zeros"], [(tc, tz) for tc in range(1, 16) for tz in range(16 - tc + 1)])     # Tables 9-7, 9-8
    assert not _missing(h["cdc_total_zeros"], [(tc, tz) for tc in range(1, 4) for tz in range(4 - tc + 1)])   # Table 9-9 (a)
    assert not _missing(h["run_before"], [(zl, r) for zl in range(1, 8) for r in range((zl if zl < 7 else 14) + 1)])   # Table 9-10
    assert (h["suffix_len"] > 0).all(), h["suffix_len"]
    assert (h["prefix14"] > 0).all() and (h["prefix15"] > 0).all(), (h["prefix14"], h["prefix15"])


def test_long_slots_vectors_and_skip_runs(run):
    h, epb, wide_skip = run
    assert h["long_residual_slots"] >= 1 and h["long_header_slots"] >= 1   # slots of more than 64 bits: coded twice by the device
    assert h["max_mvd"] >= 1024
    assert wide_skip >= 1 and h["skip_run_ends_slice"] >= 1 and h["pcm_after_skip_run"] >= 1
    assert epb >= 1


def test_refusal_input_overflows_exactly_the_first_slice():
    """what test_gpu_entropy_random's refusal test relies on: in the refused step item 0's first slice is above its share - above
    the whole allocation the encoder gives it, 4096 bytes more - by a modest margin; every other slice of every step and item is
    inside its share"""
    mbw, rows = slice_geometry(REFUSAL_CASE)
    assert len(rows) == 3
    for step, oracles, _ in refusal_sequence(2):
        for g, o in enumerate(oracles):
            bits = o.slice_bits()
            for k, (b, r) in enumerate(zip(bits, rows)):
                if (step, g, k) == ("refused", 0, 0):
                    print("refused slice: %d bits, share %d (+ %d allocated beyond it)" % (b, share_bits(mbw, r), 8 * 4096))
                    assert 8 * 4096 + share_bits(mbw, r) < b < 1.25 * share_bits(mbw, r), (b, share_bits(mbw, r))
                else:
                    assert b <= share_bits(mbw, r) - (SLICE_GUARD_BITS + SLICE_TAIL_BITS), (step, g, k, bits)


def test_batch_items_differ_in_length_and_in_ipcm_presence():
    """the lockstep batches of the GPU test are not G copies of one picture: in every step the items' access units differ in
    length, and in at least one step of at least one batch some items hold an I_PCM macroblock and some do not (the header of
    such a picture says disable_deblocking_filter_idc 1: k_bit_scan picks it per item)"""
    mixed = 0
    for c, batch in BATCH_CASES:
        for oracles, aus, _ in batch_pictures(c, batch):
            assert len(set(len(a) for a in aus)) > 1, case_id(c)
            mixed += len({bool((o.mbinfo()["type"] == 3).any()) for o in oracles}) == 2
    print("steps with and without I_PCM side by side: %d" % mixed)
    assert mixed >= 1


def test_new_feature_bits_draw_nothing_unless_set():
    """streams of the earlier feature values are what they were (test_random_stream_golden_vectors pins them byte for byte);
    here: the new bits change the picture, and a picture without them does not depend on hit counting"""
    a = OracleEncoder(64, 48, qp=26)
    b = OracleEncoder(64, 48, qp=26)
    for k in range(3):
        x, _, _ = a.random_picture(90 + k, features=PCM)
        y, _, _ = b.random_picture(90 + k, features=PCM | DENSE)
        assert x != y
    a.close()
    b.close()
