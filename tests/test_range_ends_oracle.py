"""CPU proof for tests/range_ends.py: what the range-ends streams (generator feature 131072) hold, that every one of them is a
conforming stream, and that the product's host parser reads them.  Nothing here asks the product what a stream holds: the facts
come from the writer's counters and side information and from the statistics of the oracle's independent decoder, which shares no
function or table with the writer."""
import numpy as np
import pytest

import range_ends as R
from media_amd import h264dec
from oracle_lib import OracleDecoder

EVERY = R.CASES + R.GROUP
WITH_BIT = [c for c in EVERY if c.features & R.RE]


@pytest.mark.parametrize("case", EVERY, ids=[c.name for c in EVERY])
def test_every_picture_is_decoded_and_stays_inside_the_ranges_of_the_standard(case):
    """R.stream() has the independent decoder decode every picture (it asserts that).  Then, per picture, from that decoder's own
    statistics: no scaled coefficient, transform intermediate or DC-transform value leaves -2^15 .. 2^15 - 1 (8.5.10 - 8.5.13);
    level_prefix stays <= 15 in Baseline / Main (A.2.1, A.2.2) and <= 16 in High (no larger one can come out of 8-bit video); every
    vector used lies inside A.3.1's limits for the level_idc written; and the decoder met the very levels the writer wrote.
    The 8.5 bound is asserted for every stream written with the new bit, none left out.  The group's one stream WITHOUT it is
    not held to it: the generator's older features draw a macroblock's levels for the QP in force before its mb_qp_delta, and
    the statistics added with this module measure 270 528 in its picture 1."""
    for i, p in enumerate(R.stream(case)):
        tag = "%s picture %d" % (case.name, i)
        if case.features & R.RE:
            assert p.stats["max_intermediate"] <= 32767, (tag, p.stats)
        assert p.max_level_prefix <= (16 if case.prof == 100 else 15), tag
        assert R.MV_LIMITS[0] <= p.stats["mv_x_min"] and p.stats["mv_x_max"] <= R.MV_LIMITS[1], (tag, p.stats)
        assert R.MV_LIMITS[2] <= p.stats["mv_y_min"] and p.stats["mv_y_max"] <= R.MV_LIMITS[3], (tag, p.stats)
        assert p.stats["max_level"] == int(np.abs(p.levels).max()), tag


@pytest.mark.parametrize("case", R.CASES, ids=[c.name for c in R.CASES])
def test_floors(case):
    m = R.measure(case)
    for k, floor in case.floors.items():
        assert m[k] >= floor, "%s: %s is %d, the case list says %d" % (case.name, k, m[k], floor)


def test_the_cases_together_reach_every_end():
    qps, p15, p16 = set(), np.zeros(7, np.int64), np.zeros(3, np.int64)
    kinds = {}
    slice_qp, limits, sides = np.zeros(52, np.int64), np.zeros(4, np.int64), np.zeros(4, np.int64)
    below = above = mvd_writer = 0
    edge = {v: 0 for v in (-129, -128, -127, 127, 128, 129)}
    dec_limits, dec_mvd, dec_prefix, largest = set(), 0, 0, 0
    for c in WITH_BIT:
        for p in R.stream(c):
            coded = ~np.isin(p.mb["type"], (2, 3))
            qps |= {int(q) for q in p.mbqp[coded]}
            for k, v in R.residual_kinds(p).items():
                for q in R.QP_ENDS:
                    kinds[k, q] = kinds.get((k, q), 0) + int((v & (p.mbqp == q)).sum())
            p15 += p.hits["re_prefix15_max"].astype(np.int64)
            p16 += p.hits["re_prefix16"].astype(np.int64)
            slice_qp += p.hits["re_slice_qp"].astype(np.int64)
            limits += p.hits["re_mv_limit"].astype(np.int64)
            sides += np.array([p.stats[k] for k in ("out_left", "out_right", "out_top", "out_bottom")], np.int64)
            below, above = below + int(p.hits["re_qpi_below_0"]), above + int(p.hits["re_qpi_above_51"])
            mvd_writer += int(p.hits["re_mvd_over_8192"])
            for v in edge:
                edge[v] += int((p.levels == v).sum())
            dec_limits |= {(k, p.stats[k]) for k in ("mv_x_min", "mv_x_max", "mv_y_min", "mv_y_max")}
            dec_mvd, dec_prefix = max(dec_mvd, p.stats["max_mvd"]), max(dec_prefix, p.max_level_prefix)
            largest = max(largest, p.stats["max_level"])
    assert qps == set(range(52)), "QP_Y values no coded macroblock has: %s" % sorted(set(range(52)) - qps)
    missing = [(k, q) for (k, q), n in sorted(kinds.items()) if n == 0]
    assert not missing and len(kinds) == 5 * len(R.QP_ENDS), "residual kinds without a macroblock at an end QP: %s" % missing
    assert slice_qp[0] > 0 and slice_qp[51] > 0, "SliceQP_Y 0 and 51 (pic_init_qp_minus26 + slice_qp_delta)"
    assert below > 0 and above > 0, "QP_Y + chroma_qp_index_offset below 0 and above 51"
    # the largest magnitude level_prefix 15 codes, at every suffixLength; the decoder met the largest of them
    assert (p15 > 0).all(), "suffixLengths without a level of level_prefix 15 and an all-ones suffix: %s" % p15
    assert largest >= 2528
    # level_prefix 16: in Intra16x16 DC and in chroma DC blocks, nowhere else; and the decoder read it as 16
    assert p16[0] > 0 and p16[1] > 0 and p16[2] == 0 and dec_prefix == 16, (p16, dec_prefix)
    assert all(n > 0 for n in edge.values()), edge
    assert (limits > 0).all(), limits
    assert dec_limits >= set(zip(("mv_x_min", "mv_x_max", "mv_y_min", "mv_y_max"), R.MV_LIMITS)), "the decoder predicted with vectors at all four limits"
    assert (sides > 0).all(), "partitions whose reference lies wholly outside, per side: %s" % sides
    assert mvd_writer > 0 and dec_mvd > 8192, (mvd_writer, dec_mvd)


def test_group_steps():
    """the four-stream group: the stream without the new bit sits between streams with it, and the large levels of its steps
    outgrow the lists (1 024 entries at first, then twice what did not fit plus 1 024) at exactly R.GROUP_GROWTH - the first time
    with no stream alone above 1 024, the second time beyond what the first growth made room for"""
    assert [bool(c.features & R.RE) for c in R.GROUP] == [True, True, False, True]
    per = [[R.large_levels(p) for p in R.stream(c)] for c in R.GROUP]
    total = tuple(sum(col) for col in zip(*per))
    assert total == R.GROUP_LARGE
    cap, grown = 1024, []
    for t, n in enumerate(total):
        if n > cap:
            grown.append(t)
            cap = 2 * n + 1024
        else:
            assert n <= 1024, "step %d: a set of the double-buffered host list that has not grown yet would grow here" % t
    assert tuple(grown) == R.GROUP_GROWTH and len(grown) == 2
    first = sorted(s[grown[0]] for s in per)
    assert first[-1] <= 1024 < first[-1] + first[-2], first


TYPE_TO_KIND = {0: OracleDecoder.KIND_I16, 4: OracleDecoder.KIND_I4, 3: OracleDecoder.KIND_IPCM, 2: OracleDecoder.KIND_SKIP,
                1: OracleDecoder.KIND_INTER, 5: OracleDecoder.KIND_INTER, 6: OracleDecoder.KIND_INTER, 7: OracleDecoder.KIND_INTER}


@pytest.mark.parametrize("case", EVERY, ids=[c.name for c in EVERY])
def test_host_parser_reads_what_was_written(case):
    """the product's host parser (mi355x_h264_parser_*, media_amd/csrc/h264_parse.h) against the independent facts, picture by
    picture: macroblock types, coded_block_pattern, TotalCoeff, QP_Y per macroblock, every level the stream carries - those
    outside a signed byte, which the parser keeps in a list of their own, included - and the vector and reference index of every
    4x4 block of every inter macroblock, which the generator wrote as differences from its own predictions and the independent
    decoder added up again.  A parser that bounds mvd_l0 instead of the vector refuses the streams of this module."""
    par = h264dec.Parser()
    for i, p in enumerate(R.stream(case)):
        tag = "%s picture %d" % (case.name, i)
        assert par.parse(p.au), tag
        mb, _, _, lv = par.arrays()
        for fld in ("type", "cbp", "tc"):
            assert np.array_equal(mb[fld], p.mb[fld]), "%s: %s" % (tag, fld)
        assert [TYPE_TO_KIND[int(t)] for t in mb["type"]] == list(p.kinds), tag
        assert np.array_equal(par.mbqp(), p.mbqp), "%s: QP_Y" % tag
        cbp, i16 = p.mb["cbp"].astype(np.int32), p.mb["type"] == 0
        read = np.zeros(p.levels.shape, bool)
        read[i16, 0:16] = True
        for q in range(4):
            read[(cbp >> q) & 1 == 1, 16 + 64 * q: 16 + 64 * (q + 1)] = True
        read[(cbp >> 4) >= 1, 272:280] = True
        read[(cbp >> 4) == 2, 280:408] = True
        read[np.isin(p.mb["type"], (2, 3)), :] = False
        assert not np.where(~read, p.levels, 0).any(), "%s: the writer's levels lie in lists the stream carries" % tag
        got = np.where(read, lv.astype(np.int32), 0)
        if not np.array_equal(got, p.levels):
            k, j = (int(v[0]) for v in np.nonzero(got != p.levels))
            raise AssertionError("%s: macroblock %d (type %d, QP %d) level %d is %d, written %d" % (tag, k, p.mb["type"][k], p.mbqp[k], j, got[k, j], p.levels[k, j]))
        mv4, refq = par.vectors4()
        inter = np.isin(p.mb["type"], (1, 2, 5, 6, 7))
        want = p.mv4[inter]
        assert np.array_equal(mv4[inter].astype(np.int32), want[:, :, :2]), "%s: vectors per 4x4 block" % tag
        quad = [2 * (b >> 3) + ((b >> 1) & 1) for b in range(16)]
        assert np.array_equal(refq[inter][:, quad].astype(np.int32), want[:, :, 2]), "%s: reference index per 4x4 block" % tag
    par.close()
