"""CPU proof for tests/pred_cells.py: the list reaches what it claims.  Every fact comes from the oracle decoder's own account of its
prediction (h264o_dec_pred: oracle/h264_oracle.h), which knows nothing of the product: every cell the standard allows is met at least
FLOOR times, no cell it forbids is met at all, the account agrees with a recount from the decoder's vectors and with the writer's
counters, the product's host parser finds the neighbour availability the oracle decoder used, and every picture is conforming.  The
coverage of the older lists is printed beside the new one's (DESIGN.md section 10 holds the same table)."""
import functools

import numpy as np
import pytest

import dec_group
import pred_cells as P
import range_ends
from media_amd import h264dec, synth
from oracle_lib import OracleEncoder, OracleDecoder, Pred

RAND = [c for c in P.CASES if c.kind == "rand"]
INTER = (OracleDecoder.KIND_INTER, OracleDecoder.KIND_SKIP)


@functools.lru_cache(maxsize=None)
def total():
    return P.account(P.CASES)


def test_every_legal_cell_is_met(capsys):
    """no exception beyond P.UNREACHABLE, and nothing is declared there without its subclause"""
    t = total()
    legal = sum(int(a.sum()) for a in P.LEGAL.values())
    with capsys.disabled():
        print("\n%d cells, %d legal by rule, %d declared unreachable; the thinnest: %s" % (Pred.COUNT, legal, len(P.UNREACHABLE), P.thin(t, 1 << 30)[:12]))
    assert all(isinstance(why, str) and "." in why and any(ch.isdigit() for ch in why) for why in P.UNREACHABLE.values()), "a subclause next to every unreachable cell"
    assert all(P.LEGAL[name][idx] for name, idx in P.UNREACHABLE), "declared unreachable, and excluded by rule already"
    below = P.thin(t)
    assert not below, "(section, index, times met) below the floor of %d: %s" % (P.FLOOR, below)
    reached = [(k, int(t[k[0]][k[1]])) for k in P.UNREACHABLE if t[k[0]][k[1]]]
    assert not reached, "declared unreachable, and met: %s" % reached


def test_no_cell_the_rules_exclude_is_met():
    """the rules of P.legal_cells() are the standard's: a count in a cell they exclude is a wrong rule or a wrong account"""
    t = total()
    wrong = [(name, tuple(int(i) for i in idx), int(t[name][idx])) for name, _ in Pred.SECTIONS for idx in zip(*np.nonzero(~P.LEGAL[name] & (t[name] > 0)))]
    assert not wrong, wrong
    assert sum(int(a.sum()) for a in P.LEGAL.values()) == 676 and int(P.LEGAL["l_clip"].sum()) == 46 and int(P.LEGAL["i4"].sum()) == 43


def recount(pic):
    """from h264o_dec_mb_mv and h264o_dec_mb_kind alone: [ref_idx_l0][yFrac][xFrac] over the 4x4 blocks of the inter macroblocks, their
    number, and the horizontally adjacent pairs by how their vectors differ"""
    inter = np.isin(pic.kinds, INTER)
    v = pic.mv4[inter].astype(np.int64)   # (n, 16, 3)
    ref = np.zeros((3, 4, 4), np.int64)
    np.add.at(ref, (v[:, :, 2].ravel(), (v[:, :, 1] & 3).ravel(), (v[:, :, 0] & 3).ravel()), 1)
    a, b = v[:, 0::2, :2], v[:, 1::2, :2]   # raster blocks (0, 1), (2, 3) ... : the pairs inside the 8x8 quadrants
    same = (a == b).all(axis=2)
    integer = ((a >> 3) != (b >> 3)).any(axis=2)
    return ref, 16 * int(inter.sum()), np.array([same.sum(), (~same & integer).sum(), (~same & ~integer).sum()], np.int64)


@pytest.mark.parametrize("case", P.CASES, ids=[c.name for c in P.CASES])
def test_the_account_is_honest_and_the_parser_finds_the_same_neighbours(case):
    """per picture: the account's per-block table, its number of inter 4x4 blocks and its pair classes equal a recount in Python from
    the decoder's vectors and kinds; the per-partition tables add up to one another; (random cases) the Intra4x4 mode totals are the
    writer's; the product's host parser reads the access unit and its availability bits per macroblock are those the oracle decoder
    used; the intermediates of 8.5 stay inside 16 bits"""
    par = h264dec.Parser()
    for i, p in enumerate(P.stream(case)):
        tag = "%s picture %d" % (case.name, i)
        ref, blocks, pairs = recount(p)
        assert np.array_equal(p.pred["b_ref"], ref) and int(p.pred["b_ref"].sum()) == blocks, tag
        assert np.array_equal(p.pred["c_pair"], pairs), (tag, p.pred["c_pair"], pairs)
        parts = int(p.pred["l_shape"].sum())
        assert parts == p.pred["l_ref"].sum() == p.pred["c_frac"].sum() == p.pred["l_rel"][0].sum() == p.pred["l_rel"][1].sum() == p.pred["c_rel"][0].sum(), tag
        assert int(p.pred["l_shape"][0].sum()) == int((p.kinds == OracleDecoder.KIND_SKIP).sum()), tag
        assert int(p.pred["i4"].sum()) == 16 * int((p.kinds == OracleDecoder.KIND_I4).sum()) and int(p.pred["i16"].sum()) == int((p.kinds == OracleDecoder.KIND_I16).sum()), tag
        assert int(p.pred["ic"].sum()) == int(np.isin(p.kinds, (OracleDecoder.KIND_I4, OracleDecoder.KIND_I16)).sum()), tag
        assert (p.pred["i4_nb"].sum(axis=1) == p.pred["i4"].sum()).all(), tag
        if p.i4_hits is not None:
            assert np.array_equal(p.pred["i4"].sum(axis=1), p.i4_hits.sum(axis=0)), (tag, p.pred["i4"].sum(axis=1), p.i4_hits.sum(axis=0))
        assert p.stats["max_intermediate"] <= 32767, (tag, p.stats)
        assert par.parse(p.au), tag
        got = par.mbavail()
        assert np.array_equal(got, p.avail), "%s: macroblocks %s: the parser has %s, the independent decoder used %s" % (
            tag, np.nonzero(got != p.avail)[0][:8], got[got != p.avail][:8], p.avail[got != p.avail][:8])
        if not p.constrained:   # (bits 4..7 differ from bits 0..3 only under constrained_intra_pred_flag)
            assert np.array_equal(p.avail >> 4, p.avail & 15), tag
    par.close()
    if case.kind == "rand" and case.features & P.CI and case.w * case.h >= 48 * 48:
        assert any(((p.avail >> 4) != (p.avail & 15)).any() for p in P.stream(case)), "%s: constrained_intra_pred_flag is in force" % case.name


def test_sizes_lengths_and_features():
    assert {(c.w, c.h) for c in P.CASES} == {(16, 16), (32, 16), (16, 48), (48, 48), (64, 48), (96, 80), (112, 64)}
    assert all(c.pictures in (6, 12) for c in P.CASES)
    assert all(c.prof == 100 and c.refs == 3 for c in P.CASES if (c.w, c.h) == (112, 64))
    for bit in (32, 64, 128):
        assert all(c.features & bit for c in RAND)
    for bit in (P.CI, P.RE, P.PC):
        assert any(c.features & bit for c in RAND) and any(not c.features & bit for c in RAND)
    assert {c.refs for c in RAND} == {1, 2, 3} and {c.prof for c in P.CASES} == {66, 77, 100}
    assert any(c.kind == "enc" for c in P.CASES)


def _sweep():
    """the encoder's own streams, QP 10 .. 51: 64x48, six pictures each, content and profile in turn"""
    for qp in range(10, 52):
        prof, refs, content = ((66, 1, "split"), (77, 1, "s1"), (100, 3, "s1"))[qp % 3]
        enc = OracleEncoder(64, 48, qp=qp, gop=1000, profile_idc=prof, refs=refs)
        yield [enc.encode(f)[0] for f in synth.sequence(content, 64, 48, 6)]
        enc.close()


def test_coverage_of_the_lists_side_by_side(capsys):
    """the table of DESIGN.md section 10: per family the legal cells, those never met and those met fewer than FLOOR times, the older
    lists against the new one.  The rows of the older lists are printed, not asserted (a list may get better); asserted is that the
    new list's row is complete"""
    lists = {}
    acc = Pred()
    for c in range_ends.CASES:
        acc = acc + P.account_of([p.au for p in range_ends.stream(c)])
    lists["range_ends"] = acc
    acc = Pred()
    for c in dec_group.CASES:
        for k in range(len(c.streams)):
            acc = acc + P.account_of([p[0] for p in dec_group.stream_pictures(c, k)])
    lists["dec_group"] = acc
    acc = Pred()
    for aus in _sweep():
        acc = acc + P.account_of(aus)
    lists["encoder QP 10..51"] = acc
    lists["pred_cells"] = total()
    rows = {k: P.coverage(v) for k, v in lists.items()}
    with capsys.disabled():
        fams = list(rows["pred_cells"])
        print("\n%-20s" % "list" + "".join("%26s" % f for f in fams))
        print("%-20s" % "(legal cells)" + "".join("%26d" % rows["pred_cells"][f][0] for f in fams))
        for name, r in rows.items():
            print("%-20s" % name + "".join("%26s" % ("never %d, < %d: %d" % (r[f][1], P.FLOOR, r[f][2])) for f in fams))
    assert all(never == 0 and below == 0 for _, never, below in rows["pred_cells"].values()), rows["pred_cells"]
