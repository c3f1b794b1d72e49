"""CPU proof for tests/deblock_cells.py: the list holds what it claims.  Every fact comes from the oracle decoder's own account of
its loop filter (h264o_dec_dbf: oracle/h264_oracle.h), which knows nothing of the product: every (plane kind, bS, indexA 16 .. 51)
cell changes samples on at least FLOOR lines, every indexB is filtered, every branch and context cell is met, every picture is
conforming, and every rewritten header is in force.  The coverage of the older lists is printed beside the new one's (DESIGN.md
section 10 holds the same table)."""
import functools

import numpy as np
import pytest

import deblock_cells as D
import dec_group
import range_ends
from media_amd import h264dec, synth
from oracle_lib import OracleEncoder, OracleDecoder, Dbf
from slice_header import read_header
from temporal import nal_units

ENC = [c for c in D.CASES if c.kind == "enc"]


@functools.lru_cache(maxsize=None)
def total():
    return D.account(D.CASES)


def test_every_index_of_both_planes_and_every_strength_changes_samples():
    """no exception: luma and chroma, bS 1 .. 4, indexA 16 .. 51 - at least FLOOR lines where a sample changed; below 16 lines are
    evaluated and never filtered (alpha = beta = 0)"""
    t = total()
    chg = t.tables["a_changed"]
    thin = [(("luma", "chroma")[k], b + 1, a, int(chg[k, b, a])) for k in range(2) for b in range(4) for a in range(16, 52) if chg[k, b, a] < D.FLOOR]
    assert not thin, "(kind, bS, indexA, changed lines) below the floor of %d: %s" % (D.FLOOR, thin)
    for k in range(2):
        assert t.tables["a_eval"][k, :, :16].sum() > 0 and t.tables["a_filt"][k, :, :16].sum() == 0
        assert (t.tables["a_eval"][k, :, :16].sum(axis=0) > 0).all(), "every indexA below 16 is evaluated"


def test_every_indexB_is_filtered_and_ap_is_met_true_and_false():
    t = total()
    bf = t.tables["b_filt"]
    for k in range(2):
        assert (bf[k].sum(axis=0)[16:] > 0).all(), [i for i in range(16, 52) if bf[k].sum(axis=0)[i] == 0]
        assert bf[k][:, :16].sum() == 0
    n, ap, aq = bf[D.LUMA].sum(axis=0)[16:], t.tables["b_ap"][D.LUMA].sum(axis=0)[16:], t.tables["b_aq"][D.LUMA].sum(axis=0)[16:]
    assert ((ap > 0) & (ap < n)).all() and ((aq > 0) & (aq < n)).all(), (ap, aq, n)


def test_index_classes_cross():
    """pictures with indexA >= 16 and indexB < 16 and the reverse (their rows of D.LOW_ROWS): lines evaluated, none filtered"""
    pics = D.stream(D.BY_NAME["low_66_split"])
    for i, p in enumerate(pics):
        if p.reheaded:
            a, b = p.row.qp + 2 * p.row.oa, p.row.qp + 2 * p.row.ob
            assert (a < 16 or b < 16) and p.dbf.tables["a_eval"].sum() > 0 and p.dbf.tables["a_filt"].sum() == 0, (i, p.row)
    rows = [p.row for p in pics if p.reheaded]
    assert any(r.qp + 2 * r.oa >= 16 > r.qp + 2 * r.ob for r in rows) and any(r.qp + 2 * r.ob >= 16 > r.qp + 2 * r.oa for r in rows)
    assert any(r.qp + 2 * r.oa < 16 and r.qp + 2 * r.ob < 16 for r in rows)


def test_every_branch_and_context_cell_is_met():
    t = total()
    assert len(D.UNREACHABLE) <= 3
    unmet = [c for c in D.BRANCH_CELLS if D.branch_count(t, c) == 0 and c not in D.UNREACHABLE]
    unmet += [c for c in D.CONTEXT_CELLS if t.ctx[c] == 0 and c not in D.UNREACHABLE]
    assert not unmet, unmet
    reached = [c for c in D.UNREACHABLE if (t.ctx[c] if isinstance(c, str) else D.branch_count(t, c))]
    assert not reached, "declared unreachable, and met: %s" % reached


def test_the_schedule_aims_every_index_under_two_offsets():
    """every luma indexA 16 .. 51, every chroma indexA 16 .. 51 (QPc of the encoder's streams: chroma_qp_index_offset 0) and every
    indexB 16 .. 51 is the aim of rows with at least two different offsets; every row is coded at or above its target QP"""
    la, ca, lb = {}, {}, {}
    for r in D.SCHEDULE:
        assert r.coded >= r.qp and r.coded in [min(51, max(10, r.qp + b)) for b in (0, 4, 8)], r
        la.setdefault(min(51, max(0, r.qp + 2 * r.oa)), set()).add(r.oa)
        ca.setdefault(min(51, max(0, D.QPC[r.qp] + 2 * r.oa)), set()).add(r.oa)
        lb.setdefault(min(51, max(0, r.qp + 2 * r.ob)), set()).add(r.ob)
    for name, m in (("luma indexA", la), ("chroma indexA", ca), ("indexB", lb)):
        one = [i for i in range(16, 52) if len(m.get(i, ())) < 2]
        # QPc <= 39 (Table 8-15) and the offset is even and <= 12: 50 = 38 + 12 and 51 = 39 + 12 are the only ways there.  Those two
        # are aimed at under two different SliceQP_Y instead
        if name == "chroma indexA":
            assert one == [50, 51] and all(len({r.qp for r in D.SCHEDULE if D.QPC[r.qp] + 2 * r.oa == i}) >= 2 for i in one), one
            continue
        assert not one, "%s under fewer than two offsets: %s" % (name, one)
    assert any(i < 16 for i in la) and any(i < 16 for i in lb) and 0 in lb


@pytest.mark.parametrize("case", D.CASES, ids=[c.name for c in D.CASES])
def test_every_picture_is_conforming_and_every_new_header_is_in_force(case):
    """D.stream() has the independent decoder decode every picture (it asserts that).  Its greatest intermediate of 8.5.10 - 8.5.13
    stays inside 16 bits.  A re-headed picture decodes to other samples than the encoder's own access unit does in its place
    (same pictures in front): the new header is in force.  The product's host parser reads the header the row asks for."""
    pics = D.stream(case)
    par = h264dec.Parser()
    for i, p in enumerate(pics):
        tag = "%s picture %d %s" % (case.name, i, p.row)
        assert p.stats["max_intermediate"] <= 32767, (tag, p.stats)
        assert par.parse(p.au), tag
        if p.reheaded:
            info = par.info()
            assert (info["deblock_idc"], info["filter_oa"], info["filter_ob"]) == (p.row.idc, 2 * p.row.oa, 2 * p.row.ob), (tag, info)
            # SliceQP_Y of every slice as the row names it (slice k: qp - k * step); the encoder writes no mb_qp_delta, so it is the
            # QP_Y of every macroblock of the slice
            first = [read_header(n).first_mb for n in nal_units(p.au) if (n[0] & 31) in (1, 5)] + [len(p.kinds)]
            want = np.concatenate([np.full(first[k + 1] - first[k], p.row.qp - k * p.row.step) for k in range(len(first) - 1)])
            assert info["qp"] == p.row.qp and np.array_equal(par.mbqp(), want), (tag, info["qp"], par.mbqp())
            dec = OracleDecoder()
            for q in pics[:i]:
                dec.decode(q.au)
            assert dec.decode(p.orig) == 1
            assert any(not np.array_equal(dec.plane(k), p.planes[k]) for k in range(3)), "%s: the same samples under the old header" % tag
            dec.close()
    par.close()
    if case.kind == "enc":
        assert sum(p.pcm for p in pics) <= 2, "pictures left alone for an I_PCM macroblock"
        assert all(p.reheaded or p.pcm or (p.row.qp, p.row.oa, p.row.ob, p.row.idc) == (p.row.coded, 0, 0, 0) for p in pics)


def test_sizes_and_lengths():
    sizes = {(c.w, c.h) for c in D.CASES}
    assert sizes == {(16, 16), (32, 16), (16, 48), (64, 48), (96, 80)}
    assert all(c.slices for c in D.CASES if c.kind == "enc" and (c.w, c.h) == (96, 80))
    assert all(6 <= len(c.rows) <= 12 for c in ENC)
    assert {c.prof for c in ENC} == {66, 77, 100} and any(c.refs == 3 and c.prof == 100 for c in ENC)


def _sweep():
    """the encoder's own streams, QP 10 .. 51: 64x48, six pictures each, content and profile in turn"""
    for qp in range(10, 52):
        prof, _, refs, content, _, _ = D.CONFIGS[qp % 3]
        enc = OracleEncoder(64, 48, qp=qp, gop=1000, profile_idc=prof, refs=refs)
        yield [enc.encode(f)[0] for f in synth.sequence("s1" if content == "cut" else content, 64, 48, 6)]
        enc.close()


def test_coverage_of_the_lists_side_by_side(capsys):
    """the table of DESIGN.md section 10: the older lists against the new one.  The rows of the older lists are printed, not
    asserted (a list may get better); asserted is that the new list's row is complete"""
    lists = {}
    acc = Dbf()
    for c in range_ends.CASES:
        acc = acc + D.account_of([p.au for p in range_ends.stream(c)])
    lists["range_ends"] = acc
    acc = Dbf()
    for c in dec_group.CASES:
        for k in range(len(c.streams)):
            acc = acc + D.account_of([p[0] for p in dec_group.stream_pictures(c, k)])
    lists["dec_group"] = acc
    acc = Dbf()
    for aus in _sweep():
        acc = acc + D.account_of(aus)
    lists["encoder QP 10..51"] = acc
    lists["deblock_cells"] = total()
    rows = {k: D.coverage(v) for k, v in lists.items()}
    with capsys.disabled():
        keys = list(rows["deblock_cells"])
        print("\n%-20s" % "list" + "".join("%18s" % k for k in keys))
        for name, r in rows.items():
            print("%-20s" % name + "".join("%18d" % r[k] for k in keys))
    new = rows["deblock_cells"]
    assert all(new[k] == 0 for k in new if k not in ("lines", "filtered")), new
