"""The stream-hub matrix on the CPU oracle alone (no GPU): proof that the case list of tests/stream_matrix.py, which
tests/test_gpu_stream_matrix.py runs through capi.Stream, is worth running.

On the oracle, the list codes an IDR and a P picture at every QP 10..51 in Baseline and in High; reaches the saturating paths
tests/test_gpu_saturation.py pins, as far as a stream (one reference picture) can, above floors committed in
stream_matrix.FLOORS; holds I_PCM pictures, P pictures with intra macroblocks, P pictures with 16x8, 8x16 and 8x8 partitions
and an access unit that needs emulation prevention; and holds the geometries the issue names.  Every picture is also decoded
by the independent decoder and, in the saturation groups, held against the prediction restated from the standard."""
import numpy as np
import pytest
import adversarial
import spec_pred
import stream_matrix as sm
from oracle_lib import OracleDecoder


def run_stream(s, cov=None, check_pred=False):
    """code the stream on the oracle; returns per picture (qp, idr, mbinfo, access unit, filtered: final planes != pre-filter)"""
    orc, dec = sm.oracle_for(s), OracleDecoder()
    srows = adversarial.slice_rows(orc.ch // 16, s.slices)
    history, out = [], []
    for i, f in enumerate(sm.frames(s)):
        if i and s.qps[i] != s.qps[i - 1]:
            orc.set_qp(s.qps[i])
        au, idr = orc.encode(f, force_idr=i in s.force_idr_at)
        tag = "%s %dx%d profile %d picture %d qp %d" % (s.kind, s.w, s.h, s.prof, i, s.qps[i])
        assert dec.decode(au) == 1, tag
        for p in range(3):
            assert np.array_equal(dec.plane(p), orc.recon(p)), tag + ": decoder plane %d" % p
        assert dec.max_mb_bits <= 3200 and dec.max_level_prefix <= 15, tag
        mbinfo = orc.mbinfo()
        if check_pred:
            if idr:
                history = []
            before = dict(cov)
            spec_pred.check_picture([orc.recon_pre(p) for p in range(3)], history, spec_pred.coded_planes(f, s.w, s.h, orc.cw, orc.ch),
                                    mbinfo, orc.mvq(), orc.mbaux(), orc.levels(), srows, tag=tag, counters=cov)
            sm.tally(cov, s.qps[i], mbinfo, dec.max_level_prefix, before)
            history = [tuple(orc.recon(p) for p in range(3))]
        filtered = any(not np.array_equal(orc.recon(p), orc.recon_pre(p)) for p in range(3))
        out.append((s.qps[i], idr, mbinfo, au, filtered))
    orc.close()
    dec.close()
    return out


@pytest.mark.parametrize("prof", [66, 100])
def test_every_qp_codes_an_idr_and_a_p_picture(prof):
    seen = {True: set(), False: set()}
    intra_in_p = parts = escaped = 0
    for s in sm.all_qps(prof):
        for qp, idr, mb, au, _ in run_stream(s):
            seen[idr].add(qp)
            if not idr:
                intra_in_p += bool(np.isin(mb["type"], (0, 3, 4)).any())
                parts += all((mb["type"] == t).any() for t in (5, 6, 7))
            escaped += b"\x00\x00\x03" in au[au.rfind(b"\x00\x00\x00\x01") + 5:]
    want = set(range(10, 52))
    assert seen[True] == want, "QPs without an IDR picture: %s" % sorted(want - seen[True])
    assert seen[False] == want, "QPs without a P picture: %s" % sorted(want - seen[False])
    assert intra_in_p >= 1, "no P picture with intra macroblocks"
    assert parts >= 1, "no P picture with 16x8, 8x16 and 8x8 partitions together"
    assert escaped >= 1, "no access unit needs emulation prevention"


def saturation_counts(kind):
    cov = {}
    for prof in sm.SAT_PROFILES:
        for s in sm.saturation(prof):
            if s.kind == kind:
                run_stream(s, cov, check_pred=True)
    return cov


@pytest.mark.parametrize("kind", list(adversarial.GENERATORS))
def test_saturation_through_one_reference_reaches_its_floors(kind):
    cov = saturation_counts(kind)
    assert set(sm.FLOORS[kind]) <= set(sm.FLOOR_KEYS)
    short = sm.short_of_floors(kind, cov)
    assert not short, "%s: coverage below its floor: %s (counts %s)" % (kind, ", ".join(short), cov)


def test_the_floors_name_every_counter_somewhere():
    """fractional positions, vectors outside the picture, clamped 6-tap intermediates, clamped plane predictions (luma and
    chroma), I_PCM, level_prefix 15 at both QP ends and TotalCoeff 16: each pinned for at least one content"""
    for key in sm.FLOOR_KEYS:
        assert any(sm.FLOORS[k].get(key, 0) > 0 for k in sm.FLOORS), key


def test_flag_streams_are_i_pcm_all_skip_and_intra_in_p():
    for s in sm.flags(sm.FLAGS_ORDERS[0]):
        for i, (qp, idr, mb, au, filtered) in enumerate(run_stream(s)):
            if s.kind == "noise":
                assert (mb["type"] == 3).any() and not filtered, "picture %d: an I_PCM picture is not filtered" % i
            elif idr:
                continue
            elif s.kind == "s2":
                assert not np.isin(mb["type"], (0, 3, 4)).any() and (i < 2 or (mb["type"] == 2).all()), "picture %d: no intra, then all P_Skip" % i
            else:
                assert np.isin(mb["type"], (0, 4)).any() and filtered, "picture %d: intra macroblocks in a filtered P picture" % i
    assert sorted(sm.FLAGS_ORDERS[1]) == list(range(6)) and sm.FLAGS_ORDERS[1] != sm.FLAGS_ORDERS[0]


def test_the_list_holds_the_geometries_and_options():
    groups = sm.geometry()
    sizes = [(g[0].w, g[0].h) for g in groups]
    for wh in ((16, 16), (32, 16), (16, 48), (18, 18), (50, 34), (130, 98), (2048, 16), adversarial.SIZE):
        assert wh in sizes, wh
    assert len(groups) >= 8 + 24 and len(set(sizes)) >= 30
    for g in groups:
        assert len(g) == 3 and len({(s.w, s.h, s.prof, s.slices, s.search, s.nodeblock, s.nv12_device) for s in g}) == 1, "one engine per group"
        assert g[0].w % 2 == 0 and g[0].h % 2 == 0
    for field, values in (("nodeblock", (0, 1)), ("search", (0, 1)), ("slices", (0, 3)), ("nv12_device", (False, True))):
        assert {getattr(g[0], field) for g in groups} == set(values), field
    assert any(((g[0].w + 15) // 16) % 2 == 1 and ((g[0].h + 15) // 16) % 2 == 1 for g in groups), "odd macroblock counts"
    assert {(s.w, s.h) for wh in sm.FILTER_FORM_SIZES for s in sm.filter_forms(*wh)} == {(176, 112), (64, 16), (16, 64)}
    assert (sm.FILTER_FORM_STREAMS + 2) // 3 >= 8, "a P step of the filter-form groups can hold eight pictures"
    assert [(s.w, s.h) for s in sm.full_size()] == [(1920, 1080)] * 4
    assert sm.churn()[1].force_idr_at == (3,)


def print_counts():
    """python tests/test_stream_matrix_oracle.py: the oracle's counts and the floors to commit (count less a tenth)"""
    for kind in adversarial.GENERATORS:
        cov = saturation_counts(kind)
        print('    "%s": {%s},' % (kind, ", ".join('"%s": %d' % (k, cov[k] - (cov[k] + 9) // 10) for k in sm.FLOOR_KEYS if cov.get(k, 0) - (cov.get(k, 0) + 9) // 10 > 0)))
        print("    # counts:", {k: cov.get(k, 0) for k in sm.FLOOR_KEYS})


if __name__ == "__main__":
    print_counts()
