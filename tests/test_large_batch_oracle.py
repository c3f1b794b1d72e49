"""The large lockstep steps on the CPU oracle alone (no GPU): proof that the case list of tests/large_batch.py, which
tests/test_gpu_large_batch.py runs on the GPU, is worth running.

For every case: all items' streams differ pairwise (an item coded from another item's data cannot pass); every content kind
reaches what it is there for - I_PCM, Intra4x4 and Intra16x16 inside P pictures, 16x8 / 8x16 / 8x8 partitions, all-skip P
pictures, a vector that points outside the picture - and does so at an item index of 24 or more (48 or more in the case of 64
items): in a picture the row wavefront walks to; the sparse and the dense variant lie on their own sides of the threshold of
the schedule switch, by the engine's running mean restated in large_batch.schedule with its constants read from engine.h; and
every access unit decodes on the independent decoder to the oracle encoder's reconstruction."""
import numpy as np
import pytest
import large_batch as lb

INTER = (1, 5, 6, 7)    # (P_Skip's vector is the predicted one: MbInfo does not carry it)


def vectors_outside(pic, w, h):
    """8x8 quadrants of inter macroblocks whose vector (integer part) takes them over the picture's edge"""
    mbw, n = (w + 15) // 16, 0
    for m in np.nonzero(np.isin(pic.mbinfo["type"], INTER))[0]:
        for q in range(4):
            x = 16 * (m % mbw) + 8 * (q & 1) + (int(pic.mvq[m, 2 * q]) >> 2)
            y = 16 * (m // mbw) + 8 * (q >> 1) + (int(pic.mvq[m, 2 * q + 1]) >> 2)
            n += x < 0 or y < 0 or x + 8 > w or y + 8 > h
    return n


def reaches(kind, pic, c):
    """does this P / IDR picture of an item of `kind` hold what the kind is in the list for"""
    t = pic.mbinfo["type"]
    if kind in (lb.PCM_KIND, "s3"):    # (s3 is noise: at the QPs of these cases it goes I_PCM as well)
        return bool((t == 3).any())
    if pic.idr:
        return False
    if kind in ("cut", "flip", "patch"):
        return bool((t == 4).any()) and lb.to_intra(pic) > 0
    if kind == "gradient":
        return bool((t == 0).any()) and lb.to_intra(pic) > 0
    if kind == "split":
        return all((t == k).any() for k in (5, 6, 7))
    if kind == "still":
        return pic.all_skip
    return vectors_outside(pic, c.w, c.h) > 0    # s1, scroll


def first_item_reaching(c, pics, kind, lowest):
    for g in range(lowest, c.G):
        if c.kinds[g][0] == kind and any(reaches(kind, p, c) for call in pics for p in call[g]):
            return g
    return None


@pytest.mark.parametrize("c", lb.DIRECT_CASES, ids=[c.name for c in lb.DIRECT_CASES])
def test_every_item_differs_and_every_kind_reaches_a_walked_picture(c):
    pics, _ = lb.expected(c, True)    # (decodes every access unit and compares the planes)
    for call in range(c.calls):
        gops = [b"".join(p.au for p in pics[call][g]) for g in range(c.G)]
        assert len(set(gops)) == c.G, "%s call %d: two items code to the same stream" % (c.name, call)
        # beyond the slice header's idr_pic_id: the pictures themselves differ
        assert len({lb.frames(c, call, g)[-1].tobytes() for g in range(c.G)}) == c.G, "%s call %d: two items show the same picture" % (c.name, call)
    for kind in {k for k, _ in c.kinds}:
        assert first_item_reaching(c, pics, kind, 0) is not None, "%s: no item of %s reaches what it is there for" % (c.name, kind)
    k = lb.engine_constants()
    for kind in c.late:
        assert first_item_reaching(c, pics, kind, k["INTRA_SLOTS"]) is not None, "%s: %s reaches nothing at an item of %d or more" % (c.name, kind, k["INTRA_SLOTS"])
        if c.G >= 2 * k["INTRA_SLOTS"] + 8:
            assert first_item_reaching(c, pics, kind, 2 * k["INTRA_SLOTS"]) is not None, "%s: %s reaches nothing in the third pass of the walk" % (c.name, kind)


def test_the_walk_cases_are_the_sizes_and_walks_the_list_names():
    k = lb.engine_constants()
    slots = k["INTRA_SLOTS"]
    walks = {c.name: [min(slots, c.G - y) for y in range(0, c.G, slots)] for c in lb.WALK_CASES}
    assert walks == {"baseline_64": [24, 24, 16], "high_40": [24, 16], "main_2refs_25": [24, 1], "slices_32": [24, 8]}
    assert [(c.w, c.h, c.prof, c.refs, c.slices) for c in lb.WALK_CASES] == [(64, 48, 66, 0, 0), (96, 80, 100, 0, 0), (96, 80, 77, 2, 0), (176, 144, 66, 0, 3)]
    for c in lb.WALK_CASES:
        assert c.calls == 2 and c.gop in (4, 5)
        if c.G >= 32:
            assert c.late >= frozenset(lb.PATTERN), "%s: every kind lies at an item of 24 or more" % c.name
    assert lb.by_name("main_2refs_25").kinds[24][0] == "cut" and lb.by_name("main_2refs_25").late == {"cut"}
    assert all(c.G >= 32 and c.calls >= 3 for c in (lb.SPARSE, lb.DENSE))
    for c, walk in zip(lb.SLOTS3_CASES, ([3, 3, 2], [3, 3, 2], [3, 3, 1], [3, 3, 1])):
        assert [min(3, c.G - y) for y in range(0, c.G, 3)] == walk
    assert lb.SLOTS1_CASE.G == 4 and lb.PSLOTS3_CASE.G == 8 and 1 < 3 < lb.PSLOTS3_CASE.G


def test_sparse_and_dense_lie_on_their_sides_of_the_schedule_switch():
    k = lb.engine_constants()
    thr = 16 * k["PINTRA_SPARSE_MBS"]
    pics, _ = lb.expected(lb.SPARSE)
    sched = lb.schedule(lb.SPARSE, pics, k)
    assert len(sched) == lb.SPARSE.calls * (lb.SPARSE.gop - 1)
    assert all(p <= thr for _, _, p in sched), "sparse: the mean rises above the threshold: %s" % sched
    counts = [lb.to_intra(p) for call in pics for gop in call for p in gop if not p.idr]
    assert any(1 <= x <= k["PINTRA_SPARSE_MBS"] for x in counts), "sparse: no P picture with 1 .. %d intra macroblocks" % k["PINTRA_SPARSE_MBS"]
    assert max(counts) <= k["PINTRA_SPARSE_MBS"] and counts.count(0) > len(counts) // 2, "sparse: a few intra macroblocks in a few items, none in the rest"
    assert any(p > 0 for _, _, p in sched), "sparse: the mean never left zero: the counters would not be seen to arrive"
    pics, _ = lb.expected(lb.DENSE)
    sched = lb.schedule(lb.DENSE, pics, k)
    assert all(p > thr for call, _, p in sched if call >= 1), "dense: the mean falls to the threshold or below after the first call: %s" % sched
    assert sched[0][2] <= thr, "dense: the first P step of all is still on the sparse side (the switch happens inside the run)"
    # the child-process case with three pictures resident at a time (MI355X_H264_PINTRA_SLOTS overrides the rule), the same
    # content: every P step has intra macroblocks in pictures a workgroup starts with AND in pictures it walks to, whichever of the
    # three grid positions takes them
    c = lb.PSLOTS3_CASE
    pics, _ = lb.expected(c)
    for call in range(c.calls):
        for i in range(1, c.gop):
            with_intra = [g for g in range(c.G) if lb.to_intra(pics[call][g][i])]
            assert {g % 3 for g in with_intra if g >= 3} == {0, 1, 2} and {g for g in with_intra if g < 3} == {0, 1, 2}, (call, i, with_intra)


def test_the_handed_over_count_agrees_with_mbinfo():
    """large_batch.to_intra counts from the oracle's record of the motion stage's decision.  MbInfo alone does not say it: an
    I_PCM macroblock of a P picture is either an intra macroblock that outgrew CAVLC (handed over: counted) or an inter one that
    did (never handed over).  Everywhere else the two agree: handed over <=> Intra16x16 or Intra4x4"""
    seen_pcm_in_p = 0
    for c in lb.DIRECT_CASES:
        pics, _ = lb.expected(c)
        for call in pics:
            for gop in call:
                for p in gop:
                    if p.idr:
                        continue
                    t = p.mbinfo["type"]
                    assert np.array_equal((p.decision == 1) & (t != 3), np.isin(t, (0, 4))), c.name
                    assert not ((p.decision == 2) & ~np.isin(t, (1, 2))).any(), "%s: a settled macroblock is P_L0_16x16 or P_Skip" % c.name
                    assert not ((p.decision == 2) & (p.mbinfo["cbp"] != 0)).any(), "%s: a settled macroblock has nothing coded" % c.name
                    seen_pcm_in_p += int((t == 3).sum())
    assert seen_pcm_in_p > 0


def test_hub_groups():
    for name, make in lb.HUB_GROUPS.items():
        specs = make()
        assert len(specs) in (48, 64) and len(specs) <= lb.HUB_ITEMS
        assert len({(s.w, s.h, s.prof, s.slices, s.search, s.nodeblock, s.nv12_device) for s in specs}) == 1, "one engine per group"
        assert all((s.w, s.h) == lb.HUB_SIZE and s.gop == 3 and len(s.qps) == 6 for s in specs)
        assert {s.qps[0] for s in specs} == set(range(10, 52)), "%s: every QP 10 .. 51" % name
        pictures = [b"".join(f.tobytes() for f in lb.sm.frames(s)) for s in specs]
        assert len(set(pictures)) == len(specs), "%s: every stream shows pictures of its own" % name
    assert any(s.nv12_device for make in lb.HUB_GROUPS.values() for s in make())
    walk = lb.hub_group(lb.HUB_WALK_STREAMS)
    assert len(walk) == 12 and lb.HUB_WALK_SLOTS == 2
