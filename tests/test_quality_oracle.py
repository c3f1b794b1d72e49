"""What the case list of tests/quality.py holds, proved on the CPU oracle alone (no device): without these facts the GPU test of the
quality report (tests/test_gpu_quality.py) could pass while cropping, I_PCM pictures, the 64-bit sums, the reconstruction ring, the
bands or the item strides went untested."""
import itertools
import numpy as np
import quality as q


def test_restatement_on_a_hand_made_picture():
    """2 x 2 macroblocks of coded size, display 18 x 18: one differing sample per plane inside, one outside the display size"""
    w, h = 18, 18
    src = [np.zeros((18, 18), np.uint8), np.zeros((9, 9), np.uint8), np.zeros((9, 9), np.uint8)]
    rec = [np.zeros((32, 32), np.uint8), np.zeros((16, 16), np.uint8), np.zeros((16, 16), np.uint8)]
    rec[0][17, 16] = 3          # macroblock (1, 1), inside
    rec[0][18, 0] = 200         # outside the display height
    rec[1][0, 8] = 2            # Cb, macroblock (0, 1)
    rec[1][0, 9] = 100          # outside the display width
    rec[2][8, 0] = 5            # Cr, macroblock (1, 0)
    r = q.expected(src, rec, w, h)
    assert r.sse == (9, 4, 25) and r.samples == (324, 81, 81)
    assert r.map.tolist() == [[0, 4], [25, 9]]
    top, bottom = q.expected(src, rec, w, h, 0, 1), q.expected(src, rec, w, h, 1, 1)
    assert top.sse == (0, 4, 0) and top.samples == (16 * 18, 8 * 9, 8 * 9) and bottom.sse == (9, 0, 25) and bottom.samples == (2 * 18, 9, 9)
    assert q.add(top, bottom).sse == r.sse and q.add(top, bottom).samples == r.samples and np.array_equal(q.add(top, bottom).map, r.map)
    assert q.psnr(0, 10) == float("inf") and abs(q.psnr(65025, 1)) < 1e-12


def test_partial_macroblocks_make_a_difference():
    c = q.CROP
    assert c.w % 16 and c.h % 16 and c.w % 4 == 2
    pics = q.oracle_run(c)
    assert [p.idr for p in pics] == [True, False, False, False, True]
    differ = [i for i, p in enumerate(pics) if p.rec.sse != p.coded.sse]
    print("34x18: display and coded sums differ in pictures", differ, [(p.rec.sse, p.coded.sse) for p in pics])
    assert differ, "the sum over the display samples equals the sum over the coded size in every picture: cropping is untested"
    assert all(sum(p.rec.sse) > 0 for p in pics)


def test_pcm_case_holds_pcm_macroblocks_with_no_error():
    pics = q.oracle_run(q.PCM)
    n = 0
    for p in pics:
        pcm = (p.mbtypes == 3).reshape(p.rec.map.shape)
        n += int(pcm.sum())
        assert not p.rec.map[pcm].any(), "an I_PCM macroblock's samples are its source's"
    assert n > 0, "no I_PCM macroblock in the case"


def test_luma_sse_of_the_1080p_noise_picture_needs_64_bits():
    pics = q.oracle_run(q.BIG)
    print("1080p noise at QP 51: sse", pics[0].rec.sse)
    assert pics[0].idr and pics[0].rec.sse[0] > 2 ** 32


def test_multi_reference_case_rewrites_every_ring_slot():
    c = q.REFS3
    assert c.refs == 3 and c.pictures >= 6
    assert min(q.ring_rewrites(c.refs, c.pictures)) >= 1, q.ring_rewrites(c.refs, c.pictures)
    pics = q.oracle_run(c)
    assert [p.idr for p in pics] == [i == 0 for i in range(c.pictures)]   # (one GOP: the ring goes round without a restart)
    assert len({p.rec.sse for p in pics}) == c.pictures


def test_band_records_add_up_to_the_single_instance():
    c = q.SLICES
    one, two = q.oracle_run(c), q.oracle_bands(c, 2)
    assert q.band_rows(c.h, c.slices, 0, 2) == (0, 3) and q.band_rows(c.h, c.slices, 1, 2) == (3, 2)
    for i, (p, (au, recs)) in enumerate(zip(one, two)):
        assert au == p.au, "picture %d: the bands' access unit" % i
        s = q.add(*recs)
        assert s.sse == p.rec.sse and s.samples == p.rec.samples and np.array_equal(s.map, p.rec.map), "picture %d" % i
        assert all(sum(r.sse) > 0 for r in recs)
        assert not recs[0].map[3:].any() and not recs[1].map[:3].any()


def test_lockstep_and_hub_items_are_distinct():
    gops = q.oracle_gops()
    for t in range(q.GOPS[0].pictures):
        for a, b in itertools.combinations(range(len(q.GOPS)), 2):
            assert gops[a][t].rec.sse != gops[b][t].rec.sse and not np.array_equal(gops[a][t].rec.map, gops[b][t].rec.map), (t, a, b)
    b4 = q.oracle_run(q.BATCH4)
    assert len({p.rec.sse for p in b4}) == len(b4)
    hub = [q.oracle_run(c) for c in q.HUB]
    assert [c.qp for c in q.HUB] == [20, 26, 32, 38, 44] and len(q.HUB) == 5
    for t in range(q.HUB[0].pictures):
        for a, b in itertools.combinations(range(5), 2):
            assert hub[a][t].rec.sse != hub[b][t].rec.sse and not np.array_equal(hub[a][t].rec.map, hub[b][t].rec.map), (t, a, b)
    # the stream that sits out a tick codes picture t - 1 while the others code picture t: still no two equal
    k, tick = q.HUB_SITS_OUT
    for t in range(tick + 1, q.HUB[0].pictures):
        assert all(hub[k][t - 1].rec.sse != hub[a][t].rec.sse for a in range(5) if a != k)


def test_plugin_case_cuts_at_its_last_picture():
    """the scene cut of the plugin case: picture 2 of the `cut` content has nothing in common with picture 1"""
    c = q.PLUGIN
    assert c.pictures == 3 and c.gop >= 30
    run = q.plugin_replay(c, (c.qp,) * 3)
    assert [(p.idr, cut) for p, cut in run] == [(True, False), (False, False), (True, True)]
    assert all(min(p.rec.sse) > 0 for p, _ in run), "a picture without error (I_PCM) would be told from no comparison only by its flags"
