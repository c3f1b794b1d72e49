"""What tests/ssim.py states and what its case list holds, proved on the CPU oracle alone (no device): the known answers of the
header's definition, the window counts, the bounds the header claims for the integer terms, the distance from the floating-point
SSIM, and the facts without which the GPU test (tests/test_gpu_ssim.py) could pass while negative windows, the floor of a negative
quotient, I_PCM pictures, the bands or the item strides went untested."""
import itertools
import numpy as np
import quality as q
import ssim as S


def _window(a, b):
    """(l, c, q) of one 8x8 window given as two arrays"""
    l, c, qq = S.evaluate(S.window_sums(np.asarray(a, np.uint8).reshape(8, 8), np.asarray(b, np.uint8).reshape(8, 8)))
    assert l.shape == (1, 1)
    return int(l[0, 0]), int(c[0, 0]), int(qq[0, 0])


def test_known_answers():
    noise = np.random.default_rng(3).integers(0, 256, 64)
    half = np.array([0] * 32 + [255] * 32)
    assert _window(noise, noise) == (65536, 65536, 65536)
    assert _window(np.full(64, 100), np.full(64, 110)) == (65239, 65536, 65239)
    assert _window(np.zeros(64), np.full(64, 255)) == (0, 65536, 0)
    assert _window(half, 255 - half) == (65536, -65305, -65305)
    # floor, not truncation: the negative quotient is no integer (truncation would give -65304)
    t = S.evaluate_py(32 * 255, 32 * 255, 64 * 65025, 0)[3]
    assert t["cn"] < 0 and t["cn"] % t["cd"] != 0 and t["cn"] // t["cd"] == -65305 and -((-t["cn"]) // t["cd"]) == -65304


def test_window_counts():
    """(W / 4 - 1) * (H / 4 - 1) per plane; 34x18 has chroma planes of 17x9: 3 x 1 windows"""
    for (w, h), want in (((16, 16), (9, 1, 1)), ((34, 18), (7 * 3, 3 * 1, 3 * 1)), ((50, 34), (11 * 7, 5 * 3, 5 * 3))):
        src = [np.zeros((h, w), np.uint8), np.zeros((h // 2, w // 2), np.uint8), np.zeros((h // 2, w // 2), np.uint8)]
        cw, ch = (w + 15) // 16 * 16, (h + 15) // 16 * 16
        rec = [np.zeros((ch, cw), np.uint8), np.zeros((ch // 2, cw // 2), np.uint8), np.zeros((ch // 2, cw // 2), np.uint8)]
        r = S.expected(src, rec, w, h)
        assert r.windows == want == (S.window_count(w, h), S.window_count(w // 2, h // 2), S.window_count(w // 2, h // 2)), (w, h)
        assert r.sum == tuple(65536 * n for n in want) and int(r.map.sum()) == 65536 * want[0]
        # every window brute force: origin (4i, 4j), 8x8, wholly inside
        assert want[0] == sum(1 for j in range(0, h, 4) for i in range(0, w, 4) if i + 8 <= w and j + 8 <= h)
    assert S.oracle_run(S.TINY)[0].rec.windows == (9, 1, 1) and S.oracle_run(q.CROP)[0].rec.windows == (21, 3, 3)
    assert S.oracle_run(q.NV12)[0].rec.windows == (77, 15, 15)


def test_map_entries_are_the_windows_whose_origin_lies_in_the_macroblock():
    p = S.oracle_run(q.CROP)[1].rec      # 34x18: 3 x 2 macroblocks, 7 x 3 luma windows
    assert p.map.shape == (2, 3) and p.q[0].shape == (3, 7)
    for my, mx in itertools.product(range(2), range(3)):
        want = sum(int(p.q[0][j, i]) for j in range(3) for i in range(7) if (4 * j) // 16 == my and (4 * i) // 16 == mx)
        assert int(p.map[my, mx]) == want
    assert not p.map[1].any()            # (origin rows 0, 4, 8 only: 16 + 8 > 18)


def test_int64_equals_python_integers_and_the_bounds_hold():
    """every window of every case: numpy's int64 evaluation against Python integers, and what the header states about the terms"""
    n = 0
    worst = {"pre": 0, "num": 0}
    for c in S.ALL:
        for pic in S.oracle_run(c):
            for plane in range(3):
                sums = pic.rec.sums[plane]
                l, cc, qq = S.evaluate(sums)
                for idx in np.ndindex(*qq.shape):
                    pl, pc, pq, t = S.evaluate_py(*(int(v[idx]) for v in sums))
                    assert (pl, pc, pq) == (int(l[idx]), int(cc[idx]), int(qq[idx])), (c.name, plane, idx)
                    assert pq == int(pic.rec.q[plane][idx])
                    assert 0 <= pl <= 65536 and -65535 <= pc <= 65536
                    assert 2 * abs(t["covar"]) <= t["vars"]
                    pre = max(abs(t["vars"]), abs(t["covar"]), t["ld"], t["cd"], t["ln"] >> 16, abs(t["cn"] >> 16) + 1)
                    assert pre < 2 ** 31 and abs(t["ln"]) < 2 ** 47 and abs(t["cn"]) < 2 ** 47 and 416 <= t["ld"] < 2 ** 30 and 416 <= t["cd"] < 2 ** 30
                    worst["pre"], worst["num"] = max(worst["pre"], pre), max(worst["num"], abs(t["ln"]), abs(t["cn"]))
                    n += 1
    print("%d windows; largest term before the shifts 2^%.2f, largest shifted numerator 2^%.2f" % (n, np.log2(worst["pre"]), np.log2(worst["num"])))
    assert n > 190000


def test_distance_from_the_floating_point_ssim():
    worst = 0.0
    for c in S.ALL:
        for pic in S.oracle_run(c):
            for plane in range(3):
                if pic.rec.q[plane].size:
                    worst = max(worst, float(np.abs(pic.rec.q[plane] / 65536.0 - S.float_ssim(pic.rec.sums[plane])).max()))
    print("largest |q / 65536 - float SSIM| = %.3g" % worst)
    assert worst < 2.0 ** -14


def test_an_i_pcm_picture_is_65536_in_every_window():
    for p in S.oracle_run(q.PCM):
        assert all((x == 65536).all() for x in p.rec.q) and p.rec.sum == tuple(65536 * n for n in p.rec.windows)
        assert p.sse.sse == (0, 0, 0)
        # (a 48-sample axis has origins 0 .. 40: four in each of the first two macroblocks, three in the last)
        assert np.array_equal(p.rec.map, 65536 * np.outer([4, 4, 3], [4, 4, 3]))


def test_two_band_instances_lose_exactly_the_straddling_windows():
    c = q.SLICES
    one, two = S.oracle_run(c), S.oracle_bands(c, 2)
    bands = [q.band_rows(c.h, c.slices, r, 2) for r in range(2)]
    assert bands == [(0, 3), (3, 2)]
    lost = []
    for p, b in ((0, 16), (1, 8), (2, 8)):
        pw, ph = (c.w, c.h) if p == 0 else (c.w // 2, c.h // 2)
        edge = b * bands[1][0]
        rows = [y for y in range(0, ph, 4) if y + 8 <= ph and y < edge < y + 8]     # origin above the edge, last row below it
        lost.append((rows, len(rows) * (pw // 4 - 1)))
    assert [n for _, n in lost] == [23, 11, 11]
    for i, (p, (au, recs)) in enumerate(zip(one, two)):
        assert au == p.au, "picture %d: the bands' access unit" % i
        for plane in range(3):
            assert recs[0].rec.windows[plane] + recs[1].rec.windows[plane] == p.rec.windows[plane] - lost[plane][1], (i, plane)
            gone = sum(int(p.rec.q[plane][y // 4].sum()) for y in lost[plane][0])
            assert recs[0].rec.sum[plane] + recs[1].rec.sum[plane] == p.rec.sum[plane] - gone, (i, plane)
            assert gone > 0
        assert not recs[0].rec.map[3:].any() and not recs[1].rec.map[:3].any()
        assert recs[0].rec.map[:3].any() and recs[1].rec.map[3:].any()
        # the windows a band keeps are the single instance's: the map differs only in the macroblock row above the edge
        both = recs[0].rec.map.astype(np.int64) + recs[1].rec.map
        assert np.array_equal(both[[0, 1, 3, 4]], p.rec.map[[0, 1, 3, 4]]) and not np.array_equal(both[2], p.rec.map[2])


def test_the_list_holds_negative_windows():
    """the floor of a negative quotient and the arithmetic shift of a negative product are exercised: measured on the oracle"""
    neg = [[int((x < 0).sum()) for x in p.rec.q] for p in S.oracle_run(S.NOISE51)]
    print("noise 64x48 at QP 51: windows with q < 0 per picture (Y, U, V):", neg)
    assert len(neg) == 3 and all(1 <= n[0] <= 2 for n in neg)
    big = S.oracle_run(q.BIG)[0].rec
    assert int((big.q[0] < 0).sum()) == 1093
    for c in S.ALL:
        if c.qp <= 46:
            assert not any((x < 0).any() for p in S.oracle_run(c) for x in p.rec.q), c.name


def test_lockstep_and_hub_items_are_distinct():
    gops = S.oracle_gops()
    for t in range(q.GOPS[0].pictures):
        for a, b in itertools.combinations(range(len(q.GOPS)), 2):
            assert gops[a][t].rec.sum != gops[b][t].rec.sum and not np.array_equal(gops[a][t].rec.map, gops[b][t].rec.map), (t, a, b)
    b4 = S.oracle_run(q.BATCH4)
    assert len({p.rec.sum for p in b4}) == len(b4)
    hub = [S.oracle_run(c) for c in q.HUB]
    for t in range(q.HUB[0].pictures):
        for a, b in itertools.combinations(range(5), 2):
            assert hub[a][t].rec.sum != hub[b][t].rec.sum and not np.array_equal(hub[a][t].rec.map, hub[b][t].rec.map), (t, a, b)
    k, tick = q.HUB_SITS_OUT
    for t in range(tick + 1, q.HUB[0].pictures):
        assert all(hub[k][t - 1].rec.sum != hub[a][t].rec.sum for a in range(5) if a != k)
    # the SSE records of the same pictures are the ones tests/quality.py computes
    assert all(p.sse.sse == w.rec.sse for c in q.HUB for p, w in zip(S.oracle_run(c), q.oracle_run(c)))
