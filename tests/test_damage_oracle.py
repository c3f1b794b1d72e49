"""What the damage cases of tests/damage.py hold (no GPU): the tile counts and payload bytes they expect follow from the restated
definition in Python integers, the missed-change pictures really compose to something else than the caller's picture, the fallback
boundary is exact, detect equals a brute-force comparison, and the edge cases the GPU tests lean on are really among them."""
import numpy as np
import pytest
import damage as dm

FMTS = [dm.I420, dm.NV12, dm.RGBA]


def test_grid_tile_bytes_and_payload_in_integers():
    assert dm.grid(34, 18) == (1, 2) and dm.grid(66, 34) == (2, 3) and dm.grid(128, 48) == (2, 3) and dm.grid(1920, 1080) == (30, 68)
    assert dm.TILE_BYTES == {dm.I420: 1536, dm.NV12: 1536, dm.RGBA: 4096}
    assert dm.payload_bytes(dm.I420, 0) == 16 and dm.payload_bytes(dm.I420, 1) == 32 + 1536
    assert dm.payload_bytes(dm.RGBA, 4) == 32 + 4 * 4096 and dm.payload_bytes(dm.NV12, 5) == 48 + 5 * 1536
    # 1080p: the bottom row of tiles is half height, and the payload of every tile is larger than the picture
    assert dm.tile_rect(1920, 1080, 67 * 30)[3] == 8
    assert dm.payload_bytes(dm.I420, 30 * 68) > dm.picture_bytes(dm.I420, 1920, 1080)


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("w,h", [(34, 18), (66, 34), (128, 48), (320, 240), (1920, 1080)])
def test_fallback_boundary_is_exact(fmt, w, h):
    n = dm.most_patched_tiles(fmt, w, h)
    ntx, nty = dm.grid(w, h)
    assert dm.payload_bytes(fmt, n) < dm.picture_bytes(fmt, w, h) <= dm.payload_bytes(fmt, n + 1)
    if n:
        assert dm.upload(fmt, w, h, n) == {"bytes": dm.payload_bytes(fmt, n), "tiles": n, "tiles_total": ntx * nty, "mode": "patched"}
    assert dm.upload(fmt, w, h, n + 1)["mode"] == "whole" and dm.upload(fmt, w, h, n + 1)["bytes"] == dm.picture_bytes(fmt, w, h)
    assert dm.upload(fmt, w, h, 0) == {"bytes": 0, "tiles": 0, "tiles_total": ntx * nty, "mode": "nothing"}


def test_rectangles_clip_and_empty_ones_add_nothing():
    assert dm.rect_tiles(66, 34, [(64, 32, 2, 2)]) == {5}
    assert dm.rect_tiles(66, 34, [(63, 15, 2, 2)]) == {0, 1, 2, 3}
    assert dm.rect_tiles(66, 34, [(-9, -9, 3, 3), (70, 0, 5, 5), (5, 5, 0, 9), (5, 5, 9, 0), (0, 34, 66, 4)]) == set()
    assert dm.rect_tiles(66, 34, [(-5, -5, 10000, 10000)]) == set(range(6))
    assert dm.rect_tiles(128, 48, [(64, 16, 64, 16)]) == {3} and dm.rect_tiles(128, 48, [(64, 16, 65, 17)]) == {3, 5}


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("case", dm.CASES, ids=lambda c: c.name)
def test_cases_hold_what_they_claim(case, fmt):
    w, h = case.w, case.h
    ntx, nty = dm.grid(w, h)
    run = dm.run_case(case, fmt)
    assert len(run) >= 6 and len(run) > case.gop, "an IDR picture inside the run"
    seen = {"zero": 0, "corner": 0, "every": 0, "missed": 0, "patched": 0, "whole": 0}
    slot = None
    for i, ((caller, arg, tiles, enc, up), p) in enumerate(zip(run, case.pics)):
        if i == 0:
            assert tiles is None and np.array_equal(enc, caller) and up["mode"] == "whole" and up["bytes"] == dm.picture_bytes(fmt, w, h)
            slot = enc
            continue
        brute = {t for t in range(ntx * nty) if (dm.tile_mask(fmt, w, h, [t]) & (slot != caller)).any()}
        if arg == "detect":
            assert tiles == brute, "detect is the per-byte comparison"
            assert np.array_equal(enc, caller), "with detect the picture that is encoded is the caller's"
        else:
            assert tiles == dm.rect_tiles(w, h, arg)
            if brute - tiles:
                seen["missed"] += 1
                assert not np.array_equal(enc, caller), "a missed change composes to another picture than the caller's"
                assert np.array_equal(enc, dm.compose(fmt, w, h, slot, caller, tiles))
        n = len(tiles)
        assert up["tiles"] == n and up["tiles_total"] == ntx * nty
        pay, pic = ((16 + 4 * n + 15) // 16) * 16 + n * (4096 if fmt == dm.RGBA else 1536), (w * h * 4 if fmt == dm.RGBA else w * h * 3 // 2)
        assert up["bytes"] == (0 if n == 0 else pay if pay < pic else pic)
        assert up["mode"] == ("nothing" if n == 0 else "patched" if pay < pic else "whole")
        seen["zero"] += n == 0
        seen["every"] += n == ntx * nty
        seen["corner"] += tiles == {ntx * nty - 1} and dm.tile_rect(w, h, ntx * nty - 1)[2:] != (64, 16)
        seen[up["mode"]] = seen.get(up["mode"], 0) + 1
        # outside the damaged tiles the picture that is encoded is the slot's previous content, inside it is the caller's
        m = dm.tile_mask(fmt, w, h, tiles)
        assert np.array_equal(enc[m], caller[m]) and np.array_equal(enc[~m], slot[~m])
        slot = enc
    assert seen["zero"] >= 1 and seen["every"] >= 1 and seen["missed"] >= 1
    if (w, h) != (128, 48):
        assert seen["corner"] >= 1, "a single partial corner tile"
    assert seen["nothing"] >= 1 and seen["whole"] >= 1
    # (34x18: one nominal tile is larger than the picture in every layout, so by the fallback rule no call of it ever goes patched)
    assert seen["patched"] >= (0 if (w, h) == (34, 18) else 1)


@pytest.mark.parametrize("fmt", FMTS)
def test_detect_equals_brute_force_on_random_changes(fmt):
    rng = np.random.RandomState(5)
    for (w, h) in [(34, 18), (66, 34), (130, 50)]:
        ntx, nty = dm.grid(w, h)
        prev = dm.content(fmt, w, h, 3)
        for trial in range(12):
            new = prev.copy()
            for _ in range(rng.randint(0, 4)):
                k = rng.randint(0, new.size)
                new[k] = (int(new[k]) + 1 + rng.randint(0, 254)) & 255
            brute = {t for t in range(ntx * nty) if (dm.tile_mask(fmt, w, h, [t]) & (prev != new)).any()}
            assert dm.detect_tiles(fmt, w, h, prev, new) == brute
            assert np.array_equal(dm.compose(fmt, w, h, prev, new, brute), new)
    # the tile masks partition the picture: every byte belongs to exactly one tile
    for (w, h) in [(34, 18), (66, 34)]:
        ntx, nty = dm.grid(w, h)
        assert np.array_equal(sum(dm.tile_mask(fmt, w, h, [t]).astype(int) for t in range(ntx * nty)), np.ones(dm.picture_bytes(fmt, w, h), int))
