"""Damage tiles (include/mi355x_h264.h "damage tiles"; media_amd/csrc/damage.h, k_patch.h), restated in numpy and Python integers,
and the cases the damage tests run.

Grid: tiles of 64 x 16 luma samples at multiples of (64, 16) over the source picture; tile index = ty * tiles_x + tx; partial at the
right and bottom edge.  A tile's bytes at its full nominal size: I420 64 x 16 Y + 32 x 8 U + 32 x 8 V = 1536; NV12 64 x 16 Y + 64 x 8
interleaved = 1536; RGBA 64 x 16 x 4 = 4096.
Damage set: rectangles {x, y, w, h} -> every tile a rectangle touches after clipping; detect -> every tile with a byte inside the
picture that differs from the previous picture.
The picture that is encoded: the previous picture with the damaged tiles replaced from the caller's picture.
Payload = ((16 + 4 * tiles + 15) & ~15) + tiles * tile bytes; the call goes patched when 0 < payload < picture bytes, whole when
payload >= picture bytes, and nothing goes when no tile is damaged.  With an invalid slot (first picture, after a device-form call,
after a failure) the call is an ordinary whole upload of the caller's picture and every tile counts as damaged.

Pictures here are flat uint8 arrays in the stream's layout: I420 (Y, U, V), NV12 (Y, UV) or RGBA (h * w * 4)."""
from collections import namedtuple
import numpy as np

I420, NV12, RGBA = 0, 1, 2
TILE_W, TILE_H, HEADER = 64, 16, 16
TILE_BYTES = {I420: 64 * 16 + 2 * 32 * 8, NV12: 64 * 16 + 64 * 8, RGBA: 64 * 16 * 4}


def grid(w, h):
    return (w + TILE_W - 1) // TILE_W, (h + TILE_H - 1) // TILE_H


def picture_bytes(fmt, w, h):
    return w * h * 4 if fmt == RGBA else w * h * 3 // 2


def payload_bytes(fmt, ntiles):
    return ((HEADER + 4 * ntiles + 15) & ~15) + ntiles * TILE_BYTES[fmt]


def mode_of(fmt, w, h, ntiles):
    if ntiles == 0:
        return "nothing"
    return "patched" if payload_bytes(fmt, ntiles) < picture_bytes(fmt, w, h) else "whole"


def upload(fmt, w, h, ntiles, valid=True):
    """what last_upload reports for a damage call with `ntiles` damaged tiles on a slot that is valid or not"""
    ntx, nty = grid(w, h)
    if not valid:
        return {"bytes": picture_bytes(fmt, w, h), "tiles": ntx * nty, "tiles_total": ntx * nty, "mode": "whole"}
    m = mode_of(fmt, w, h, ntiles)
    b = {"nothing": 0, "patched": payload_bytes(fmt, ntiles), "whole": picture_bytes(fmt, w, h)}[m]
    return {"bytes": b, "tiles": ntiles, "tiles_total": ntx * nty, "mode": m}


def most_patched_tiles(fmt, w, h):
    """the largest number of tiles that still goes patched (the fallback boundary: one more goes whole)"""
    n = 0
    while payload_bytes(fmt, n + 1) < picture_bytes(fmt, w, h):
        n += 1
    return n


def rect_tiles(w, h, rects):
    """the set of tile indices the rectangles touch after clipping"""
    ntx, _ = grid(w, h)
    out = set()
    for (x, y, rw, rh) in rects:
        assert rw >= 0 and rh >= 0
        xa, ya, xb, yb = max(x, 0), max(y, 0), min(x + rw, w), min(y + rh, h)
        if xa >= xb or ya >= yb:
            continue
        for ty in range(ya // TILE_H, (yb - 1) // TILE_H + 1):
            for tx in range(xa // TILE_W, (xb - 1) // TILE_W + 1):
                out.add(ty * ntx + tx)
    return out


def tile_rect(w, h, t):
    """tile t as a rectangle inside the picture"""
    ntx, _ = grid(w, h)
    x, y = (t % ntx) * TILE_W, (t // ntx) * TILE_H
    return (x, y, min(TILE_W, w - x), min(TILE_H, h - y))


def planes(fmt, pic, w, h):
    """views of the flat picture, one per plane, as (rows, bytes per row) arrays, and per plane how many bytes a luma sample column
    takes and by how much rows are subsampled: [(view, bytes per luma column numerator, denominator, row divisor)]"""
    if fmt == RGBA:
        return [(pic.reshape(h, w * 4), 4, 1, 1)]
    y = pic[: w * h].reshape(h, w)
    if fmt == NV12:
        return [(y, 1, 1, 1), (pic[w * h:].reshape(h // 2, w), 1, 1, 2)]
    c = w * h // 4
    return [(y, 1, 1, 1), (pic[w * h: w * h + c].reshape(h // 2, w // 2), 1, 2, 2), (pic[w * h + c:].reshape(h // 2, w // 2), 1, 2, 2)]


def tile_mask(fmt, w, h, tiles):
    """a flat bool array over the picture's bytes: True where the byte belongs to one of the tiles"""
    mask = np.zeros(picture_bytes(fmt, w, h), bool)
    for t in tiles:
        x, y, tw, th = tile_rect(w, h, t)
        for view, num, den, rdiv in planes(fmt, mask, w, h):
            view[y // rdiv: (y + th) // rdiv, x * num // den: (x + tw) * num // den] = True
    return mask


def compose(fmt, w, h, prev, new, tiles):
    """the picture that is encoded: prev with the tiles replaced from new"""
    return np.where(tile_mask(fmt, w, h, tiles), new, prev).astype(np.uint8)


def detect_tiles(fmt, w, h, prev, new):
    """every tile with a byte that differs, found byte by byte: the differing bytes' tiles through a per-byte tile index map"""
    idx = np.zeros(picture_bytes(fmt, w, h), np.int64)
    ntx, nty = grid(w, h)
    for view, num, den, rdiv in planes(fmt, idx, w, h):
        rows, cols = view.shape
        ty = (np.arange(rows) * rdiv) // TILE_H
        tx = (np.arange(cols) * den // num) // TILE_W
        view[:, :] = ty[:, None] * ntx + tx[None, :]
    return set(int(t) for t in np.unique(idx[prev != new]))


def to_layout(fmt, i420, w, h, seed=0):
    """an I420 picture in the layout fmt (RGBA: any RGBA picture made from it will do, alpha is noise)"""
    if fmt == I420:
        return np.ascontiguousarray(i420)
    y, u, v = i420[: w * h], i420[w * h: w * h * 5 // 4], i420[w * h * 5 // 4:]
    if fmt == NV12:
        return np.concatenate([y, np.stack([u, v], axis=1).reshape(-1)])
    Y = y.reshape(h, w).astype(np.int32)
    U = u.reshape(h // 2, w // 2).repeat(2, 0).repeat(2, 1).astype(np.int32)
    V = v.reshape(h // 2, w // 2).repeat(2, 0).repeat(2, 1).astype(np.int32)
    r = np.clip(Y + ((359 * (V - 128)) >> 8), 0, 255)
    g = np.clip(Y - ((88 * (U - 128) + 183 * (V - 128)) >> 8), 0, 255)
    b = np.clip(Y + ((454 * (U - 128)) >> 8), 0, 255)
    a = np.random.RandomState(1000 + seed).randint(0, 256, (h, w))
    return np.stack([r, g, b, a], axis=2).astype(np.uint8).reshape(-1)


def nv12_to_i420(p, w, h):
    uv = p[w * h:].reshape(-1, 2)
    return np.concatenate([p[: w * h], uv[:, 0], uv[:, 1]])


# ---- the cases: a GOP of pictures per size.  Every picture after the first is the one before it with the bytes inside `change`
# rectangles replaced by new content; `say` is what the caller tells the library: "detect", "all" (the change rectangles), or a list of
# rectangles of its own (a missed change when they leave a changed tile out).  Sizes: 34x18 (grid 1 x 2, both tiles partial, w % 4 ==
# 2; one nominal tile is larger than the picture, so nothing of it ever goes patched), 34x66 (1 x 5, all partial, w % 4 == 2),
# 66x34 (2 x 3, partial right and bottom, w % 4 == 2), 128x48 (no partial tile).
Pic = namedtuple("Pic", "change say")
Case = namedtuple("Case", "name w h gop pics")

FULL = (-5, -5, 10000, 10000)
CASES = [
    Case("tiny_34x18", 34, 18, 4, [
        Pic([FULL], "all"),                              # first picture: whole whatever is said
        Pic([(33, 17, 1, 1)], "detect"),                 # one byte in the partial corner tile
        Pic([], "all"),                                  # nothing changed: zero tiles
        Pic([(0, 0, 34, 18)], "detect"),                 # every tile: falls back to whole
        Pic([(2, 3, 7, 2)], "all"),                      # an IDR picture (gop 4) from a patch
        Pic([(0, 0, 10, 18)], [(0, 0, 10, 10)]),         # missed change: tile 1 changed, only tile 0 said
        Pic([(30, 16, 4, 2)], "detect"),
    ]),
    Case("edge_66x34", 66, 34, 5, [
        Pic([FULL], "detect"),
        Pic([(64, 32, 2, 2)], "all"),                    # the single partial corner tile (2 x 2 samples of it)
        Pic([(60, 10, 8, 10)], "detect"),                # four tiles around a tile corner
        Pic([], "detect"),                               # zero tiles, found by comparing
        Pic([(0, 0, 66, 34)], "all"),                    # every tile
        Pic([(10, 20, 50, 4), (65, 0, 1, 1)], [(10, 20, 50, 4), (-9, -9, 3, 3), (70, 0, 5, 5), (5, 5, 0, 9)]),   # missed + empty + outside
        Pic([(0, 33, 66, 1)], "detect"),                 # the bottom row of samples: the partial bottom tiles
    ]),
    Case("tall_34x66", 34, 66, 4, [                        # grid 1 x 5: every tile partial in width, the last one in height too
        Pic([FULL], "detect"),
        Pic([(33, 65, 1, 1)], "detect"),                 # the partial corner tile alone
        Pic([(0, 15, 34, 2)], "all"),                    # two tiles: the most that goes patched
        Pic([(0, 0, 34, 66)], "all"),                    # every tile
        Pic([], "detect"),
        Pic([(0, 30, 34, 20)], [(0, 40, 3, 3)]),         # missed change: tiles 1 and 3 changed, tile 2 said
        Pic([(20, 20, 4, 30)], "detect"),
    ]),
    Case("full_128x48", 128, 48, 3, [
        Pic([FULL], "all"),
        Pic([(64, 16, 64, 16)], "all"),                  # exactly one whole tile
        Pic([(63, 15, 2, 2)], "detect"),                 # four tiles
        Pic([(0, 0, 128, 48)], "detect"),                # every tile
        Pic([], "all"),
        Pic([(0, 0, 128, 16)], [(64, 0, 64, 16)]),       # missed change
    ]),
]
BY_NAME = {c.name: c for c in CASES}


def content(fmt, w, h, seed):
    """a picture of smooth content with noise on top, in the layout"""
    rng = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    y = ((xx * 3 + yy * 5 + seed * 11) % 200 + 20 + rng.randint(0, 12, (h, w))).astype(np.uint8)
    u = ((xx[::2, ::2] + seed * 7) % 120 + 60 + rng.randint(0, 6, (h // 2, w // 2))).astype(np.uint8)
    v = ((yy[::2, ::2] * 2 + seed * 3) % 120 + 60 + rng.randint(0, 6, (h // 2, w // 2))).astype(np.uint8)
    return to_layout(fmt, np.concatenate([y.ravel(), u.ravel(), v.ravel()]), w, h, seed)


def rect_mask(fmt, w, h, rects):
    """bytes of the picture that lie inside one of the rectangles (clipped; chroma: the samples the rectangle's luma samples share)"""
    mask = np.zeros(picture_bytes(fmt, w, h), bool)
    for (x, y, rw, rh) in rects:
        xa, ya, xb, yb = max(x, 0), max(y, 0), min(x + rw, w), min(y + rh, h)
        if xa >= xb or ya >= yb:
            continue
        for view, num, den, rdiv in planes(fmt, mask, w, h):
            if den == 1:
                view[ya // rdiv: (yb - 1) // rdiv + 1, xa * num: xb * num] = True
            else:
                view[ya // rdiv: (yb - 1) // rdiv + 1, xa // den: (xb - 1) // den + 1] = True
    return mask


def run_case(case, fmt):
    """per picture: (what the caller hands over, the damage argument, the damage set the library must arrive at, the picture
    that is encoded, what last_upload must say).  The slot is valid from the second picture on."""
    w, h = case.w, case.h
    out, slot, caller = [], None, None
    for i, p in enumerate(case.pics):
        fresh = content(fmt, w, h, 40 + i)
        if caller is None:
            caller = fresh
        else:
            m = rect_mask(fmt, w, h, p.change)
            step = (fresh % 254 + 1).astype(np.uint8)          # 1 .. 254: every byte inside the change really differs from the old one
            caller = np.where(m, caller + step, caller).astype(np.uint8)
        arg = "detect" if p.say == "detect" else list(p.change if p.say == "all" else p.say)
        if slot is None:
            tiles, enc, up = None, caller.copy(), upload(fmt, w, h, 0, valid=False)
        else:
            tiles = detect_tiles(fmt, w, h, slot, caller) if arg == "detect" else rect_tiles(w, h, arg)
            enc = compose(fmt, w, h, slot, caller, tiles)
            up = upload(fmt, w, h, len(tiles))
        out.append((caller.copy(), arg, tiles, enc, up))
        slot = enc
    return out
