"""Both colour conversions over their whole domains (shared by tests/test_value_cube_oracle.py, CPU, and
tests/test_gpu_rgba_cube.py / tests/test_gpu_dec_output_cube.py, GPU): the pictures whose samples enumerate every (R, G, B) and
every (Y, U, V), small pictures of extreme triples for the geometry edges, and the conversion on the way in restated in numpy from
the words of include/mi355x_h264.h alone.  (The way out, include/mi355x_h264_dec.h, is restated in tests/dec_output.py:
rgba_from_yuv, rows_of, pack.)  Everything is a closed formula or a fixed seed; nothing is read from a file.

  RGB luma cube    16 RGBA pictures of 1024x1024: sample (x, y) of picture k is R = x & 255, G = y & 255,
                   B = 16 k + 4 (y >> 8) + (x >> 8): every (R, G, B) exactly once as a SAMPLE (the luma formula's domain)
  RGB chroma cube  64 RGBA pictures of 1024x1024 of constant 2x2 blocks: block (bx, by) of picture k is r = bx & 255, g = by & 255,
                   b = 4 k + 2 (by >> 8) + (bx >> 8): every (r, g, b) exactly once as a BLOCK MEAN (the chroma formulas' domain)
  rounding picture one uniformly random RGBA picture: in the cubes a block's four-sample sum is 0 or 2 mod 4, here all four residues
                   occur in every channel (the rounding of the mean)
  YUV cube         16 I420 pictures of 1024x1024: chroma sample (cx, cy) of picture k is U = cx & 255, V = cy & 255, and with
                   q = 2 (cy >> 8) + (cx >> 8) its four luma samples are 16 k + 4 q + 2 (y & 1) + (x & 1): every (Y, U, V) exactly
                   once as a PIXEL
  edge pictures    every triple over EDGE_VALUES^3 as a whole 2x2 block, in pictures of 18x16, 50x34 and 178x98 (widths % 4 == 2);
                   the blocks left over in the last picture are random samples, half of them 0 or 255"""
import numpy as np

N = 1024                      # side of the cube pictures
LUMA_PICTURES, CHROMA_PICTURES, YUV_PICTURES = 16, 64, 16
EDGE_VALUES = (0, 1, 15, 16, 17, 127, 128, 129, 234, 235, 236, 240, 241, 254, 255)
EDGE_SIZES = ((18, 16), (50, 34), (178, 98))
ROUNDING_SEED = 20240
# how the edge pictures are coded for the decoder: (coded width, coded height, crop left, crop top) - once cropped on the right and
# bottom only, once with left and top offsets of 2 as well.  18x16 with a top offset does not fit a coded height of 16: that one
# variant is coded 32x32
EDGE_CODED = {(18, 16): ((32, 16, 0, 0), (32, 32, 2, 2)), (50, 34): ((64, 48, 0, 0), (64, 48, 2, 2)), (178, 98): ((192, 112, 0, 0), (192, 112, 2, 2))}


def _alpha(seed):
    return np.random.RandomState(seed).randint(0, 256, (N, N)).astype(np.uint8)


def rgb_luma_cube(k):
    """picture k (0 .. 15) of the RGB luma cube: uint8 (1024, 1024, 4)"""
    x, y = np.arange(N)[None, :], np.arange(N)[:, None]
    p = np.empty((N, N, 4), np.uint8)
    p[..., 0] = x & 255
    p[..., 1] = y & 255
    p[..., 2] = 16 * k + 4 * (y >> 8) + (x >> 8)
    p[..., 3] = _alpha(1000 + k)
    return p


def rgb_chroma_cube(k):
    """picture k (0 .. 63) of the RGB chroma cube: uint8 (1024, 1024, 4), every 2x2 block of one colour"""
    bx, by = np.arange(N // 2)[None, :], np.arange(N // 2)[:, None]
    b = np.empty((N // 2, N // 2, 3), np.uint8)
    b[..., 0] = bx & 255
    b[..., 1] = by & 255
    b[..., 2] = 4 * k + 2 * (by >> 8) + (bx >> 8)
    p = np.empty((N, N, 4), np.uint8)
    p[..., :3] = b.repeat(2, 0).repeat(2, 1)
    p[..., 3] = _alpha(2000 + k)
    return p


def rounding_picture():
    return np.random.RandomState(ROUNDING_SEED).randint(0, 256, (N, N, 4)).astype(np.uint8)


def yuv_cube(k):
    """picture k (0 .. 15) of the YUV cube as planes (Y (1024, 1024), U (512, 512), V (512, 512)), uint8"""
    cx, cy = np.arange(N // 2)[None, :], np.arange(N // 2)[:, None]
    u = np.broadcast_to(cx & 255, (N // 2, N // 2)).astype(np.uint8)
    v = np.broadcast_to(cy & 255, (N // 2, N // 2)).astype(np.uint8)
    q = 2 * (cy >> 8) + (cx >> 8)
    x, y = np.arange(N)[None, :], np.arange(N)[:, None]
    lum = (16 * k + 4 * q.repeat(2, 0).repeat(2, 1) + 2 * (y & 1) + (x & 1)).astype(np.uint8)
    return lum, u, v


def i420_of(y, u, v):
    """tight I420 of three planes"""
    return np.concatenate([np.ascontiguousarray(p, dtype=np.uint8).ravel() for p in (y, u, v)])


def _noise(rng, shape):
    """random samples, half of them drawn from {0, 255}"""
    return np.where(rng.randint(0, 2, shape) == 1, 255 * rng.randint(0, 2, shape), rng.randint(0, 256, shape)).astype(np.uint8)


def edge_triples():
    """the 15^3 triples in a fixed shuffled order (every picture gets a mix of them), int array (3375, 3)"""
    v = np.array(EDGE_VALUES)
    t = np.stack(np.meshgrid(v, v, v, indexing="ij"), axis=-1).reshape(-1, 3)
    return t[np.random.RandomState(15).permutation(len(t))]


def edge_blocks(w, h):
    """the triples shared out over pictures of w x h, one per 2x2 block in raster order: [(blocks (h/2, w/2, 3) uint8,
    valid (h/2, w/2) bool)]; blocks that are not valid (the tail of the last picture) are to be filled with noise"""
    t = edge_triples()
    per = (w // 2) * (h // 2)
    out = []
    for at in range(0, len(t), per):
        part = t[at:at + per]
        b = np.zeros((per, 3), np.uint8)
        b[:len(part)] = part
        valid = np.arange(per) < len(part)
        out.append((b.reshape(h // 2, w // 2, 3), valid.reshape(h // 2, w // 2)))
    return out


def edge_rgba(w, h):
    """[RGBA picture (h, w, 4)]: the triples as (R, G, B) of whole blocks; alpha, and every sample of the left-over blocks, noise"""
    out = []
    for i, (b, valid) in enumerate(edge_blocks(w, h)):
        rng = np.random.RandomState(3000 + 97 * w + i)
        p = _noise(rng, (h, w, 4))
        full = valid.repeat(2, 0).repeat(2, 1)
        p[..., :3][full] = b.repeat(2, 0).repeat(2, 1)[full]
        out.append(p)
    return out


def edge_yuv(w, h):
    """[(Y (h, w), U, V (h/2, w/2))]: the triples as (Y, U, V) with the block's four luma samples equal; left-over blocks noise"""
    out = []
    for i, (b, valid) in enumerate(edge_blocks(w, h)):
        rng = np.random.RandomState(4000 + 97 * w + i)
        y, u, v = _noise(rng, (h, w)), _noise(rng, (h // 2, w // 2)), _noise(rng, (h // 2, w // 2))
        full = valid.repeat(2, 0).repeat(2, 1)
        y[full] = b[..., 0].repeat(2, 0).repeat(2, 1)[full]
        u[valid] = b[..., 1][valid]
        v[valid] = b[..., 2][valid]
        out.append((y, u, v))
    return out


def embed(planes, cw, ch, left, top, seed):
    """the picture (Y, U, V) placed at (left, top) (even) inside coded-size planes of noise: what a cropped stream carries"""
    y, u, v = planes
    rng = np.random.RandomState(seed)
    Y, U, V = _noise(rng, (ch, cw)), _noise(rng, (ch // 2, cw // 2)), _noise(rng, (ch // 2, cw // 2))
    Y[top:top + y.shape[0], left:left + y.shape[1]] = y
    U[top // 2:top // 2 + u.shape[0], left // 2:left // 2 + u.shape[1]] = u
    V[top // 2:top // 2 + v.shape[0], left // 2:left // 2 + v.shape[1]] = v
    return Y, U, V


# ---- the way in, restated from include/mi355x_h264.h (mi355x_h264_encode_rgba) ----
# "Y = ((66 R + 129 G + 25 B + 128) >> 8) + 16, Cb = ((-38 r - 74 g + 112 b + 128) >> 8) + 128, Cr = ((112 r - 94 g - 18 b + 128) >> 8)
# + 128 with r, g, b the rounded mean of the four samples of a 2x2 block", alpha ignored.  The shift of a negative sum is the
# arithmetic one, which is the floor of the division by 256: written as that here, in 64-bit integers.
def rgba_to_i420(rgba):
    """rgba: (h, w, 4) uint8 -> tight I420, flat uint8"""
    p = np.asarray(rgba).astype(np.int64)
    h, w = p.shape[:2]
    R, G, B = p[..., 0], p[..., 1], p[..., 2]
    y = np.floor_divide(66 * R + 129 * G + 25 * B + 128, 256) + 16
    mean = lambda c: np.floor_divide(c.reshape(h // 2, 2, w // 2, 2).sum(axis=(1, 3)) + 2, 4)
    r, g, b = mean(R), mean(G), mean(B)
    cb = np.floor_divide(-38 * r - 74 * g + 112 * b + 128, 256) + 128
    cr = np.floor_divide(112 * r - 94 * g - 18 * b + 128, 256) + 128
    for a in (y, cb, cr):
        assert a.min() >= 0 and a.max() <= 255
    return i420_of(y, cb, cr)


def explain_i420(got, want, rgba):
    """'' when the I420 pictures are equal; else where the first difference lies and which (R, G, B) went in there"""
    got, want = np.asarray(got).ravel(), np.asarray(want).ravel()
    if got.shape == want.shape and np.array_equal(got, want):
        return ""
    if got.shape != want.shape:
        return "%d bytes where %d are expected" % (got.size, want.size)
    h, w = rgba.shape[:2]
    bad = np.flatnonzero(got != want)
    i = int(bad[0])
    if i < w * h:
        y, x = divmod(i, w)
        return "%d samples differ; first: Y(%d, %d) = %d, expected %d, from (R, G, B) = %s" % (bad.size, x, y, got[i], want[i], tuple(int(c) for c in rgba[y, x, :3]))
    j = i - w * h
    plane, j = ("Cb", j) if j < (w // 2) * (h // 2) else ("Cr", j - (w // 2) * (h // 2))
    by, bx = divmod(j, w // 2)
    blk = rgba[2 * by:2 * by + 2, 2 * bx:2 * bx + 2, :3].reshape(4, 3)
    mean = tuple(int((int(s) + 2) // 4) for s in blk.astype(np.int64).sum(axis=0))
    return "%d samples differ; first: %s(%d, %d) = %d, expected %d, from the block of mean (r, g, b) = %s, samples %s" % (
        bad.size, plane, bx, by, got[i], want[i], mean, blk.tolist())


def explain_rgba(got, want, y, u, v):
    """'' when the RGBA pictures (h, w, 4) are equal; else the first wrong pixel and the (Y, U, V) it was made from"""
    if np.array_equal(got, want):
        return ""
    bad = np.argwhere((got != want).any(axis=-1))
    r, c = (int(t) for t in bad[0])
    return "%d pixels differ; first: (%d, %d) = %s, expected %s, from (Y, U, V) = (%d, %d, %d)" % (
        len(bad), c, r, got[r, c].tolist(), want[r, c].tolist(), y[r, c], u[r // 2, c // 2], v[r // 2, c // 2])
