"""Intra refresh restated (include/mi355x_h264.h, "intra refresh"): the schedule, the two row formulas of a clean band, the recovery
point SEI written spec-literally, the case list and its content.  Shared by tests/test_intra_refresh_oracle.py,
tests/test_intra_refresh_host.py and tests/test_gpu_intra_refresh.py; nothing of the encoder under test is used here.

  p = 1, 2, ... counts the P pictures since the last IDR picture, k = (p - 1) mod n.  Band k of that picture is all intra; bands
  j < k read no reference sample below luma row L = 16 * row_end(k - 1) - 1; bands j > k are unrestricted.
  A partition at luma row y0, height hp, vertical vector vy (quarter samples) reads luma rows up to
  y0 + floor(vy / 4) + hp - 1 (+ 3 when vy % 4 != 0) and chroma rows up to y0 / 2 + floor(vy / 8) + hp / 2 - 1 (+ 1 when vy % 8 != 0)."""
import functools
from collections import namedtuple
import numpy as np

MB_I16, MB_P16, MB_PSKIP, MB_IPCM, MB_I4, MB_P16X8, MB_P8X16, MB_P8X8 = range(8)
INTRA = (MB_I16, MB_IPCM, MB_I4)


# ---------------------------------------------------------------- the schedule

def schedule(n, gop, pictures, forced=(), failed=()):
    """[(idr, p, k)] per picture: an IDR picture first, every gop pictures, where forced, and after a failed picture (which does
    not go out); p restarts at each"""
    out, pos, force = [], 0, True
    for i in range(pictures):
        idr = force or i in forced or pos >= gop
        if idr:
            pos = 0
        out.append((idr, 0 if idr else pos, -1 if idr else (pos - 1) % n))
        force = i in failed
        if not force:
            pos += 1
    return out


def band_rows(mbh, n):
    """[(first row, end row)] of the n bands: ceil(mbh / n) macroblock rows each, the last may be shorter"""
    rows = (mbh + n - 1) // n
    out = [(r, min(mbh, r + rows)) for r in range(0, mbh, rows)]
    assert len(out) == n and all(b - a >= 2 for a, b in out), "the picture does not divide into %d bands of two rows or more" % n
    return out


def last_luma_row(y0, hp, vy):
    return y0 + (vy >> 2) + hp - 1 + (3 if vy % 4 else 0)


def last_chroma_row(y0, hp, vy):
    return y0 // 2 + (vy >> 3) + hp // 2 - 1 + (1 if vy % 8 else 0)


def check_picture(mbinfo, mvq, mbw, mbh, n, k):
    """asserts what a P picture with refresh band k must hold; returns how many clean-band macroblocks read exactly down to row L"""
    bands = band_rows(mbh, n)
    types = mbinfo["type"].reshape(mbh, mbw)
    mv = mvq.reshape(mbh, mbw, 4, 2)
    assert not (types == MB_IPCM).any(), "I_PCM macroblocks"
    a, b = bands[k]
    assert np.isin(types[a:b], INTRA).all(), "band %d is not all intra" % k
    if k == 0:
        return 0
    L = 16 * bands[k - 1][1] - 1
    at = 0
    for my in range(bands[k - 1][1]):
        for mx in range(mbw):
            if types[my, mx] in INTRA:
                continue
            hit = False
            for q in range(4):
                y0, vy = 16 * my + 8 * (q >> 1), int(mv[my, mx, q, 1])
                ll, lc = last_luma_row(y0, 8, vy), last_chroma_row(y0, 8, vy)
                assert ll <= L, "macroblock (%d, %d) quadrant %d: vy %d reads luma row %d > %d" % (mx, my, q, vy, ll, L)
                assert lc <= (L + 1) // 2 - 1, "macroblock (%d, %d) quadrant %d: vy %d reads chroma row %d" % (mx, my, q, vy, lc)
                hit = hit or ll == L
            at += hit
    return at


# ---------------------------------------------------------------- the recovery point SEI, D.1.7 / 7.3.2.3, bit by bit

def _ue(v):
    x = v + 1
    nb = x.bit_length()
    return [0] * (nb - 1) + [(x >> i) & 1 for i in range(nb - 1, -1, -1)]


def _pack(bits):
    assert len(bits) % 8 == 0
    return bytes(int("".join(map(str, bits[i:i + 8])), 2) for i in range(0, len(bits), 8))


def _escape(rbsp):
    out, zeros = bytearray(), 0
    for b in rbsp:
        if zeros == 2 and b <= 3:
            out.append(3)
            zeros = 0
        out.append(b)
        zeros = zeros + 1 if b == 0 else 0
    return bytes(out)


def sei_bytes(n):
    """the SEI NAL unit with its four-byte start code: nal_ref_idc 0, type 6; payloadType 6, payloadSize; recovery_frame_cnt ue(n - 1),
    exact_match_flag 1, broken_link_flag 0, changing_slice_group_idc u(2) 0; the payload's alignment (a one bit, then zero bits);
    rbsp_trailing_bits"""
    pl = _ue(n - 1) + [1] + [0] + [0, 0]
    if len(pl) % 8:
        pl += [1]
        pl += [0] * (-len(pl) % 8)
    payload = _pack(pl)
    rbsp = bytes([6, len(payload)]) + payload + b"\x80"
    return b"\x00\x00\x00\x01\x06" + _escape(rbsp)


def split_nals(au):
    """the NAL units of an access unit (four-byte start codes, as the encoder writes them), without the start codes"""
    parts = bytes(au).split(b"\x00\x00\x00\x01")
    assert parts[0] == b""
    return parts[1:]


# ---------------------------------------------------------------- the cases and their content

Case = namedtuple("Case", "name w h n prof qp pictures search step obj amp", defaults=(85,))
CASES = (
    Case("A_96x128_n4", 96, 128, 4, 66, 27, 14, 1, 3, False),
    Case("B_112x96_n3_seeded", 112, 96, 3, 77, 22, 11, 1, 7, True),
    Case("B_112x96_n3_exhaustive", 112, 96, 3, 77, 22, 11, 0, 3, False),
    Case("C_64x80_n2_high", 64, 80, 2, 100, 26, 8, 1, 3, True),
    Case("D_48x64_n2_qp10", 48, 64, 2, 66, 10, 8, 1, 3, False, 24),   # (a gentler texture: at QP 10 the full one makes I_PCM)
    Case("D_48x64_n2_qp51", 48, 64, 2, 66, 51, 8, 1, 3, False),   # (3 rows: at QP 51 a scroll by 7 left no clean-band vector at the bound)
    Case("E_1920x1080_n8", 1920, 1080, 8, 66, 26, 10, 1, 3, False),
)
BY_NAME = {c.name: c for c in CASES}
SMALL = tuple(c for c in CASES if c.w < 1000)


def cut_of(c):
    """c of the recovery test: the first picture of the second refresh cycle where the case has pictures enough, else of the first"""
    return c.n + 1 if c.pictures >= 2 * c.n + 2 else 1


@functools.lru_cache(maxsize=None)
def _texture(w, rows, seed, amp):
    """a smooth texture (features of 8 to 16 samples, no flat areas), values 40 .. 215: luma, Cb, Cr"""
    rng = np.random.RandomState(seed)

    def plane(pw, ph, cell, amp, mid):
        g = rng.uniform(-1, 1, (ph // cell + 3, pw // cell + 3))
        yy, xx = np.arange(ph) / cell, np.arange(pw) / cell
        y0, x0 = yy.astype(int), xx.astype(int)
        fy, fx = (yy - y0)[:, None], (xx - x0)[None, :]
        fy, fx = fy * fy * (3 - 2 * fy), fx * fx * (3 - 2 * fx)
        a, b = g[y0][:, x0], g[y0][:, x0 + 1]
        c, d = g[y0 + 1][:, x0], g[y0 + 1][:, x0 + 1]
        return np.clip(mid + amp * ((a * (1 - fx) + b * fx) * (1 - fy) + (c * (1 - fx) + d * fx) * fy), 0, 255).astype(np.uint8)
    return plane(w, rows, 12, amp, 128), plane(w // 2, rows // 2, 8, amp * 0.6, 128), plane(w // 2, rows // 2, 8, amp * 0.6, 128)


def _frame(c, i, seed):
    """picture i: the texture scrolled UPWARDS by c.step rows per picture (the best match of a row lies c.step rows further down in
    the previous picture); obj: a bright square that moves down and right across the band boundaries"""
    ty, tu, tv = _texture(c.w, c.h + 2 * ((c.step * c.pictures + 3) // 2) + 16, seed, c.amp)
    o = c.step * i
    oc = o // 2
    y, u, v = ty[o:o + c.h].copy(), tu[oc:oc + c.h // 2].copy(), tv[oc:oc + c.h // 2].copy()
    if c.obj:
        x0, y0 = 4 + 5 * i, 2 + 9 * i
        y[y0:y0 + 20, x0:x0 + 20] = 225
        u[y0 // 2:y0 // 2 + 10, x0 // 2:x0 // 2 + 10] = 90
    return np.concatenate([y.ravel(), u.ravel(), v.ravel()])


@functools.lru_cache(maxsize=None)
def frames(c):
    return tuple(_frame(c, i, 11) for i in range(c.pictures))


@functools.lru_cache(maxsize=None)
def frames_other(c):
    """the second content: another texture before picture cut_of(c), the case's own pictures from there on"""
    cut = cut_of(c)
    return tuple(_frame(c, i, 23) if i < cut else frames(c)[i] for i in range(c.pictures))


def planes_of(frame, w, h):
    y = frame[:w * h].reshape(h, w)
    u = frame[w * h:w * h * 5 // 4].reshape(h // 2, w // 2)
    v = frame[w * h * 5 // 4:].reshape(h // 2, w // 2)
    return y, u, v


def band_differs(a, b, bands, j):
    """planes a and b (luma, Cb, Cr of coded size) differ somewhere in the rows of band j"""
    r0, r1 = bands[j]
    return any(not np.array_equal(pa[(16 if p == 0 else 8) * r0:(16 if p == 0 else 8) * r1], pb[(16 if p == 0 else 8) * r0:(16 if p == 0 else 8) * r1])
               for p, (pa, pb) in enumerate(zip(a, b)))
