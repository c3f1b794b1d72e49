"""Colour description (include/mi355x_h264.h "colour description", include/mi355x_h264_dec.h "colour"): what the CPU tests
(tests/test_colour_oracle.py, test_colour_host.py, test_colour_parser.py) and the GPU tests (tests/test_gpu_colour_*.py) share.

  the two coefficient tables, typed here a second time from the headers' words
  both conversions restated in numpy for all four variants (the pictures come from tests/value_cube.py's generators)
  a writer and a spec-literal reader of a sequence parameter set with VUI: 7.3.2.1.1, E.1.1, E.1.2, Exp-Golomb of 9.1, emulation
    prevention of 7.4.1.1 - plain Python over lists of bits, nothing shared with the library or the oracle
  the case list

Everything is integer arithmetic, a closed formula or a fixed seed; nothing is read from a file."""
import numpy as np

BT709, BT601 = 1, 6   # matrix_coefficients, Table E-5

# (matrix, full_range): the four variants.  The first is what an undescribed stream has always been
VARIANTS = ((BT601, 0), (BT709, 0), (BT601, 1), (BT709, 1))
NAMES = {(BT601, 0): "bt601_limited", (BT709, 0): "bt709_limited", (BT601, 1): "bt601_full", (BT709, 1): "bt709_full"}
WORDS = {(BT601, 0): ("bt601", "limited"), (BT709, 0): ("bt709", "limited"), (BT601, 1): ("bt601", "full"), (BT709, 1): ("bt709", "full")}
DEFAULT = (BT601, 0)
NEW = tuple(v for v in VARIANTS if v != DEFAULT)

# the way in: Y = ((a R + b G + c B + 128) >> 8) + o, Cb / Cr = ((d r + e g + f b + 128) >> 8) + 128, clipped to 0..255
IN = {
    (BT601, 0): {"y": (66, 129, 25, 16), "cb": (-38, -74, 112), "cr": (112, -94, -18)},
    (BT709, 0): {"y": (47, 157, 16, 16), "cb": (-26, -86, 112), "cr": (112, -102, -10)},
    (BT601, 1): {"y": (77, 150, 29, 0), "cb": (-43, -85, 128), "cr": (128, -107, -21)},
    (BT709, 1): {"y": (54, 183, 19, 0), "cb": (-29, -99, 128), "cr": (128, -116, -12)},
}
# the way out: c = m (Y - o), d = U - 128, e = V - 128, R = clip255((c + rv e + 128) >> 8), G = clip255((c + gu d + gv e + 128) >> 8),
# B = clip255((c + bu d + 128) >> 8)
OUT = {
    (BT601, 0): {"m": 298, "o": 16, "rv": 409, "gu": -100, "gv": -208, "bu": 516},
    (BT709, 0): {"m": 298, "o": 16, "rv": 459, "gu": -55, "gv": -136, "bu": 541},
    (BT601, 1): {"m": 256, "o": 0, "rv": 359, "gu": -88, "gv": -183, "bu": 454},
    (BT709, 1): {"m": 256, "o": 0, "rv": 403, "gu": -48, "gv": -120, "bu": 475},
}


def variant_of(matrix, full_range):
    """the variant RGBA output applies to a stream that says (matrix, full_range): 1 is BT.709, 5 and 6 have the BT.601 numbers,
    every other code (and a stream that says nothing: matrix None) is BT.601 limited"""
    if matrix == 1:
        return (BT709, int(bool(full_range)))
    if matrix in (5, 6):
        return (BT601, int(bool(full_range)))
    return DEFAULT


def colour_word(variant):
    """mi355x_h264_dec_out_pic.colour of a picture the variant was applied to"""
    return variant[0] | (variant[1] << 8)


# ---- the conversions.  The shift of a negative sum is the arithmetic one, the floor of the division by 256: written as that ----
def luma_raw(R, G, B, variant):
    a, b, c, o = IN[variant]["y"]
    return np.floor_divide(a * R + b * G + c * B + 128, 256) + o


def chroma_raw(r, g, b, variant):
    """(Cb, Cr) before the clip, from block means"""
    out = []
    for key in ("cb", "cr"):
        d, e, f = IN[variant][key]
        out.append(np.floor_divide(d * r + e * g + f * b + 128, 256) + 128)
    return out


def block_means(rgba):
    p = np.asarray(rgba).astype(np.int64)
    h, w = p.shape[:2]
    return [np.floor_divide(p[..., c].reshape(h // 2, 2, w // 2, 2).sum(axis=(1, 3)) + 2, 4) for c in range(3)]


def rgba_to_i420(rgba, variant):
    """rgba (h, w, 4) uint8 -> tight I420, flat uint8, by the variant's formula"""
    p = np.asarray(rgba).astype(np.int64)
    y = luma_raw(p[..., 0], p[..., 1], p[..., 2], variant)
    cb, cr = chroma_raw(*block_means(rgba), variant)
    return np.concatenate([np.clip(a, 0, 255).astype(np.uint8).ravel() for a in (y, cb, cr)])


def rgb_raw(y, u, v, variant):
    """(R, G, B) before the clip, int64 arrays"""
    k = OUT[variant]
    y, u, v = (np.asarray(a).astype(np.int64) for a in (y, u, v))
    c, d, e = k["m"] * (y - k["o"]), u - 128, v - 128
    return (np.floor_divide(c + k["rv"] * e + 128, 256), np.floor_divide(c + k["gu"] * d + k["gv"] * e + 128, 256),
            np.floor_divide(c + k["bu"] * d + 128, 256))


def rgb_from_yuv(y, u, v, variant):
    """(R, G, B) uint8 of samples that already lie one to one (4:4:4)"""
    return tuple(np.clip(a, 0, 255).astype(np.uint8) for a in rgb_raw(y, u, v, variant))


def rgba_picture(y, u, v, variant):
    """the RGBA picture (h, w, 4) of I420 planes: the chroma sample of a 2x2 block serves its four pixels, A = 255"""
    up = lambda p: np.repeat(np.repeat(p, 2, axis=0), 2, axis=1)
    r, g, b = rgb_from_yuv(y, up(u), up(v), variant)
    return np.stack([r, g, b, np.full_like(r, 255)], axis=-1)


def planes(i420, w, h):
    a = np.asarray(i420)
    return a[:w * h].reshape(h, w), a[w * h:w * h * 5 // 4].reshape(h // 2, w // 2), a[w * h * 5 // 4:].reshape(h // 2, w // 2)


# ---- bits ----
class BitWriter:
    def __init__(self):
        self.b = []

    def u(self, n, v):
        assert 0 <= v < (1 << n)
        self.b += [(v >> (n - 1 - i)) & 1 for i in range(n)]
        return self

    def ue(self, v):
        n = (v + 1).bit_length()
        return self.u(n - 1, 0).u(n, v + 1)

    def rbsp(self, trailing=True):
        """the bits as bytes, behind rbsp_trailing_bits (a 1, then zeros to the byte)"""
        b = list(self.b) + ([1] if trailing else [])
        b += [0] * (-len(b) % 8)
        return bytes(int("".join(map(str, b[i:i + 8])), 2) for i in range(0, len(b), 8))


def escape(rbsp):
    """7.4.1.1: emulation_prevention_three_byte in front of every byte <= 3 that follows two zero bytes"""
    out, zeros = bytearray(), 0
    for x in rbsp:
        if zeros == 2 and x <= 3:
            out.append(3)
            zeros = 0
        out.append(x)
        zeros = zeros + 1 if x == 0 else 0
    return bytes(out)


def unescape(nal):
    """the inverse: (rbsp, number of emulation prevention bytes removed)"""
    out, zeros, removed = bytearray(), 0, 0
    for x in nal:
        if zeros >= 2 and x == 3:
            zeros, removed = 0, removed + 1
            continue
        out.append(x)
        zeros = zeros + 1 if x == 0 else 0
    return bytes(out), removed


class BitReader:
    def __init__(self, rbsp):
        self.b = [(x >> (7 - i)) & 1 for x in rbsp for i in range(8)]
        self.at = 0
        last = max(i for i, bit in enumerate(self.b) if bit)   # the stop bit of rbsp_trailing_bits
        self.stop = last

    def u(self, n):
        assert self.at + n <= self.stop, "read past the payload"
        v = 0
        for _ in range(n):
            v = (v << 1) | self.b[self.at]
            self.at += 1
        return v

    def ue(self):
        z = 0
        while self.u(1) == 0:
            z += 1
            assert z < 32, "no Exp-Golomb code of this syntax has 32 leading zeros (9.1)"
        return (1 << z) - 1 + (self.u(z) if z else 0)

    def se(self):
        k = self.ue()
        return (k + 1) // 2 if k & 1 else -(k // 2)

    def more(self):
        return self.at < self.stop


def split_nals(stream):
    """the NAL units of an Annex-B byte string, start codes removed"""
    s, out, i, n = bytes(stream), [], 0, len(stream)
    starts = []
    while i + 2 < n:
        if s[i] == 0 and s[i + 1] == 0 and s[i + 2] == 1:
            starts.append((i - 1 if i > 0 and s[i - 1] == 0 else i, i + 3))
            i += 3
        else:
            i += 1
    for k, (_, a) in enumerate(starts):
        out.append(s[a:starts[k + 1][0] if k + 1 < len(starts) else n])
    return out


# ---- E.1.2 / E.1.1 / 7.3.2.1.1, field by field; a dict in, the same dict out ----
def write_hrd(b, h):
    b.ue(len(h["cpb"]) - 1).u(4, h["bit_rate_scale"]).u(4, h["cpb_size_scale"])
    for bit_rate, cpb_size, cbr in h["cpb"]:
        b.ue(bit_rate).ue(cpb_size).u(1, cbr)
    for v in h["lengths"]:   # initial_cpb_removal_delay_length_minus1, cpb_removal_delay_length_minus1, dpb_output_delay_length_minus1, time_offset_length
        b.u(5, v)


def read_hrd(r):
    n = r.ue() + 1
    h = {"bit_rate_scale": r.u(4), "cpb_size_scale": r.u(4), "cpb": []}
    for _ in range(n):
        h["cpb"].append((r.ue(), r.ue(), r.u(1)))
    h["lengths"] = tuple(r.u(5) for _ in range(4))
    return h


VUI_KEYS = ("aspect_ratio", "overscan", "signal", "chroma_loc", "timing", "nal_hrd", "vcl_hrd", "low_delay_hrd", "pic_struct", "restriction")


def write_vui(b, v):
    """v: aspect_ratio None | idc | (255, sar_width, sar_height); overscan None | 0 | 1; signal None | dict(video_format, full_range,
    colour None | (primaries, transfer, matrix)); chroma_loc None | (top, bottom); timing None | (num_units_in_tick, time_scale,
    fixed_frame_rate_flag); nal_hrd / vcl_hrd None | hrd dict; low_delay_hrd (with an HRD); pic_struct 0 | 1; restriction None |
    (mv over boundaries, max_bytes_per_pic_denom, max_bits_per_mb_denom, log2 mv horizontal, vertical, reorder, dec buffering)"""
    ar = v.get("aspect_ratio")
    b.u(1, int(ar is not None))
    if ar is not None:
        if isinstance(ar, tuple):
            b.u(8, ar[0]).u(16, ar[1]).u(16, ar[2])
        else:
            b.u(8, ar)
    b.u(1, int(v.get("overscan") is not None))
    if v.get("overscan") is not None:
        b.u(1, v["overscan"])
    s = v.get("signal")
    b.u(1, int(s is not None))
    if s is not None:
        b.u(3, s["video_format"]).u(1, s["full_range"]).u(1, int(s.get("colour") is not None))
        if s.get("colour") is not None:
            for x in s["colour"]:
                b.u(8, x)
    b.u(1, int(v.get("chroma_loc") is not None))
    if v.get("chroma_loc") is not None:
        b.ue(v["chroma_loc"][0]).ue(v["chroma_loc"][1])
    t = v.get("timing")
    b.u(1, int(t is not None))
    if t is not None:
        b.u(32, t[0]).u(32, t[1]).u(1, t[2])
    for key in ("nal_hrd", "vcl_hrd"):
        b.u(1, int(v.get(key) is not None))
        if v.get(key) is not None:
            write_hrd(b, v[key])
    if v.get("nal_hrd") is not None or v.get("vcl_hrd") is not None:
        b.u(1, v.get("low_delay_hrd", 0))
    b.u(1, v.get("pic_struct", 0))
    rs = v.get("restriction")
    b.u(1, int(rs is not None))
    if rs is not None:
        b.u(1, rs[0])
        for x in rs[1:]:
            b.ue(x)
    return b


def read_vui(r):
    v = {}
    if r.u(1):
        idc = r.u(8)
        v["aspect_ratio"] = (idc, r.u(16), r.u(16)) if idc == 255 else idc
    if r.u(1):
        v["overscan"] = r.u(1)
    if r.u(1):
        s = {"video_format": r.u(3), "full_range": r.u(1)}
        if r.u(1):
            s["colour"] = (r.u(8), r.u(8), r.u(8))
        v["signal"] = s
    if r.u(1):
        v["chroma_loc"] = (r.ue(), r.ue())
    if r.u(1):
        v["timing"] = (r.u(32), r.u(32), r.u(1))
    nal = r.u(1)
    if nal:
        v["nal_hrd"] = read_hrd(r)
    vcl = r.u(1)
    if vcl:
        v["vcl_hrd"] = read_hrd(r)
    if nal or vcl:
        v["low_delay_hrd"] = r.u(1)
    v["pic_struct"] = r.u(1)
    if r.u(1):
        v["restriction"] = (r.u(1),) + tuple(r.ue() for _ in range(6))
    return v


def write_sps_bits(b, s):
    """seq_parameter_set_data() of 7.3.2.1.1 without the NAL header: s has profile_idc, constraints, level_idc, id,
    log2_max_frame_num_minus4, poc_type (0 with log2_max_poc_lsb_minus4, or 2), max_refs, mbw, mbh, crop None | (left, right, top,
    bottom) in units of two samples, vui None | dict"""
    b.u(8, s["profile_idc"]).u(8, s["constraints"]).u(8, s["level_idc"]).ue(s.get("id", 0))
    if s["profile_idc"] == 100:
        b.ue(1).ue(0).ue(0).u(1, 0).u(1, 0)   # chroma_format_idc, bit depths, qpprime_y_zero_transform_bypass_flag, no scaling matrices
    b.ue(s["log2_max_frame_num_minus4"]).ue(s["poc_type"])
    if s["poc_type"] == 0:
        b.ue(s["log2_max_poc_lsb_minus4"])
    b.ue(s["max_refs"]).u(1, 0).ue(s["mbw"] - 1).ue(s["mbh"] - 1).u(1, 1).u(1, 1)
    b.u(1, int(s.get("crop") is not None))
    if s.get("crop") is not None:
        for c in s["crop"]:
            b.ue(c)
    b.u(1, int(s.get("vui") is not None))
    if s.get("vui") is not None:
        write_vui(b, s["vui"])
    return b


def sps_nal(s):
    """the NAL unit (header 0x67, escaped payload) of an SPS dict"""
    return b"\x67" + escape(write_sps_bits(BitWriter(), s).rbsp())


def read_sps(nal):
    """a sequence parameter set NAL unit (header byte first) -> (dict as write_sps_bits takes it, emulation prevention bytes seen);
    frame macroblocks, 4:2:0, 8 bits, no scaling matrices, pic_order_cnt_type 0 or 2 - what this project writes and reads"""
    assert nal[0] & 0x1F == 7
    rbsp, removed = unescape(nal[1:])
    r = BitReader(rbsp)
    s = {"profile_idc": r.u(8), "constraints": r.u(8), "level_idc": r.u(8), "id": r.ue()}
    if s["profile_idc"] == 100:
        assert (r.ue(), r.ue(), r.ue(), r.u(1), r.u(1)) == (1, 0, 0, 0, 0)
    s["log2_max_frame_num_minus4"] = r.ue()
    s["poc_type"] = r.ue()
    assert s["poc_type"] in (0, 2)
    if s["poc_type"] == 0:
        s["log2_max_poc_lsb_minus4"] = r.ue()
    s["max_refs"] = r.ue()
    assert r.u(1) == 0   # gaps_in_frame_num_value_allowed_flag
    s["mbw"], s["mbh"] = r.ue() + 1, r.ue() + 1
    assert (r.u(1), r.u(1)) == (1, 1)   # frame_mbs_only_flag, direct_8x8_inference_flag
    s["crop"] = tuple(r.ue() for _ in range(4)) if r.u(1) else None
    s["vui"] = read_vui(r) if r.u(1) else None
    assert not r.more(), "bits left in front of rbsp_trailing_bits"
    return s, removed


ABSENT = {"described": 0, "matrix": 2, "full_range": 0, "primaries": 2, "transfer": 2, "chroma_loc": -1, "fps": 0, "reorder": -1, "vui": 0, "dec_buffering": -1}


def vui_in_range(v):
    """the ranges of E.2.1 a decoder can check without the rest of the stream"""
    if "chroma_loc" in v and max(v["chroma_loc"]) > 5:
        return False
    if "timing" in v and (v["timing"][0] == 0 or v["timing"][1] == 0):
        return False
    for key in ("nal_hrd", "vcl_hrd"):
        if key in v and len(v[key]["cpb"]) > 32:
            return False
    if "restriction" in v:
        _, bytes_denom, bits_denom, lh, lv, reorder, buffering = v["restriction"]
        if bytes_denom > 16 or bits_denom > 16 or lh > 16 or lv > 16 or buffering > 16 or reorder > buffering:
            return False
    return True


def report_of(vui):
    """what mi355x_h264_parser_colour reports for a sequence parameter set with this VUI (a dict of read_vui, or None): a VUI out of
    range counts as absent, all of it"""
    if vui is None or not vui_in_range(vui):
        return dict(ABSENT)
    out = dict(ABSENT, vui=1)
    s = vui.get("signal")
    if s is not None:
        out["full_range"] = s["full_range"]
        if s.get("colour") is not None:
            out["described"] = 1
            out["primaries"], out["transfer"], out["matrix"] = s["colour"]
    if "chroma_loc" in vui:
        out["chroma_loc"] = vui["chroma_loc"][0]
    if "timing" in vui:
        n, t, _ = vui["timing"]
        out["fps"] = min((t + n) // (2 * n), 0x7FFFFFFF)   # time_scale / (2 * num_units_in_tick), rounded
    if "restriction" in vui:
        out["reorder"], out["dec_buffering"] = vui["restriction"][5], vui["restriction"][6]
    return out


def report_in_range(r):
    return (r["described"] in (0, 1) and r["full_range"] in (0, 1) and all(0 <= r[k] <= 255 for k in ("matrix", "primaries", "transfer")) and
            -1 <= r["chroma_loc"] <= 5 and 0 <= r["fps"] <= 0x7FFFFFFF and -1 <= r["reorder"] <= 16 and -1 <= r["dec_buffering"] <= 16 and
            r["reorder"] <= r["dec_buffering"] and r["vui"] in (0, 1))


def expected_vui(variant, rgba_input, fps, nrefs):
    """item 4 of the description: the VUI of a described stream, as read_vui reports it"""
    matrix, full = variant
    prim = 1 if matrix == BT709 else 6
    v = {"signal": {"video_format": 5, "full_range": full, "colour": (prim, prim, matrix)}, "timing": (1, 2 * fps, 1), "pic_struct": 0,
         "restriction": (1, 0, 0, 16, 16, 0, nrefs)}
    if rgba_input:
        v["chroma_loc"] = (1, 1)
    return v


def described_vui(matrix, full_range, **more):
    """a VUI that says (matrix, full_range) with primaries and transfer 2 (unspecified), for the decoder's tests"""
    return dict({"signal": {"video_format": 5, "full_range": full_range, "colour": (2, 2, matrix)}, "pic_struct": 0}, **more)


def pcm_sps(mbw, mbh, vui, crop=None, level_idc=40):
    """the SPS tests/pcm_stream.py writes (Baseline, pic_order_cnt_type 2, one reference frame), with a VUI: spliced in its place"""
    return sps_nal({"profile_idc": 66, "constraints": 0xC0, "level_idc": level_idc, "log2_max_frame_num_minus4": 0, "poc_type": 2, "max_refs": 1,
                    "mbw": mbw, "mbh": mbh, "crop": None if crop is None else tuple(c // 2 for c in crop), "vui": vui})


def replace_sps(au, new_sps_nal):
    """the access unit with its (first) sequence parameter set NAL unit replaced"""
    nals = split_nals(au)
    k = next(i for i, n in enumerate(nals) if n[0] & 0x1F == 7)
    nals[k] = new_sps_nal
    return b"".join(b"\x00\x00\x00\x01" + n for n in nals)


# ---- the case list ----
PROFILES = (66, 77, 100)
REFS = (1, 3)
SPS_SIZES = ((64, 48), (50, 34))          # without and with cropping
STREAM_SIZES = ((50, 34), (178, 98))      # the smallest with cropping, an odd number of macroblock columns and w % 4 == 2
UNKNOWN_MATRICES = (0, 2, 5, 9)           # 5 has the BT.601 numbers; 0, 2 and 9 get BT.601 limited
