"""ctypes binding of oracle/liboracle_h264.so -- the CHECKER, test-side only."""
import ctypes as C
import os
import subprocess
import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_ODIR = os.path.join(os.path.dirname(_HERE), "oracle")
_SO = os.path.join(_ODIR, "liboracle_h264.so")

LV_STRIDE = 416
LV_LUMA_DC, LV_LUMA, LV_CHROMA_DC, LV_CHROMA_AC = 0, 16, 272, 280


class Config(C.Structure):
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("fps", C.c_int32), ("qp", C.c_int32),
                ("gop", C.c_int32), ("profile_idc", C.c_int32), ("disable_deblock", C.c_int32), ("slices", C.c_int32), ("band_index", C.c_int32), ("band_count", C.c_int32), ("refs", C.c_int32), ("search", C.c_int32)]


MBINFO_DTYPE = np.dtype([("mvx", "<i2"), ("mvy", "<i2"), ("type", "u1"), ("i16_mode", "u1"),
                         ("chroma_mode", "u1"), ("cbp", "u1"), ("tc", "u1", (24,))])
assert MBINFO_DTYPE.itemsize == 32


class Hits(C.Structure):
    """h264o_hits: what the oracle's slice data writer has written since the last reset, per syntax element"""
    _fields_ = [("coeff_token", C.c_uint32 * 4 * 17 * 4), ("cdc_token", C.c_uint32 * 4 * 5), ("total_zeros", C.c_uint32 * 16 * 16),
                ("cdc_total_zeros", C.c_uint32 * 4 * 4), ("run_before", C.c_uint32 * 15 * 8), ("suffix_len", C.c_uint32 * 7),
                ("prefix14", C.c_uint32 * 7), ("prefix15", C.c_uint32 * 7), ("mb_kind", C.c_uint32 * 8), ("mb_type", C.c_uint32 * 32 * 2),
                ("cbp_intra", C.c_uint32 * 48), ("cbp_inter", C.c_uint32 * 48), ("i4_mode", C.c_uint32 * 9 * 16),
                ("max_mvd", C.c_uint32), ("max_skip_run", C.c_uint32), ("skip_runs_over_a_row", C.c_uint32),
                ("skip_run_ends_slice", C.c_uint32), ("pcm_after_skip_run", C.c_uint32), ("long_header_slots", C.c_uint32),
                ("long_residual_slots", C.c_uint32),
                # picture level (random_picture with RAND_NONREF / RAND_SLICE_TYPES / RAND_PARAMETER_SETS)
                ("nonref_pics", C.c_uint32), ("nonref_run", C.c_uint32 * 4), ("nonref_before_idr", C.c_uint32), ("nonref_after_idr", C.c_uint32),
                ("slice_shape", C.c_uint32 * 4), ("slice_type_form", C.c_uint32 * 2), ("pps_switches", C.c_uint32), ("pps_resent", C.c_uint32),
                ("pics_no_dbf_ctrl", C.c_uint32), ("pps_id_used", C.c_uint32 * 4), ("sps_id_used", C.c_uint32 * 3), ("crop_lt_streams", C.c_uint32),
                # random_picture with RAND_RANGE_ENDS
                ("re_slice_qp", C.c_uint32 * 52), ("re_prefix15_max", C.c_uint32 * 7), ("re_prefix16", C.c_uint32 * 3), ("re_mv_limit", C.c_uint32 * 4),
                ("re_mvd_over_8192", C.c_uint32), ("re_qpi_below_0", C.c_uint32), ("re_qpi_above_51", C.c_uint32), ("re_dropped", C.c_uint32)]
    MAX_FIELDS = ("max_mvd", "max_skip_run")

    def arrays(self):
        """{field: numpy uint64 array (a copy)}"""
        return {n: np.array(np.ctypeslib.as_array(getattr(self, n)) if not isinstance(getattr(self, n), int) else getattr(self, n), dtype=np.uint64)
                for n, _ in self._fields_}


def _build():
    srcs = [os.path.join(_ODIR, f) for f in os.listdir(_ODIR) if f.endswith((".c", ".h"))]
    if not os.path.exists(_SO) or any(os.path.getmtime(s) > os.path.getmtime(_SO) for s in srcs):
        subprocess.check_call(["make", "-C", _ODIR, "-s"])


_lib = None


def lib():
    global _lib
    if _lib is None:
        _build()
        L = C.CDLL(_SO)
        vp, u8p = C.c_void_p, C.POINTER(C.c_uint8)
        L.h264o_enc_create.restype = vp
        L.h264o_enc_create.argtypes = [C.POINTER(Config)]
        L.h264o_enc_destroy.argtypes = [vp]
        L.h264o_enc_encode.restype = C.c_int64
        L.h264o_enc_encode.argtypes = [vp, vp, C.c_int, vp, C.c_int, vp, C.c_int, C.c_int, vp, C.c_size_t,
                                       C.POINTER(C.c_int)]
        for n in ("h264o_enc_coded_width", "h264o_enc_coded_height"):
            getattr(L, n).argtypes = [vp]
        for n in ("h264o_enc_recon", "h264o_enc_recon_pre"):
            getattr(L, n).restype = vp
            getattr(L, n).argtypes = [vp, C.c_int]
        L.h264o_enc_mbinfo.restype = vp
        L.h264o_enc_mbinfo.argtypes = [vp]
        L.h264o_enc_mbaux.restype = vp
        L.h264o_enc_mvq.restype = vp
        L.h264o_enc_mvq.argtypes = [vp]
        L.h264o_enc_mbaux.argtypes = [vp]
        L.h264o_enc_levels.restype = vp
        L.h264o_enc_levels.argtypes = [vp]
        L.h264o_enc_set_qp.argtypes = [vp, C.c_int]
        L.h264o_enc_last_me_cost.argtypes = [vp]
        L.h264o_enc_last_me_cost.restype = C.c_uint32
        L.h264o_enc_p_decision.restype = vp
        L.h264o_enc_p_decision.argtypes = [vp]
        L.h264o_enc_set_idr_id.argtypes = [vp, C.c_int, C.c_int]
        L.h264o_enc_halo_bytes.argtypes = [vp]
        L.h264o_enc_halo_bytes.restype = C.c_size_t
        L.h264o_enc_halo_export.argtypes = [vp, C.c_int, vp]
        L.h264o_enc_halo_export.restype = None
        L.h264o_enc_halo_import.argtypes = [vp, C.c_int, vp]
        L.h264o_enc_halo_import.restype = None
        L.h264o_enc_random_picture.restype = C.c_int64
        L.h264o_enc_random_picture.argtypes = [vp, C.c_uint32, C.c_int, C.c_int, vp, C.c_size_t, C.POINTER(C.c_int), vp]
        L.h264o_enc_last_slice_bits.restype = C.c_int64
        L.h264o_enc_last_slice_bits.argtypes = [vp]
        L.h264o_enc_slice_bits_all.argtypes = [vp, vp, C.c_int]
        L.h264o_enc_mb_bitpos.restype = vp
        L.h264o_enc_mb_bitpos.argtypes = [vp]
        L.h264o_enc_source.restype = vp
        L.h264o_enc_source.argtypes = [vp, C.c_int]
        L.h264o_enc_hits.restype = C.POINTER(Hits)
        L.h264o_enc_hits.argtypes = [vp]
        L.h264o_enc_hits_reset.restype = None
        L.h264o_enc_hits_reset.argtypes = [vp]
        L.h264o_enc_random_last.restype = None
        L.h264o_enc_random_last.argtypes = [vp, vp]
        L.h264o_dec_create.restype = vp
        L.h264o_dec_destroy.argtypes = [vp]
        L.h264o_dec_decode.argtypes = [vp, vp, C.c_size_t]
        for n in ("h264o_dec_width", "h264o_dec_height", "h264o_dec_coded_width", "h264o_dec_coded_height",
                  "h264o_dec_last_slice_type", "h264o_dec_last_nal_type", "h264o_dec_crop_left", "h264o_dec_crop_top", "h264o_dec_last_is_ref"):
            getattr(L, n).argtypes = [vp]
        L.h264o_dec_plane.restype = vp
        L.h264o_dec_plane.argtypes = [vp, C.c_int]
        L.h264o_dec_error.restype = C.c_char_p
        L.h264o_dec_error.argtypes = [vp]
        for n in ("h264o_dec_max_mb_bits", "h264o_dec_max_level_prefix"):
            getattr(L, n).argtypes = [vp]
        L.h264o_dec_ref_age.argtypes = [vp, C.c_int]
        L.h264o_dec_stat.argtypes = [vp, C.c_int]
        L.h264o_dec_dbf.restype = vp
        L.h264o_dec_dbf.argtypes = [vp]
        L.h264o_dec_pred.restype = vp
        L.h264o_dec_pred.argtypes = [vp]
        L.h264o_dec_mb_kind.argtypes = [vp, C.c_int]
        L.h264o_dec_mb_qp.argtypes = [vp, C.c_int]
        L.h264o_dec_mb_avail.argtypes = [vp, C.c_int]
        L.h264o_dec_mb_intra_mode.argtypes = [vp, C.c_int, C.c_int]
        L.h264o_dec_mb_mv.argtypes = [vp, C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]
        ip, up = C.POINTER(C.c_int), C.POINTER(C.c_uint)
        L.h264o_dec_table_coeff_token.argtypes = [C.c_int, C.c_int, C.c_int, ip, up]
        L.h264o_dec_table_total_zeros.argtypes = [C.c_int, C.c_int, C.c_int, ip, up]
        L.h264o_dec_table_run_before.argtypes = [C.c_int, C.c_int, ip, up]
        L.h264o_dec_table_misc.argtypes = [C.c_int, C.c_int, C.c_int]
        L.h264o_fdct4x4.argtypes = [vp, vp]
        L.h264o_rgba_to_i420.argtypes = [vp, C.c_int, C.c_int, C.c_int, vp]
        L.h264o_rgba_to_i420.restype = None
        L.h264o_idct4x4_add.argtypes = [vp, vp, C.c_int]
        L.h264o_quant4x4.argtypes = [vp, C.c_int, C.c_int, vp]
        L.h264o_dequant4x4.argtypes = [vp, C.c_int, vp]
        L.h264o_mc_luma.argtypes = [vp] + [C.c_int] * 9 + [vp, C.c_int]
        L.h264o_mc_chroma.argtypes = [vp] + [C.c_int] * 9 + [vp, C.c_int]
        L.h264o_luma_sample_ref.argtypes = [vp] + [C.c_int] * 7
        for n in ("h264o_sad16x16", "h264o_satd16x16", "h264o_satd8x8"):
            getattr(L, n).argtypes = [vp, C.c_int, vp, C.c_int]
        L.h264o_pred16x16.argtypes = [vp, C.c_int, C.c_int, C.c_int, vp]
        L.h264o_pred_chroma8x8.argtypes = [vp, C.c_int, C.c_int, C.c_int, vp]
        L.h264o_deblock_picture.argtypes = [vp, vp, vp, C.c_int, C.c_int, vp, vp, C.c_int, vp, C.c_int, C.c_int]
        L.h264o_ue_bits.argtypes = [C.c_uint32, C.POINTER(C.c_uint32)]
        L.h264o_se_bits.argtypes = [C.c_int32, C.POINTER(C.c_uint32)]
        L.h264o_cavlc_block.argtypes = [vp, C.c_int, C.c_int, vp]
        L.h264o_nal_escape.restype = C.c_size_t
        L.h264o_nal_escape.argtypes = [vp, C.c_size_t, vp]
        _lib = L
    return _lib


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def rgba_to_i420(rgba, width, height, stride=None):
    """the oracle's RGBA ingest (oracle/h264_rgba.c): uint8 RGBA rows -> tight I420 as a flat uint8 array"""
    a = np.ascontiguousarray(rgba, dtype=np.uint8)
    out = np.zeros(width * height * 3 // 2, np.uint8)
    lib().h264o_rgba_to_i420(a.ctypes.data, int(stride or 4 * width), width, height, out.ctypes.data)
    return out


class OracleEncoder:
    def __init__(self, width, height, qp=26, gop=30, fps=30, profile_idc=66, disable_deblock=0, slices=0, band_index=0, band_count=0, refs=0, search=1):
        self.cfg = Config(width, height, fps, qp, gop, profile_idc, disable_deblock, slices, band_index, band_count, refs, search)
        self.h = lib().h264o_enc_create(C.byref(self.cfg))
        if not self.h:
            raise ValueError("oracle rejected config")
        self.width, self.height = width, height
        self.cw = lib().h264o_enc_coded_width(self.h)
        self.ch = lib().h264o_enc_coded_height(self.h)
        self.out = np.zeros(width * height * 8 + (1 << 16), dtype=np.uint8)

    def encode(self, i420, force_idr=False):
        w, h = self.width, self.height
        f = np.ascontiguousarray(i420, dtype=np.uint8)
        y, u, v = f[: w * h], f[w * h: w * h * 5 // 4], f[w * h * 5 // 4:]
        idr = C.c_int(0)
        n = lib().h264o_enc_encode(self.h, _ptr(y), w, _ptr(u), w // 2, _ptr(v), w // 2, int(force_idr),
                                   _ptr(self.out), self.out.size, C.byref(idr))
        if n < 0:
            raise RuntimeError("oracle encode failed %d" % n)
        return bytes(self.out[:n]), bool(idr.value)

    RAND_QP, RAND_CHROMA_OFF, RAND_FILTER_OFF, RAND_PCM, RAND_IDC, RAND_SUBPARTS, RAND_SLICES, RAND_REORDER, RAND_OPENH264_HEADERS, RAND_BIG_LEVELS, RAND_CONSTRAINED_INTRA, RAND_ALL = 1, 2, 4, 8, 16, 32, 64, 128, 256, 512, 1024, 2047
    # not part of RAND_ALL (the decoder-peer tests): dense residual blocks; syntax the encoder's entropy stage codes to the same bytes
    # (mi355x_h264_debug_code_syntax); a first slice that outgrows its payload share (refusal path only, not conforming)
    RAND_DENSE, RAND_ENCODER_SHAPED, RAND_SATURATE_FIRST_SLICE = 2048, 4096, 8192
    # picture level: non-reference pictures; I and P slices in any non-IDR picture; several parameter sets, left / top cropping
    RAND_NONREF, RAND_SLICE_TYPES, RAND_PARAMETER_SETS = 16384, 32768, 65536
    # the ends of the QP, level and vector ranges (oracle/h264_oracle.h says what is drawn; tests/range_ends.py holds the cases)
    RAND_RANGE_ENDS = 131072
    # windows of the inter prediction at the picture's edges, many intra macroblocks in P slices (with RAND_SUBPARTS; tests/pred_cells.py)
    RAND_PRED_CELLS = 262144
    SHAPE_ALL_I, SHAPE_I_THEN_P, SHAPE_P_THEN_I, SHAPE_ALL_P = 0, 1, 2, 3

    def random_picture(self, seed, force_idr=False, features=31):
        """one picture of random conforming syntax (h264o_enc_random_picture): (access unit, is_idr, QP_Y per macroblock);
        mbinfo() / mvq() / mbaux() / levels() then hold what was written"""
        idr = C.c_int(0)
        n_mb = (self.cw // 16) * (self.ch // 16)
        mbqp = np.zeros(n_mb, dtype=np.uint8)
        n = lib().h264o_enc_random_picture(self.h, int(seed) & 0xFFFFFFFF, int(force_idr), int(features), _ptr(self.out), self.out.size,
                                           C.byref(idr), _ptr(mbqp))
        if n < 0:
            raise RuntimeError("oracle random picture failed %d" % n)
        return bytes(self.out[:n]), bool(idr.value), mbqp

    def random_last(self):
        """picture level of the last random_picture: is_ref, pps_id, sps_id, crop_left, crop_top (luma samples), pic_init_qp,
        shape (SHAPE_*), deblock_control"""
        a = np.zeros(8, np.int32)
        lib().h264o_enc_random_last(self.h, _ptr(a))
        return dict(zip(("is_ref", "pps_id", "sps_id", "crop_left", "crop_top", "pic_init_qp", "shape", "deblock_control"), (int(v) for v in a)))

    def _plane(self, fn, p):
        cw, ch = (self.cw, self.ch) if p == 0 else (self.cw // 2, self.ch // 2)
        addr = fn(self.h, p)
        return np.ctypeslib.as_array(C.cast(addr, C.POINTER(C.c_uint8)), shape=(ch, cw)).copy()

    def recon(self, p):
        return self._plane(lib().h264o_enc_recon, p)

    def recon_pre(self, p):
        return self._plane(lib().h264o_enc_recon_pre, p)

    def mbinfo(self):
        n = (self.cw // 16) * (self.ch // 16)
        addr = lib().h264o_enc_mbinfo(self.h)
        raw = np.ctypeslib.as_array(C.cast(addr, C.POINTER(C.c_uint8)), shape=(n * 32,)).copy()
        return raw.view(MBINFO_DTYPE)

    def mbaux(self):
        """16 bytes per macroblock: Intra4x4PredMode of the blocks of an Intra4x4 macroblock (blkIdx order)"""
        n = (self.cw // 16) * (self.ch // 16)
        addr = lib().h264o_enc_mbaux(self.h)
        return np.ctypeslib.as_array(C.cast(addr, C.POINTER(C.c_uint8)), shape=(n, 16)).copy()

    def mvq(self):
        """(x, y) vectors of the four 8x8 quadrants of every macroblock (meaningful for inter macroblocks)"""
        n = (self.cw // 16) * (self.ch // 16)
        addr = lib().h264o_enc_mvq(self.h)
        return np.ctypeslib.as_array(C.cast(addr, C.POINTER(C.c_int16)), shape=(n, 8)).copy()

    def levels(self):
        n = (self.cw // 16) * (self.ch // 16)
        addr = lib().h264o_enc_levels(self.h)
        return np.ctypeslib.as_array(C.cast(addr, C.POINTER(C.c_int16)), shape=(n, LV_STRIDE)).copy()

    def set_qp(self, qp):
        if lib().h264o_enc_set_qp(self.h, qp) != 0:
            raise ValueError("bad qp")

    def halo_bytes(self):
        return lib().h264o_enc_halo_bytes(self.h)

    def halo_export(self, edge, ptr):
        lib().h264o_enc_halo_export(self.h, edge, ptr)

    def halo_import(self, edge, ptr):
        lib().h264o_enc_halo_import(self.h, edge, ptr)

    def set_idr_id(self, nxt, step=1):
        lib().h264o_enc_set_idr_id(self.h, nxt, step)

    def me_cost(self):
        return lib().h264o_enc_last_me_cost(self.h)

    P_CODED, P_TO_INTRA, P_SETTLED = 0, 1, 2

    def p_decision(self):
        """per macroblock of the last P picture: P_CODED (searched, coded as an inter macroblock), P_TO_INTRA (searched, handed to
        the intra pass) or P_SETTLED (one of the "nothing left to code" tests: no search, nothing coded)"""
        n = (self.cw // 16) * (self.ch // 16)
        addr = lib().h264o_enc_p_decision(self.h)
        return np.ctypeslib.as_array(C.cast(addr, C.POINTER(C.c_uint8)), shape=(n,)).copy()

    def slice_bits(self):
        """bits of every slice of the last picture, first_mb_in_slice up to and including rbsp_stop_one_bit"""
        a = np.zeros(256, np.int64)
        n = lib().h264o_enc_slice_bits_all(self.h, _ptr(a), a.size)
        return [int(v) for v in a[:n]]

    def last_slice_data_bits(self):
        """bits of slice_data() of the last picture (all its slices), headers and trailing bits not counted"""
        return lib().h264o_enc_last_slice_bits(self.h)

    def mb_bitpos(self):
        """per macroblock of the last picture: the bit of its slice's RBSP at which its syntax starts"""
        n = (self.cw // 16) * (self.ch // 16)
        addr = lib().h264o_enc_mb_bitpos(self.h)
        return np.ctypeslib.as_array(C.cast(addr, C.POINTER(C.c_uint32)), shape=(n,)).copy()

    def source_i420(self):
        """the source picture as a tight display-size I420 array (after random_picture: the samples drawn for I_PCM macroblocks)"""
        w, h = self.width, self.height
        return np.concatenate([self._plane(lib().h264o_enc_source, p)[: (h // 2 if p else h), : (w // 2 if p else w)].ravel() for p in range(3)])

    def hits(self):
        return lib().h264o_enc_hits(self.h).contents.arrays()

    def hits_reset(self):
        lib().h264o_enc_hits_reset(self.h)

    def close(self):
        if self.h:
            lib().h264o_enc_destroy(self.h)
            self.h = None

    def __del__(self):
        self.close()


class OracleDecoder:
    def __init__(self):
        self.h = lib().h264o_dec_create()

    def decode(self, data):
        buf = np.frombuffer(bytes(data), dtype=np.uint8)
        rc = lib().h264o_dec_decode(self.h, _ptr(buf), buf.size)
        if rc < 0:
            raise RuntimeError("decode error: " + lib().h264o_dec_error(self.h).decode())
        return rc

    def plane(self, p):
        cw, ch = lib().h264o_dec_coded_width(self.h), lib().h264o_dec_coded_height(self.h)
        if p:
            cw, ch = cw // 2, ch // 2
        addr = lib().h264o_dec_plane(self.h, p)
        return np.ctypeslib.as_array(C.cast(addr, C.POINTER(C.c_uint8)), shape=(ch, cw)).copy()

    @property
    def size(self):
        return lib().h264o_dec_width(self.h), lib().h264o_dec_height(self.h)

    @property
    def crop(self):
        """(left, top) in luma samples: where the cropped picture of `size` starts inside plane(0)"""
        return lib().h264o_dec_crop_left(self.h), lib().h264o_dec_crop_top(self.h)

    def cropped(self, p):
        """plane p cut to the display size by the decoder's own crop offsets"""
        (w, h), (x, y) = self.size, self.crop
        s = 2 if p else 1
        return self.plane(p)[y // s:(y + h) // s, x // s:(x + w) // s]

    @property
    def last_is_ref(self):
        return bool(lib().h264o_dec_last_is_ref(self.h))

    def ref_ages(self):
        """RefPicList0 of the last P slice: per entry, the number of reference pictures decoded since that one"""
        return tuple(lib().h264o_dec_ref_age(self.h, i) for i in range(3))

    # statistics of the last decoded picture
    KIND_I4, KIND_I16, KIND_IPCM, KIND_INTER, KIND_SKIP = 1, 2, 3, 4, 5

    def mb_kinds(self):
        n = (lib().h264o_dec_coded_width(self.h) // 16) * (lib().h264o_dec_coded_height(self.h) // 16)
        return np.array([lib().h264o_dec_mb_kind(self.h, i) for i in range(n)], dtype=np.int32)

    def mb_qps(self):
        n = (lib().h264o_dec_coded_width(self.h) // 16) * (lib().h264o_dec_coded_height(self.h) // 16)
        return np.array([lib().h264o_dec_mb_qp(self.h, i) for i in range(n)], dtype=np.int32)

    def mb_avail(self):
        """per macroblock: its neighbours left, top, top-right, top-left available (bits 0..3) and available for intra prediction (bits 4..7)"""
        n = (lib().h264o_dec_coded_width(self.h) // 16) * (lib().h264o_dec_coded_height(self.h) // 16)
        return np.array([lib().h264o_dec_mb_avail(self.h, i) for i in range(n)], dtype=np.uint8)

    def mb_intra_modes(self):
        """per macroblock: Intra4x4PredMode of its sixteen 4x4 blocks (raster order), Intra16x16PredMode, intra_chroma_pred_mode"""
        n = (lib().h264o_dec_coded_width(self.h) // 16) * (lib().h264o_dec_coded_height(self.h) // 16)
        return np.array([[lib().h264o_dec_mb_intra_mode(self.h, i, k) for k in range(18)] for i in range(n)], dtype=np.uint8)

    def mb_mv(self, addr, blk4=0):
        x, y, r = C.c_int(0), C.c_int(0), C.c_int(0)
        lib().h264o_dec_mb_mv(self.h, addr, blk4, C.byref(x), C.byref(y), C.byref(r))
        return x.value, y.value, r.value

    @property
    def max_mb_bits(self):
        return lib().h264o_dec_max_mb_bits(self.h)

    @property
    def max_level_prefix(self):
        return lib().h264o_dec_max_level_prefix(self.h)

    STATS = ("max_intermediate", "max_level", "max_mvd", "mv_x_min", "mv_x_max", "mv_y_min", "mv_y_max",
             "out_left", "out_right", "out_top", "out_bottom")

    def stats(self):
        """h264o_dec_stat of the last decoded picture, by name"""
        return {n: lib().h264o_dec_stat(self.h, i) for i, n in enumerate(self.STATS)}

    def dbf(self):
        """h264o_dec_dbf of the last decoded picture: a Dbf (a copy)"""
        n = lib().h264o_dec_dbf_count()
        assert n == Dbf.COUNT, "oracle/h264_oracle.h and Dbf disagree about H264O_DBF_COUNT"
        return Dbf(np.ctypeslib.as_array(C.cast(lib().h264o_dec_dbf(self.h), C.POINTER(C.c_uint32)), shape=(n,)).astype(np.int64))

    def pred(self):
        """h264o_dec_pred of the last decoded picture: a Pred (a copy)"""
        n = lib().h264o_dec_pred_count()
        assert n == Pred.COUNT, "oracle/h264_oracle.h and Pred disagree about H264O_PRED_COUNT"
        return Pred(np.ctypeslib.as_array(C.cast(lib().h264o_dec_pred(self.h), C.POINTER(C.c_uint32)), shape=(n,)).astype(np.int64))

    def close(self):
        if self.h:
            lib().h264o_dec_destroy(self.h)
            self.h = None

    def __del__(self):
        self.close()


class Dbf:
    """the loop filter's account of one picture, or the sum of several (oracle/h264_oracle.h, H264O_DBF_*): tables[name] is
    (kind 0 luma / 1 chroma, bS - 1, index 0..51), cells[name] is (kind, bS - 1), ctx[name] a number"""
    TABLES = ("a_eval", "a_filt", "a_changed", "b_filt", "b_ap", "b_aq")
    CELLS = ("rej_alpha", "rej_p", "rej_q", "apaq_00", "apaq_01", "apaq_10", "apaq_11", "delta_clip_neg", "delta_clip_pos", "delta_unclipped",
             "delta_zero", "p1_clip_neg", "p1_clip_pos", "p1_unclipped", "q1_clip_neg", "q1_clip_pos", "q1_unclipped", "clip1_p0_at_0",
             "clip1_p0_at_255", "clip1_q0_at_0", "clip1_q0_at_255", "strong_00", "strong_01", "strong_10", "strong_11", "strong_false")
    CTX = ("left_qp_diff", "top_qp_diff", "left_qp_odd", "top_qp_odd", "pcm_p", "pcm_q", "cbcr_diff", "qpi_clip_0", "qpi_clip_51",
           "idc2_slice_edge_alone", "idc0_slice_edge_qp_diff", "t8_beside_4x4") + tuple("edge_%d_%d" % (d, e) for d in range(2) for e in range(4))
    COUNT = len(TABLES) * 416 + len(CELLS) * 8 + len(CTX)

    def __init__(self, flat=None):
        self.flat = np.zeros(self.COUNT, np.int64) if flat is None else flat
        nt, nc = len(self.TABLES) * 416, len(self.CELLS) * 8
        self.tables = dict(zip(self.TABLES, self.flat[:nt].reshape(len(self.TABLES), 2, 4, 52)))
        self.cells = dict(zip(self.CELLS, self.flat[nt:nt + nc].reshape(len(self.CELLS), 2, 4)))
        self.ctx = dict(zip(self.CTX, self.flat[nt + nc:]))

    def __add__(self, other):
        return Dbf(self.flat + other.flat)


class Pred:
    """the prediction account of one picture, or the sum of several (oracle/h264_oracle.h, H264O_PRED_*, says what every cell counts):
    p["name"] is the section as an array of its shape, in the header's order"""
    SHAPES = ("skip", "16x16", "16x8", "8x16", "8x8", "8x4", "4x8", "4x4")
    RELATIONS = ("inside", "cross_low", "cross_high", "beyond_low", "beyond_high", "cross_both")
    REASONS = ("outside", "other_slice", "not_yet_decoded", "constrained_inter", "same_mb", "intra_mb", "ipcm_mb", "inter_mb")
    SIDES = ("left", "top", "top_left", "top_right")
    SECTIONS = (("l_shape", (8, 4, 4)), ("l_ref", (3, 4, 4)), ("l_rel", (2, 4, 6)), ("l_cross", (2, 4, 2, 4)), ("l_corner", (2, 2)),
                ("b_ref", (3, 4, 4)), ("b_align", (4, 4)), ("b_rdist", (5,)), ("l_clip", (16, 3, 2)), ("c_frac", (8, 8)), ("c_rel", (2, 2, 6)),
                ("c_cross", (2, 2, 2, 4)), ("c_rdist", (8,)), ("c_pair", (3,)), ("c_pair_mixed", (1,)), ("i4", (9, 16)), ("i4_nb", (4, 8)),
                ("i4_tr_nyd", (16,)), ("i4_tr", (2, 2)), ("i16", (4, 8)), ("ic", (4, 8)), ("ic_dc", (4, 2, 2)), ("plane_clip", (2, 2)), ("ibi", (4, 2)))
    COUNT = sum(int(np.prod(shape)) for _, shape in SECTIONS)

    def __init__(self, flat=None):
        self.flat = np.zeros(self.COUNT, np.int64) if flat is None else flat
        self.sections, at = {}, 0
        for name, shape in self.SECTIONS:
            n = int(np.prod(shape))
            self.sections[name] = self.flat[at:at + n].reshape(shape)
            at += n

    def __getitem__(self, name):
        return self.sections[name]

    def __add__(self, other):
        return Pred(self.flat + other.flat)
