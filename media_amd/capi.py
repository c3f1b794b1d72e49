"""ctypes binding of the C ABI in include/mi355x_h264.h (media_amd/lib/libmi355x_h264.so).

This is plumbing for tests and bench.py; the product's host side is the C++
VideoEncoderMI355X class in media_amd/host/.  There is no fallback: if the HIP
library is missing or no device is usable, loading / creating raises.
"""
import ctypes as C
import os
import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "libmi355x_h264.so")
if os.environ.get("MI355X_H264_LIB"):   # A/B measurements: another build of the same library (media_amd/csrc/Makefile target `ab`)
    LIB_PATH = os.environ["MI355X_H264_LIB"]

LV_STRIDE = 416
MBINFO_DTYPE = np.dtype([("mvx", "<i2"), ("mvy", "<i2"), ("type", "u1"), ("i16_mode", "u1"),
                         ("chroma_mode", "u1"), ("cbp", "u1"), ("tc", "u1", (24,))])
FRAME_IDR, FRAME_P = 1, 3
DBG_RECON_Y, DBG_RECON_U, DBG_RECON_V, DBG_MBINFO, DBG_LEVELS, DBG_PRE_Y, DBG_PRE_U, DBG_PRE_V, DBG_MBAUX, DBG_MVQ, DBG_SRC = range(11)
K_NAMES = ["me", "tq", "intra", "cavlc", "deblock"]   # index = MI355X_H264_K_* (1: the id is still called K_PMB: k_tq / k_tq8 replaced k_pmb2)

EXPORTS = [
    "mi355x_h264_abi_version", "mi355x_h264_default_config", "mi355x_h264_create", "mi355x_h264_destroy",
    "mi355x_h264_encode", "mi355x_h264_encode_device", "mi355x_h264_encode_batch_device",
    "mi355x_h264_force_idr", "mi355x_h264_last_error", "mi355x_h264_coded_width", "mi355x_h264_coded_height",
    "mi355x_h264_debug_keep_pre", "mi355x_h264_debug_read", "mi355x_h264_stats_enable", "mi355x_h264_stats_read",
    "mi355x_h264_set_qp", "mi355x_h264_set_idr_pic_id", "mi355x_h264_encode_nv12", "mi355x_h264_encode_nv12_device",
    "mi355x_h264_encode_gops_device", "mi355x_h264_last_me_cost", "mi355x_h264_encode_rgba", "mi355x_h264_encode_rgba_device",
    "mi355x_h264_stream_open", "mi355x_h264_stream_close", "mi355x_h264_stream_encode", "mi355x_h264_stream_set_qp",
    "mi355x_h264_stream_force_idr", "mi355x_h264_stream_set_idr_pic_id", "mi355x_h264_stream_last_me_cost",
    "mi355x_h264_stream_last_error", "mi355x_h264_stream_debug_read", "mi355x_h264_stream_hub_stats",
    "mi355x_h264_stream_encode_device", "mi355x_h264_stream_encode_nv12", "mi355x_h264_stream_encode_rgba",
    "mi355x_h264_debug_code_syntax", "mi355x_h264_stream_debug_keep_pre", "mi355x_h264_stream_debug_last_step",
    "mi355x_h264_stream_open_ex", "mi355x_h264_stream_open_scaled", "mi355x_h264_stream_source_width", "mi355x_h264_stream_source_height",
    "mi355x_h264_quality_enable", "mi355x_h264_quality_read", "mi355x_h264_quality_map",
    "mi355x_h264_stream_quality_enable", "mi355x_h264_stream_last_quality", "mi355x_h264_stream_quality_map",
    "mi355x_h264_quality_enable_ex", "mi355x_h264_stream_quality_enable_ex", "mi355x_h264_quality_ssim_read", "mi355x_h264_quality_ssim_map",
    "mi355x_h264_stream_last_ssim", "mi355x_h264_stream_ssim_map",
    "mi355x_h264_debug_mem_guard", "mi355x_h264_debug_mem_guard_get", "mi355x_h264_debug_mem_tally", "mi355x_h264_debug_mem_check",
    "mi355x_h264_debug_mem_poke", "mi355x_h264_stream_debug_mem_check", "mi355x_h264_dec_debug_mem_check",
    "mi355x_h264_dec_group_debug_mem_check", "mi355x_h264_dec_group_debug_mem_poke",
    "mi355x_h264_create_colour", "mi355x_h264_stream_open_colour", "mi355x_h264_colour_of", "mi355x_h264_stream_colour",
    "mi355x_h264_dec_colour", "mi355x_h264_dec_set_rgba_colour", "mi355x_h264_dec_group_colour", "mi355x_h264_dec_group_set_rgba_colour",
    "mi355x_h264_parser_colour",
    "mi355x_h264_dec_set_output_size", "mi355x_h264_dec_output_size", "mi355x_h264_dec_group_set_output_size", "mi355x_h264_dec_group_output_size",
    "mi355x_h264_set_temporal_layers", "mi355x_h264_last_temporal_id", "mi355x_h264_stream_last_temporal_id",
    "mi355x_h264_set_intra_refresh", "mi355x_h264_last_refresh_band", "mi355x_h264_stream_last_refresh_band",
    "mi355x_h264_dec_set_loss_mode", "mi355x_h264_dec_damage", "mi355x_h264_dec_damage_map",
    "mi355x_h264_dec_group_set_loss_mode", "mi355x_h264_dec_group_damage", "mi355x_h264_dec_group_damage_map",
    "mi355x_h264_parser_set_loss_mode", "mi355x_h264_parser_loss",
    "mi355x_h264_stream_encode_damage", "mi355x_h264_stream_encode_nv12_damage", "mi355x_h264_stream_encode_rgba_damage",
    "mi355x_h264_stream_last_upload", "mi355x_h264_stream_debug_patch_stats",
]
E_ARG, E_OVERFLOW = -1, -5   # MI355X_H264_E_*
INPUT_I420, INPUT_NV12, INPUT_RGBA = 0, 1, 2   # MI355X_H264_INPUT_*
STREAM_MULTIREF, STREAM_TEMPORAL2, STREAM_INTRA_REFRESH = 1, 8, 32   # MI355X_H264_STREAM_* (mi355x_h264_stream_open_ex)
MATRIX_BT709, MATRIX_BT601 = 1, 6   # MI355X_H264_MATRIX_* (matrix_coefficients, Table E-5)
DAMAGE_DETECT = -0x44414D47   # MI355X_H264_DAMAGE_DETECT
UPLOAD_WHOLE, UPLOAD_PATCHED, UPLOAD_NOTHING, UPLOAD_IN_PLACE = range(4)   # MI355X_H264_UPLOAD_*
UPLOAD_NAMES = ["whole", "patched", "nothing", "in_place"]


class Config(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("width", C.c_int32), ("height", C.c_int32), ("fps", C.c_int32),
                ("bitrate", C.c_int32), ("gop", C.c_int32), ("profile_idc", C.c_int32), ("rc_mode", C.c_int32),
                ("qp", C.c_int32), ("device", C.c_int32), ("disable_deblock", C.c_int32),
                ("batch", C.c_int32), ("input_format", C.c_int32), ("slices", C.c_int32), ("band_index", C.c_int32), ("band_count", C.c_int32), ("refs", C.c_int32), ("search", C.c_int32)]


class Rect(C.Structure):
    """mi355x_h264_rect"""
    _fields_ = [("x", C.c_int32), ("y", C.c_int32), ("w", C.c_int32), ("h", C.c_int32)]


def _damage_args(damage):
    """(rects pointer or None, n, what to keep alive) of Stream.encode*(damage=...): "detect", or a sequence of (x, y, w, h)"""
    if isinstance(damage, str):
        if damage != "detect":
            raise ValueError("damage: None, \"detect\" or a list of (x, y, w, h)")
        return None, DAMAGE_DETECT, None
    rects = (Rect * max(1, len(damage)))(*[Rect(*[int(v) for v in r]) for r in damage])
    return (rects if len(damage) else None), len(damage), rects


class Colour(C.Structure):
    """mi355x_h264_colour"""
    _fields_ = [("struct_size", C.c_uint32), ("matrix", C.c_int32), ("full_range", C.c_int32)]


def colour_struct(colour):
    """a description as the C ABI takes it, from ("bt601" | "bt709", "limited" | "full"), from (matrix code, full_range) or from a
    Colour; None stays None (no description)"""
    if colour is None or isinstance(colour, Colour):
        return colour
    m, r = colour
    m = {"bt709": MATRIX_BT709, "bt601": MATRIX_BT601}.get(m, m)
    r = {"limited": 0, "full": 1}.get(r, r)
    if isinstance(m, str) or isinstance(r, str):
        raise ValueError("colour = %r: (\"bt601\" | \"bt709\", \"limited\" | \"full\")" % (colour,))
    return Colour(C.sizeof(Colour), int(m), int(r))


def _colour_read(fn, handle):
    """what mi355x_h264_colour_of / _stream_colour report: ("bt709", "full"), or None for a handle without a description"""
    c = Colour()
    rc = fn(handle, C.byref(c))
    if rc < 0:
        raise EncoderError("colour read -> %d" % rc)
    return ({MATRIX_BT709: "bt709", MATRIX_BT601: "bt601"}[c.matrix], "full" if c.full_range else "limited") if rc else None


class Stats(C.Structure):
    _fields_ = [("ms", C.c_double * 5), ("launches", C.c_uint64 * 5), ("mbs", C.c_uint64 * 5),
                ("frames", C.c_uint64), ("p_mbs", C.c_uint64), ("me_searched_mbs", C.c_uint64), ("tq_coded_mbs", C.c_uint64)]


class Quality(C.Structure):
    """mi355x_h264_quality"""
    _fields_ = [("sse", C.c_uint64 * 3), ("samples", C.c_uint64 * 3), ("bytes", C.c_uint32), ("qp", C.c_uint32),
                ("frame_type", C.c_uint32), ("valid", C.c_uint32)]


def psnr(sse, samples):
    """10 * log10(255^2 * samples / sse) on the host; an SSE of 0 gives inf (nothing compared: nan)"""
    import math
    if not samples:
        return float("nan")
    return float("inf") if sse == 0 else 10.0 * math.log10(65025.0 * samples / sse)


class Ssim(C.Structure):
    """mi355x_h264_ssim"""
    _fields_ = [("sum", C.c_int64 * 3), ("windows", C.c_uint64 * 3), ("valid", C.c_uint32), ("reserved", C.c_uint32)]


QUALITY_SSE, QUALITY_SSIM = 1, 2   # MI355X_H264_QUALITY_*


def ssim_mean(total, windows):
    """sum / (65536 * windows) on the host (nothing compared: nan)"""
    return total / (65536.0 * windows) if windows else float("nan")


def _with_ssim(rec, s):
    """the SSIM record s (an Ssim) added to the SSE record's dict: `ssim` (Y, U, V means), `ssim_sum`, `ssim_windows`"""
    tot, win = [int(v) for v in s.sum], [int(v) for v in s.windows]
    rec["ssim_sum"], rec["ssim_windows"] = tot, win
    rec["ssim"] = [ssim_mean(a, b) if s.valid else float("nan") for a, b in zip(tot, win)]
    return rec


def _quality_record(q):
    """a Quality as a dict, `psnr` (Y, U, V) added"""
    sse, samples = [int(v) for v in q.sse], [int(v) for v in q.samples]
    return {"sse": sse, "samples": samples, "bytes": int(q.bytes), "qp": int(q.qp), "frame_type": int(q.frame_type), "valid": bool(q.valid),
            "psnr": [psnr(a, b) if q.valid else float("nan") for a, b in zip(sse, samples)]}


_lib = None


def lib():
    """load the HIP library; raises OSError when it has not been built"""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise OSError("HIP extension missing: %s (run __graft_entry__.build())" % LIB_PATH)
        L = C.CDLL(LIB_PATH)
        vp = C.c_void_p
        L.mi355x_h264_default_config.argtypes = [C.POINTER(Config)]
        L.mi355x_h264_create.argtypes = [C.POINTER(Config), C.POINTER(vp)]
        L.mi355x_h264_destroy.argtypes = [vp]
        L.mi355x_h264_destroy.restype = None
        L.mi355x_h264_encode.argtypes = [vp, vp, C.c_int, vp, C.c_int, vp, C.c_int, C.POINTER(vp),
                                         C.POINTER(C.c_uint32), C.POINTER(C.c_int)]
        L.mi355x_h264_encode_device.argtypes = [vp, vp, C.POINTER(vp), C.POINTER(C.c_uint32), C.POINTER(C.c_int)]
        L.mi355x_h264_encode_nv12.argtypes = [vp, vp, C.c_int, vp, C.c_int, C.POINTER(vp), C.POINTER(C.c_uint32), C.POINTER(C.c_int)]
        L.mi355x_h264_encode_nv12_device.argtypes = [vp, vp, C.POINTER(vp), C.POINTER(C.c_uint32), C.POINTER(C.c_int)]
        L.mi355x_h264_encode_rgba.argtypes = [vp, vp, C.c_int, C.POINTER(vp), C.POINTER(C.c_uint32), C.POINTER(C.c_int)]
        L.mi355x_h264_encode_rgba_device.argtypes = [vp, vp, C.POINTER(vp), C.POINTER(C.c_uint32), C.POINTER(C.c_int)]
        L.mi355x_h264_encode_batch_device.argtypes = [vp, vp, C.c_size_t, C.c_int, vp, C.c_size_t, vp,
                                                      C.POINTER(C.c_size_t)]
        L.mi355x_h264_encode_gops_device.argtypes = [vp, vp, C.c_size_t, C.c_size_t, C.c_int, vp, C.c_size_t, vp, vp]
        L.mi355x_h264_last_me_cost.argtypes = [vp, vp]
        L.mi355x_h264_force_idr.argtypes = [vp]
        L.mi355x_h264_set_qp.argtypes = [vp, C.c_int]
        L.mi355x_h264_set_idr_pic_id.argtypes = [vp, C.c_int, C.c_int]
        L.mi355x_h264_band_info.argtypes = [vp, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_size_t)]
        L.mi355x_h264_band_halo_export.argtypes = [vp, C.c_int, vp]
        L.mi355x_h264_band_halo_import.argtypes = [vp, C.c_int, vp]
        L.mi355x_h264_last_error.argtypes = [vp]
        L.mi355x_h264_last_error.restype = C.c_char_p
        L.mi355x_h264_coded_width.argtypes = [vp]
        L.mi355x_h264_coded_height.argtypes = [vp]
        L.mi355x_h264_debug_keep_pre.argtypes = [vp, C.c_int]
        L.mi355x_h264_debug_read.argtypes = [vp, C.c_int, vp, C.c_size_t]
        L.mi355x_h264_debug_read.restype = C.c_int64
        L.mi355x_h264_debug_code_syntax.argtypes = [vp, vp, vp, vp, vp, vp, C.POINTER(vp), C.POINTER(C.c_uint32), C.POINTER(C.c_int)]
        L.mi355x_h264_stream_open.argtypes = [C.POINTER(Config), C.POINTER(vp)]
        L.mi355x_h264_stream_open_ex.argtypes = [C.POINTER(Config), C.c_uint32, C.POINTER(vp)]
        if hasattr(L, "mi355x_h264_stream_open_scaled"):   # (an A/B library of an earlier build has no scaled streams)
            L.mi355x_h264_stream_open_scaled.argtypes = [C.POINTER(Config), C.c_uint32, C.c_int, C.c_int, C.POINTER(vp)]
            L.mi355x_h264_stream_source_width.argtypes = [vp]
            L.mi355x_h264_stream_source_height.argtypes = [vp]
        L.mi355x_h264_stream_close.argtypes = [vp]
        L.mi355x_h264_stream_close.restype = None
        L.mi355x_h264_stream_encode.argtypes = [vp, vp, C.c_int, vp, C.c_int, vp, C.c_int, C.POINTER(vp), C.POINTER(C.c_uint32), C.POINTER(C.c_int)]
        L.mi355x_h264_stream_encode_device.argtypes = [vp, vp, C.POINTER(vp), C.POINTER(C.c_uint32), C.POINTER(C.c_int)]
        L.mi355x_h264_stream_encode_nv12.argtypes = [vp, vp, C.c_int, vp, C.c_int, C.POINTER(vp), C.POINTER(C.c_uint32), C.POINTER(C.c_int)]
        L.mi355x_h264_stream_encode_rgba.argtypes = [vp, vp, C.c_int, C.POINTER(vp), C.POINTER(C.c_uint32), C.POINTER(C.c_int)]
        if hasattr(L, "mi355x_h264_stream_encode_damage"):
            tail = [C.POINTER(Rect), C.c_int, C.POINTER(vp), C.POINTER(C.c_uint32), C.POINTER(C.c_int)]
            L.mi355x_h264_stream_encode_damage.argtypes = [vp, vp, C.c_int, vp, C.c_int, vp, C.c_int] + tail
            L.mi355x_h264_stream_encode_nv12_damage.argtypes = [vp, vp, C.c_int, vp, C.c_int] + tail
            L.mi355x_h264_stream_encode_rgba_damage.argtypes = [vp, vp, C.c_int] + tail
            L.mi355x_h264_stream_last_upload.argtypes = [vp, C.POINTER(C.c_uint64), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(C.c_int)]
            L.mi355x_h264_stream_debug_patch_stats.argtypes = [vp, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
        L.mi355x_h264_stream_set_qp.argtypes = [vp, C.c_int]
        L.mi355x_h264_stream_force_idr.argtypes = [vp]
        L.mi355x_h264_stream_set_idr_pic_id.argtypes = [vp, C.c_int]
        L.mi355x_h264_stream_last_me_cost.argtypes = [vp, C.POINTER(C.c_uint32)]
        L.mi355x_h264_stream_last_error.argtypes = [vp]
        L.mi355x_h264_stream_last_error.restype = C.c_char_p
        L.mi355x_h264_stream_coded_width.argtypes = [vp]
        L.mi355x_h264_stream_coded_height.argtypes = [vp]
        L.mi355x_h264_stream_debug_read.argtypes = [vp, C.c_int, vp, C.c_size_t]
        L.mi355x_h264_stream_debug_read.restype = C.c_int64
        L.mi355x_h264_stream_debug_keep_pre.argtypes = [vp, C.c_int]
        L.mi355x_h264_stream_debug_last_step.argtypes = [vp, C.POINTER(C.c_uint64), C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]
        L.mi355x_h264_stream_hub_stats.argtypes = [vp, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_int)]
        L.mi355x_h264_quality_enable.argtypes = [vp, C.c_int]
        L.mi355x_h264_quality_read.argtypes = [vp, C.POINTER(Quality), C.c_size_t]
        L.mi355x_h264_quality_read.restype = C.c_int64
        L.mi355x_h264_quality_map.argtypes = [vp, C.c_int, vp, C.c_size_t]
        L.mi355x_h264_quality_map.restype = C.c_int64
        L.mi355x_h264_stream_quality_enable.argtypes = [vp, C.c_int]
        L.mi355x_h264_stream_last_quality.argtypes = [vp, C.POINTER(Quality)]
        L.mi355x_h264_stream_quality_map.argtypes = [vp, vp, C.c_size_t]
        L.mi355x_h264_stream_quality_map.restype = C.c_int64
        if hasattr(L, "mi355x_h264_quality_enable_ex"):   # (an A/B library of an earlier build, MI355X_H264_LIB, has no SSIM)
            L.mi355x_h264_quality_enable_ex.argtypes = [vp, C.c_uint]
            L.mi355x_h264_stream_quality_enable_ex.argtypes = [vp, C.c_uint]
            L.mi355x_h264_quality_ssim_read.argtypes = [vp, C.POINTER(Ssim), C.c_size_t]
            L.mi355x_h264_quality_ssim_read.restype = C.c_int64
            L.mi355x_h264_quality_ssim_map.argtypes = [vp, C.c_int, vp, C.c_size_t]
            L.mi355x_h264_quality_ssim_map.restype = C.c_int64
            L.mi355x_h264_stream_last_ssim.argtypes = [vp, C.POINTER(Ssim)]
            L.mi355x_h264_stream_ssim_map.argtypes = [vp, vp, C.c_size_t]
            L.mi355x_h264_stream_ssim_map.restype = C.c_int64
        L.mi355x_h264_stats_enable.argtypes = [vp, C.c_int]
        if hasattr(L, "mi355x_h264_set_temporal_layers"):
            L.mi355x_h264_set_temporal_layers.argtypes = [vp, C.c_int]
            L.mi355x_h264_last_temporal_id.argtypes = [vp]
            L.mi355x_h264_stream_last_temporal_id.argtypes = [vp]
        if hasattr(L, "mi355x_h264_set_intra_refresh"):
            L.mi355x_h264_set_intra_refresh.argtypes = [vp, C.c_int]
            L.mi355x_h264_last_refresh_band.argtypes = [vp]
            L.mi355x_h264_stream_last_refresh_band.argtypes = [vp]
        if hasattr(L, "mi355x_h264_debug_mem_guard"):   # (an A/B library of an earlier build, MI355X_H264_LIB, has no guard mode)
            L.mi355x_h264_debug_mem_guard.argtypes = [C.c_int64, C.c_int]
            L.mi355x_h264_debug_mem_guard_get.argtypes = [C.POINTER(C.c_int64), C.POINTER(C.c_int)]
            L.mi355x_h264_debug_mem_tally.argtypes = [C.c_int]
            L.mi355x_h264_debug_mem_tally.restype = C.c_int64
            for name in ("mi355x_h264_debug_mem_check", "mi355x_h264_stream_debug_mem_check", "mi355x_h264_dec_debug_mem_check",
                         "mi355x_h264_dec_group_debug_mem_check"):
                getattr(L, name).argtypes = [vp, C.POINTER(C.c_int), C.c_char_p, C.c_size_t]
            for name in ("mi355x_h264_debug_mem_poke", "mi355x_h264_dec_group_debug_mem_poke"):
                getattr(L, name).argtypes = [vp, C.c_char_p, C.c_int64, C.c_int]
        L.mi355x_h264_stats_read.argtypes = [vp, C.POINTER(Stats), C.c_int]
        if hasattr(L, "mi355x_h264_create_colour"):   # (an A/B library of an earlier build has no colour descriptions)
            L.mi355x_h264_create_colour.argtypes = [C.POINTER(Config), C.POINTER(Colour), C.POINTER(vp)]
            L.mi355x_h264_stream_open_colour.argtypes = [C.POINTER(Config), C.c_uint32, C.c_int, C.c_int, C.POINTER(Colour), C.POINTER(vp)]
            L.mi355x_h264_colour_of.argtypes = [vp, C.POINTER(Colour)]
            L.mi355x_h264_stream_colour.argtypes = [vp, C.POINTER(Colour)]
        _lib = L
    return _lib


class EncoderError(RuntimeError):
    rc = 0   # the MI355X_H264_E_* code, where a call returned one


# ---- the guard mode of the library's own memory (include/mi355x_h264.h, mi355x_h264_debug_mem_guard) ----
def mem_guard(guard_bytes, poison=False):
    """the process-wide switch, for owners created afterwards; returns the setting it replaces, as (guard_bytes, poison)"""
    was = mem_guard_get()
    rc = lib().mi355x_h264_debug_mem_guard(int(guard_bytes), int(bool(poison)))
    if rc != 0:
        err = EncoderError("mi355x_h264_debug_mem_guard(%d) -> %d" % (guard_bytes, rc))
        err.rc = rc
        raise err
    return was


def mem_guard_get():
    g, p = C.c_int64(), C.c_int()
    lib().mi355x_h264_debug_mem_guard_get(C.byref(g), C.byref(p))
    return g.value, bool(p.value)


def mem_tally(reset=False):
    """damaged guard regions found while blocks were freed, process-wide"""
    return int(lib().mi355x_h264_debug_mem_tally(int(reset)))


def _mem_check(fn, handle, last_error):
    """(damaged regions, regions examined, report lines: "examined blocks=B slack=S", then one per damaged region) of one of the
    four check calls; raises EncoderError (rc = E_ARG: the
    owner was created without guards)"""
    regions, buf = C.c_int(), C.create_string_buffer(1 << 16)
    n = fn(handle, C.byref(regions), buf, len(buf))
    if n < 0:
        err = EncoderError("mem_check -> %d: %s" % (n, last_error()))
        err.rc = n
        raise err
    return n, regions.value, [ln for ln in buf.value.decode().split("\n") if ln]


def _planes(f, w, h, strides, nv12=False):
    """(address, stride) of every plane for the host entry points.  f: one tight picture (numpy uint8) - or, with `strides`, a
    sequence of separate plane arrays (Y, U, V; NV12: Y, UV) whose rows lie strides[k] bytes apart; also returns what to keep alive"""
    if strides is None:
        f = np.ascontiguousarray(f, dtype=np.uint8)
        base = f.ctypes.data
        if nv12:
            return [(base, w), (base + w * h, w)], f
        return [(base, w), (base + w * h, w // 2), (base + w * h * 5 // 4, w // 2)], f
    keep = [np.ascontiguousarray(p, dtype=np.uint8) for p in f]
    return [(p.ctypes.data, int(st)) for p, st in zip(keep, strides)], keep


def _debug_read(obj, fn, what):
    """one MI355X_H264_DBG_* buffer of an Encoder's or a Stream's last picture as a numpy array in its natural shape"""
    if what in (DBG_RECON_Y, DBG_PRE_Y):
        a = np.empty((obj.ch, obj.cw), np.uint8)
    elif what in (DBG_RECON_U, DBG_RECON_V, DBG_PRE_U, DBG_PRE_V):
        a = np.empty((obj.ch // 2, obj.cw // 2), np.uint8)
    elif what == DBG_MBINFO:
        a = np.empty(obj.nmb, MBINFO_DTYPE)
    elif what == DBG_MBAUX:
        a = np.empty((obj.nmb, 16), np.uint8)
    elif what == DBG_MVQ:
        a = np.empty((obj.nmb, 8), np.int16)
    elif what == DBG_LEVELS:
        a = np.empty((obj.nmb, LV_STRIDE), np.int16)
    elif what == DBG_SRC:   # the tight source picture in staging memory (I420; NV12 for NV12 input), display size, flat
        a = np.empty(obj.width * obj.height * 3 // 2, np.uint8)
    else:
        raise ValueError("debug_read(%r)" % (what,))
    n = fn(obj.h, what, a.ctypes.data, a.nbytes)
    if n != a.nbytes:
        err = EncoderError("debug_read(%d) -> %d%s" % (what, n, ": " + obj.last_error() if n == E_ARG else ""))
        err.rc = n   # (E_ARG for DBG_SRC: the last picture was read in place, there is no staging picture)
        raise err
    return a


class Encoder:
    """thin object wrapper; argument meaning follows mi355x_h264_config"""

    def __init__(self, width, height, qp=26, gop=30, fps=30, profile_idc=66, device=0, disable_deblock=0,
                 bitrate=5000000, rc_mode=0, batch=1, input_format=0, slices=0, band_index=0, band_count=0, refs=0, search=1, colour=None, temporal_layers=1,
                 intra_refresh=False):
        """colour = ("bt601" | "bt709", "limited" | "full"): the encoder is created with mi355x_h264_create_colour - its SPS carries
        the description and encode_rgba converts with that variant; None: mi355x_h264_create.
        temporal_layers = 2: every second P picture is a non-reference picture (mi355x_h264_set_temporal_layers).
        intra_refresh: the `slices` bands are coded all intra in turn, one per P picture (mi355x_h264_set_intra_refresh)"""
        L = lib()
        self.h = None
        if intra_refresh and (not 2 <= slices <= 32 or refs > 1 or temporal_layers != 1 or band_count > 1):   # (before the device is touched)
            err = EncoderError("intra_refresh: slices 2 .. 32, one reference picture, one temporal layer, no band instance")
            err.rc = E_ARG
            raise err
        if temporal_layers not in (1, 2) or (temporal_layers == 2 and band_count > 1):   # (refused before the device is touched)
            err = EncoderError("temporal_layers: 1 or 2, and 2 not on a band instance")
            err.rc = E_ARG
            raise err
        cfg = Config()
        L.mi355x_h264_default_config(C.byref(cfg))
        cfg.width, cfg.height, cfg.qp, cfg.gop, cfg.fps = width, height, qp, gop, fps
        cfg.profile_idc, cfg.device, cfg.disable_deblock = profile_idc, device, disable_deblock
        cfg.bitrate, cfg.rc_mode, cfg.batch = bitrate, rc_mode, batch
        cfg.input_format = input_format   # 0 I420, 1 NV12: layout of pictures handed over in device memory
        cfg.slices = slices               # > 1: that many bands of macroblock rows, one slice NAL unit each
        cfg.band_index, cfg.band_count = band_index, band_count   # band_count > 1: this instance codes its share of the slices
        cfg.refs = refs                                           # reference frames searched (0 / 1: one, the reference preset)
        cfg.search = search                                       # 0 exhaustive integer search, 1 seeded by the previous picture's vector (the default)
        self.batch = batch
        self.h = C.c_void_p()
        if colour is None:
            rc = L.mi355x_h264_create(C.byref(cfg), C.byref(self.h))
        else:
            rc = L.mi355x_h264_create_colour(C.byref(cfg), C.byref(colour_struct(colour)), C.byref(self.h))
        if rc != 0:
            self.h = None
            err = EncoderError("mi355x_h264_create%s failed: %d" % ("" if colour is None else "_colour", rc))
            err.rc = rc
            raise err
        self.width, self.height = width, height
        self.cw, self.ch = L.mi355x_h264_coded_width(self.h), L.mi355x_h264_coded_height(self.h)
        self.nmb = (self.cw // 16) * (self.ch // 16)
        if temporal_layers != 1:
            try:
                self.set_temporal_layers(temporal_layers)
            except EncoderError:
                self.close()
                raise
        if intra_refresh:
            try:
                self.set_intra_refresh(True)
            except EncoderError:
                self.close()
                raise

    def set_intra_refresh(self, on):
        """before the first picture, on an encoder with slices = 2 .. 32 (mi355x_h264_set_intra_refresh)"""
        self._check(lib().mi355x_h264_set_intra_refresh(self.h, 1 if on else 0))

    @property
    def last_refresh_band(self):
        """the all-intra band k of the last finished picture; -1 for an IDR picture or with refresh off"""
        return lib().mi355x_h264_last_refresh_band(self.h)

    def _check(self, rc):
        if rc != 0:
            err = EncoderError("rc=%d: %s" % (rc, lib().mi355x_h264_last_error(self.h).decode()))
            err.rc = rc
            raise err

    def set_temporal_layers(self, layers):
        """1 or 2, before the first picture (mi355x_h264_set_temporal_layers)"""
        self._check(lib().mi355x_h264_set_temporal_layers(self.h, int(layers)))

    @property
    def last_temporal_id(self):
        """temporal layer (0 / 1) of the last finished picture"""
        return lib().mi355x_h264_last_temporal_id(self.h)

    @property
    def colour(self):
        """the description the encoder was created with, ("bt709", "full") ..., or None"""
        return _colour_read(lib().mi355x_h264_colour_of, self.h)

    def encode(self, i420, strides=None):
        """host I420 (numpy uint8, width*height*3/2) -> (bytes, frame_type); with strides = (y, u, v) in bytes, i420 is the
        three planes as separate arrays"""
        ((y, ys), (u, us), (v, vs)), keep = _planes(i420, self.width, self.height, strides)   # keep: alive during the call
        out, n, ft = C.c_void_p(), C.c_uint32(), C.c_int()
        self._check(lib().mi355x_h264_encode(self.h, y, ys, u, us, v, vs, C.byref(out), C.byref(n), C.byref(ft)))
        del keep
        return C.string_at(out.value, n.value), ft.value

    def encode_nv12(self, nv12, strides=None):
        """host NV12 (Y plane then interleaved UV) -> (bytes, frame_type); with strides = (y, uv), nv12 is the two planes"""
        ((y, ys), (uv, uvs)), keep = _planes(nv12, self.width, self.height, strides, nv12=True)
        out, n, ft = C.c_void_p(), C.c_uint32(), C.c_int()
        self._check(lib().mi355x_h264_encode_nv12(self.h, y, ys, uv, uvs, C.byref(out), C.byref(n), C.byref(ft)))
        return C.string_at(out.value, n.value), ft.value

    def code_syntax(self, mbinfo, levels, mvq, mbaux, src_i420):
        """mi355x_h264_debug_code_syntax: one picture per batch item from given decisions (arrays in the debug_read layouts, `batch`
        items one after the other; src_i420: `batch` tight pictures).  Returns (rc, [access unit or None per item], frame_type):
        the error code is returned, not raised - the items that did not fail are still delivered"""
        a = [np.ascontiguousarray(x) for x in (mbinfo, levels, mvq, mbaux, src_i420)]
        sizes = (self.nmb * 32, self.nmb * LV_STRIDE * 2, self.nmb * 16, self.nmb * 16, self.width * self.height * 3 // 2)
        for x, n in zip(a, sizes):
            if x.nbytes != n * self.batch:
                raise ValueError("array of %d bytes where %d x %d are expected" % (x.nbytes, self.batch, n))
        out, n, ft = (C.c_void_p * self.batch)(), (C.c_uint32 * self.batch)(), C.c_int()
        rc = lib().mi355x_h264_debug_code_syntax(self.h, *[x.ctypes.data for x in a], out, n, C.byref(ft))
        return rc, [C.string_at(out[g], n[g]) if out[g] else None for g in range(self.batch)], ft.value

    def last_error(self):
        return lib().mi355x_h264_last_error(self.h).decode()

    def encode_rgba(self, rgba, stride=None):
        """host RGBA (height x width x 4 bytes, or rows `stride` bytes apart) -> (bytes, frame_type)"""
        f = np.ascontiguousarray(rgba, dtype=np.uint8)
        out, n, ft = C.c_void_p(), C.c_uint32(), C.c_int()
        self._check(lib().mi355x_h264_encode_rgba(self.h, f.ctypes.data, int(stride or 4 * self.width), C.byref(out), C.byref(n), C.byref(ft)))
        return C.string_at(out.value, n.value), ft.value

    def encode_rgba_device(self, dev_ptr):
        out, n, ft = C.c_void_p(), C.c_uint32(), C.c_int()
        self._check(lib().mi355x_h264_encode_rgba_device(self.h, C.c_void_p(dev_ptr), C.byref(out), C.byref(n), C.byref(ft)))
        return C.string_at(out.value, n.value), ft.value

    def encode_device(self, dev_ptr):
        out, n, ft = C.c_void_p(), C.c_uint32(), C.c_int()
        self._check(lib().mi355x_h264_encode_device(self.h, C.c_void_p(dev_ptr), C.byref(out), C.byref(n), C.byref(ft)))
        return C.string_at(out.value, n.value), ft.value

    def encode_batch_device(self, dev_ptr, stride, count, out_buf, sizes):
        """out_buf: numpy uint8 host buffer; sizes: numpy uint32[count]; returns total bytes"""
        tot = C.c_size_t()
        self._check(lib().mi355x_h264_encode_batch_device(self.h, C.c_void_p(dev_ptr), stride, count,
                                                          out_buf.ctypes.data, out_buf.size, sizes.ctypes.data,
                                                          C.byref(tot)))
        return tot.value

    def encode_gops_device(self, dev_ptr, frame_stride, gop_stride, frames_per_gop, out_buf, out_cap_per_gop, sizes, gop_bytes):
        """lockstep encode of `batch` closed GOPs; out_buf uint8[batch*out_cap_per_gop], sizes uint32[batch*frames],
        gop_bytes uint64[batch]"""
        self._check(lib().mi355x_h264_encode_gops_device(self.h, C.c_void_p(dev_ptr), frame_stride, gop_stride, frames_per_gop,
                                                         out_buf.ctypes.data, out_cap_per_gop, sizes.ctypes.data,
                                                         gop_bytes.ctypes.data))

    def me_cost(self):
        a = np.zeros(self.batch, np.uint32)
        self._check(lib().mi355x_h264_last_me_cost(self.h, a.ctypes.data))
        return a

    def force_idr(self):
        self._check(lib().mi355x_h264_force_idr(self.h))

    def set_qp(self, qp):
        self._check(lib().mi355x_h264_set_qp(self.h, qp))

    def set_idr_pic_id(self, nxt, step=1):
        self._check(lib().mi355x_h264_set_idr_pic_id(self.h, nxt, step))

    def band_info(self):
        """(first macroblock row, rows, first slice, slices, halo bytes) of the band this instance codes"""
        r0, rows, s0, ns, hb = C.c_int(), C.c_int(), C.c_int(), C.c_int(), C.c_size_t()
        self._check(lib().mi355x_h264_band_info(self.h, C.byref(r0), C.byref(rows), C.byref(s0), C.byref(ns), C.byref(hb)))
        return r0.value, rows.value, s0.value, ns.value, hb.value

    def halo_export(self, edge, d_dst):
        """edge 0: this band's top rows, 1: its bottom rows, of the newest reconstruction -> device buffer"""
        self._check(lib().mi355x_h264_band_halo_export(self.h, edge, d_dst))

    def halo_import(self, edge, d_src):
        """edge 0: rows right above the band (the upper neighbour's bottom rows), 1: rows right below"""
        self._check(lib().mi355x_h264_band_halo_import(self.h, edge, d_src))

    def keep_pre(self, on=True):
        self._check(lib().mi355x_h264_debug_keep_pre(self.h, int(on)))

    def debug_read(self, what):
        return _debug_read(self, lib().mi355x_h264_debug_read, what)

    def quality_enable(self, on=True, ssim=False):
        """the quality report (mi355x_h264_quality_enable): SSE per plane and per macroblock of every picture from the next one on;
        ssim: SSIM beside it (mi355x_h264_quality_enable_ex with both metrics)"""
        if on and ssim:
            self._check(lib().mi355x_h264_quality_enable_ex(self.h, QUALITY_SSE | QUALITY_SSIM))
        else:
            self._check(lib().mi355x_h264_quality_enable(self.h, int(on)))
        self._ssim = bool(on and ssim)

    def quality(self, cap=None):
        """the records of every picture of the last call, in the order of sizes[] (mi355x_h264_quality_read), as dicts with `psnr`
        (Y, U, V; computed here) added; raises EncoderError (rc = E_ARG) when there is nothing to read"""
        n = 4096 if cap is None else cap
        a = (Quality * max(n, 1))()
        got = lib().mi355x_h264_quality_read(self.h, a, n)
        if got < 0:
            self._check(int(got))
        recs = [_quality_record(a[i]) for i in range(got)]
        if getattr(self, "_ssim", False) or os.environ.get("MI355X_H264_QUALITY") == "3":   # (SSIM off: the dictionaries are what they were)
            b = (Ssim * max(n, 1))()
            if lib().mi355x_h264_quality_ssim_read(self.h, b, n) == got:
                recs = [_with_ssim(r, b[i]) for i, r in enumerate(recs)]
        return recs

    def ssim_map(self, item=0):
        """the sum of q over the luma windows whose origin lies in the macroblock, of the last picture of batch item `item`: int32
        (rows, columns)"""
        m = np.zeros((self.ch // 16, self.cw // 16), np.int32)
        got = lib().mi355x_h264_quality_ssim_map(self.h, item, m.ctypes.data, m.size)
        if got < 0:
            self._check(int(got))
        return m

    def quality_map(self, item=0):
        """SSE per macroblock (all planes added) of the last picture of batch item `item`: uint32 (rows, columns)"""
        m = np.zeros((self.ch // 16, self.cw // 16), np.uint32)
        got = lib().mi355x_h264_quality_map(self.h, item, m.ctypes.data, m.size)
        if got < 0:
            self._check(int(got))
        return m

    def mem_check(self):
        """(damaged regions, regions examined, report lines): mi355x_h264_debug_mem_check"""
        return _mem_check(lib().mi355x_h264_debug_mem_check, self.h, self.last_error)

    def mem_poke(self, block, offset, value):
        """one byte of a guard region set from the host (value -1: put back); returns the call's code"""
        return lib().mi355x_h264_debug_mem_poke(self.h, block.encode(), int(offset), int(value))

    def stats_enable(self, on=True):
        self._check(lib().mi355x_h264_stats_enable(self.h, int(on)))

    def stats(self, reset=True):
        s = Stats()
        self._check(lib().mi355x_h264_stats_read(self.h, C.byref(s), int(reset)))
        return {"frames": s.frames, "p_mbs": s.p_mbs, "me_searched_mbs": s.me_searched_mbs, "tq_coded_mbs": s.tq_coded_mbs,
                "kernels": {K_NAMES[i]: {"ms": s.ms[i], "launches": s.launches[i], "mbs": s.mbs[i]} for i in range(5)}}

    def close(self):
        if getattr(self, "h", None):
            lib().mi355x_h264_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Stream:
    """a stream of the shared engine (include/mi355x_h264.h, "streams"): one picture per call, coded together with the pictures
    other streams of the same geometry deliver at about the same time; thread-safe across streams (one thread per stream).
    input_format (INPUT_I420 / INPUT_NV12 / INPUT_RGBA) is the layout of every picture of the stream, from host or device memory.
    refs 2 / 3: that many reference pictures are searched; the stream is opened with mi355x_h264_stream_open_ex (as it is whenever
    `flags` is given: the flags of that call).  src_size = (SW, SH): a scaled stream (mi355x_h264_stream_open_scaled) - every encode
    call takes pictures of SW x SH, which the device resamples to width x height; debug_read(DBG_SRC) is the resampled picture.
    colour = ("bt601" | "bt709", "limited" | "full"): a described stream (mi355x_h264_stream_open_colour; combines with src_size
    and flags): its SPS carries the description, and RGBA pictures are converted with that variant.
    temporal_layers = 2: MI355X_H264_STREAM_TEMPORAL2 joins the flags - every second P picture is a non-reference picture; any other
    value but 1 is refused here (the flag has no way to carry it)"""

    def __init__(self, width, height, qp=26, gop=30, fps=30, profile_idc=66, device=0, disable_deblock=0, slices=0, search=1,
                 input_format=0, refs=0, flags=None, src_size=None, colour=None, temporal_layers=1,
                 intra_refresh=False):
        """intra_refresh: MI355X_H264_STREAM_INTRA_REFRESH joins the flags - the `slices` bands are coded all intra in turn"""
        L = lib()
        cfg = Config()
        L.mi355x_h264_default_config(C.byref(cfg))
        cfg.width, cfg.height, cfg.qp, cfg.gop, cfg.fps = width, height, qp, gop, fps
        cfg.profile_idc, cfg.device, cfg.disable_deblock, cfg.slices, cfg.search = profile_idc, device, disable_deblock, slices, search
        cfg.input_format = input_format
        cfg.refs = refs
        if flags is None and refs > 1:
            flags = STREAM_MULTIREF
        if temporal_layers not in (1, 2):
            err = EncoderError("temporal_layers: 1 or 2")
            err.rc = E_ARG
            raise err
        if temporal_layers == 2:
            flags = (flags or 0) | STREAM_TEMPORAL2
        if intra_refresh:
            flags = (flags or 0) | STREAM_INTRA_REFRESH
        self.h = C.c_void_p()
        if colour is not None:
            sw, sh = (width, height) if src_size is None else (int(src_size[0]), int(src_size[1]))
            rc = L.mi355x_h264_stream_open_colour(C.byref(cfg), flags or 0, sw, sh, C.byref(colour_struct(colour)), C.byref(self.h))
        elif src_size is not None:
            rc = L.mi355x_h264_stream_open_scaled(C.byref(cfg), flags or 0, int(src_size[0]), int(src_size[1]), C.byref(self.h))
        elif flags is None:
            rc = L.mi355x_h264_stream_open(C.byref(cfg), C.byref(self.h))
        else:
            rc = L.mi355x_h264_stream_open_ex(C.byref(cfg), flags, C.byref(self.h))
        if rc != 0:
            self.h = None
            err = EncoderError("mi355x_h264_stream_open%s failed: %d" % ("_colour" if colour is not None else "_scaled" if src_size is not None else "" if flags is None else "_ex", rc))
            err.rc = rc
            raise err
        self.width, self.height = width, height
        self.src_width, self.src_height = (width, height) if src_size is None else (int(src_size[0]), int(src_size[1]))   # what the calls take
        self.cw, self.ch = L.mi355x_h264_stream_coded_width(self.h), L.mi355x_h264_stream_coded_height(self.h)
        self.nmb = (self.cw // 16) * (self.ch // 16)

    def _check(self, rc):
        if rc != 0:
            err = EncoderError("rc=%d: %s" % (rc, lib().mi355x_h264_stream_last_error(self.h).decode()))
            err.rc = rc
            raise err

    def encode(self, i420, strides=None, damage=None):
        """host I420; with strides = (y, u, v) in bytes, i420 is the three planes as separate arrays.  damage (here and on the NV12
        and RGBA forms): None - the ordinary call, the whole picture; "detect" or [(x, y, w, h), ...] - the damage call
        (mi355x_h264_stream_encode_damage): only the tiles that changed are transferred"""
        ((y, ys), (u, us), (v, vs)), keep = _planes(i420, self.src_width, self.src_height, strides)
        out, n, ft = C.c_void_p(), C.c_uint32(), C.c_int()
        if damage is None:
            self._check(lib().mi355x_h264_stream_encode(self.h, y, ys, u, us, v, vs, C.byref(out), C.byref(n), C.byref(ft)))
        else:
            rects, nr, keep2 = _damage_args(damage)
            self._check(lib().mi355x_h264_stream_encode_damage(self.h, y, ys, u, us, v, vs, rects, nr, C.byref(out), C.byref(n), C.byref(ft)))
        return C.string_at(out.value, n.value), ft.value

    @property
    def last_upload(self):
        """what the stream's last picture put on the link (mi355x_h264_stream_last_upload): bytes, damaged tiles, the grid's
        tiles, mode ("whole" / "patched" / "nothing" / "in_place")"""
        b, t, tt, m = C.c_uint64(), C.c_uint32(), C.c_uint32(), C.c_int()
        self._check(lib().mi355x_h264_stream_last_upload(self.h, C.byref(b), C.byref(t), C.byref(tt), C.byref(m)))
        return {"bytes": b.value, "tiles": t.value, "tiles_total": tt.value, "mode": UPLOAD_NAMES[m.value]}

    def patch_stats(self):
        """k_patch_step launches of this stream's engine so far and the tiles they wrote (mi355x_h264_stream_debug_patch_stats)"""
        a, b = C.c_uint64(), C.c_uint64()
        self._check(lib().mi355x_h264_stream_debug_patch_stats(self.h, C.byref(a), C.byref(b)))
        return {"launches": a.value, "tiles": b.value}

    def encode_device(self, dev_ptr):
        """one tight picture in the stream's layout, in device memory of the stream's device; read in place"""
        out, n, ft = C.c_void_p(), C.c_uint32(), C.c_int()
        self._check(lib().mi355x_h264_stream_encode_device(self.h, C.c_void_p(dev_ptr), C.byref(out), C.byref(n), C.byref(ft)))
        return C.string_at(out.value, n.value), ft.value

    def encode_nv12(self, nv12, strides=None, damage=None):
        """host NV12 (Y plane then interleaved UV); with strides = (y, uv), nv12 is the two planes as separate arrays"""
        ((y, ys), (uv, uvs)), keep = _planes(nv12, self.src_width, self.src_height, strides, nv12=True)
        out, n, ft = C.c_void_p(), C.c_uint32(), C.c_int()
        if damage is None:
            self._check(lib().mi355x_h264_stream_encode_nv12(self.h, y, ys, uv, uvs, C.byref(out), C.byref(n), C.byref(ft)))
        else:
            rects, nr, keep2 = _damage_args(damage)
            self._check(lib().mi355x_h264_stream_encode_nv12_damage(self.h, y, ys, uv, uvs, rects, nr, C.byref(out), C.byref(n), C.byref(ft)))
        return C.string_at(out.value, n.value), ft.value

    def encode_rgba(self, rgba, stride=None, damage=None):
        """host RGBA (height x width x 4 bytes, or rows `stride` bytes apart)"""
        f = np.ascontiguousarray(rgba, dtype=np.uint8)
        out, n, ft = C.c_void_p(), C.c_uint32(), C.c_int()
        if damage is None:
            self._check(lib().mi355x_h264_stream_encode_rgba(self.h, f.ctypes.data, int(stride or 4 * self.src_width), C.byref(out), C.byref(n), C.byref(ft)))
        else:
            rects, nr, keep2 = _damage_args(damage)
            self._check(lib().mi355x_h264_stream_encode_rgba_damage(self.h, f.ctypes.data, int(stride or 4 * self.src_width), rects, nr, C.byref(out), C.byref(n), C.byref(ft)))
        return C.string_at(out.value, n.value), ft.value

    def last_error(self):
        return lib().mi355x_h264_stream_last_error(self.h).decode()

    @property
    def last_temporal_id(self):
        """temporal layer (0 / 1) of the stream's last finished picture"""
        return lib().mi355x_h264_stream_last_temporal_id(self.h)

    @property
    def last_refresh_band(self):
        """the all-intra band k of the stream's last finished picture; -1 for an IDR picture or with refresh off"""
        return lib().mi355x_h264_stream_last_refresh_band(self.h)

    @property
    def colour(self):
        """the description the stream was opened with, ("bt709", "full") ..., or None"""
        return _colour_read(lib().mi355x_h264_stream_colour, self.h)

    def source_size(self):
        """(width, height) of the pictures the calls take (mi355x_h264_stream_source_width / _height)"""
        return lib().mi355x_h264_stream_source_width(self.h), lib().mi355x_h264_stream_source_height(self.h)

    def set_qp(self, qp):
        self._check(lib().mi355x_h264_stream_set_qp(self.h, qp))

    def force_idr(self):
        self._check(lib().mi355x_h264_stream_force_idr(self.h))

    def me_cost(self):
        c = C.c_uint32()
        self._check(lib().mi355x_h264_stream_last_me_cost(self.h, C.byref(c)))
        return c.value

    def recon(self, p):
        n = self.cw * self.ch // (4 if p else 1)
        a = np.zeros(n, np.uint8)
        got = lib().mi355x_h264_stream_debug_read(self.h, DBG_RECON_Y + p, a.ctypes.data, a.size)
        if got != n:
            raise EncoderError("stream_debug_read -> %d" % got)
        return a.reshape(self.ch // (2 if p else 1), self.cw // (2 if p else 1))

    def debug_read(self, what):
        """as Encoder.debug_read, of this stream's last picture (DBG_PRE_* after keep_pre)"""
        return _debug_read(self, lib().mi355x_h264_stream_debug_read, what)

    def keep_pre(self, on=True):
        """keep the pre-filter planes of every stream of this stream's engine (mi355x_h264_stream_debug_keep_pre)"""
        self._check(lib().mi355x_h264_stream_debug_keep_pre(self.h, int(on)))

    def quality_enable(self, on=True, ssim=False):
        """the quality report for every stream of this stream's engine (mi355x_h264_stream_quality_enable); ssim: SSIM beside the
        SSE (mi355x_h264_stream_quality_enable_ex with both metrics)"""
        if on and ssim:
            self._check(lib().mi355x_h264_stream_quality_enable_ex(self.h, QUALITY_SSE | QUALITY_SSIM))
        else:
            self._check(lib().mi355x_h264_stream_quality_enable(self.h, int(on)))

    def quality(self):
        """the record of this stream's last picture, `psnr` added; raises EncoderError (rc = E_ARG) when there is none"""
        q = Quality()
        self._check(lib().mi355x_h264_stream_last_quality(self.h, C.byref(q)))
        rec, s = _quality_record(q), Ssim()
        # (the switch belongs to the shared engine, so another stream may have asked for SSIM: the record says whether there is one)
        if lib().mi355x_h264_stream_last_ssim(self.h, C.byref(s)) == 0:
            rec = _with_ssim(rec, s)
        return rec

    def ssim_map(self):
        """the sum of q over the luma windows whose origin lies in the macroblock, of this stream's last picture: int32 (rows, columns)"""
        m = np.zeros((self.ch // 16, self.cw // 16), np.int32)
        got = lib().mi355x_h264_stream_ssim_map(self.h, m.ctypes.data, m.size)
        if got < 0:
            self._check(int(got))
        return m

    def quality_map(self):
        """SSE per macroblock of this stream's last picture: uint32 (rows, columns)"""
        m = np.zeros((self.ch // 16, self.cw // 16), np.uint32)
        got = lib().mi355x_h264_stream_quality_map(self.h, m.ctypes.data, m.size)
        if got < 0:
            self._check(int(got))
        return m

    def mem_check(self):
        """(damaged regions, regions examined, report lines) of the hub's blocks and the shared engine's"""
        return _mem_check(lib().mi355x_h264_stream_debug_mem_check, self.h, self.last_error)

    def last_step(self):
        """the lockstep step that coded this stream's last picture (mi355x_h264_stream_debug_last_step)"""
        ser, n, pos, idr = C.c_uint64(), C.c_int(), C.c_int(), C.c_int()
        self._check(lib().mi355x_h264_stream_debug_last_step(self.h, C.byref(ser), C.byref(n), C.byref(pos), C.byref(idr)))
        return {"serial": ser.value, "pictures": n.value, "position": pos.value, "idr": bool(idr.value)}

    def hub_stats(self):
        st, pc, mx, op = C.c_uint64(), C.c_uint64(), C.c_uint64(), C.c_int()
        self._check(lib().mi355x_h264_stream_hub_stats(self.h, C.byref(st), C.byref(pc), C.byref(mx), C.byref(op)))
        return {"steps": st.value, "pictures": pc.value, "max_batch": mx.value, "open_streams": op.value}

    def close(self):
        if getattr(self, "h", None):
            lib().mi355x_h264_stream_close(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
