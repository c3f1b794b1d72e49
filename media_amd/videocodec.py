"""ctypes driver of the C++ plugin surface (media_amd/lib/libVideoCodec.so) through the
flat shim in media_amd/host/capi_shim.cpp: CreateVideoEncoder -> VideoEncoder virtuals.
Used by tests to exercise the drop-in boundary the way the reference's caller would."""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "libVideoCodec.so")

# EncoderRetCode (include/VideoCodecApi.h)
SUCCESS, CREATE_FAIL, INIT_FAIL, START_FAIL, ENCODE_FAIL, STOP_FAIL, DESTROY_FAIL, REGISTER_FAIL, RESET_FAIL, \
    FORCE_KEY_FRAME_FAIL, SET_ENCODE_PARAMS_FAIL = range(11)

_lib = None


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise OSError("host library missing: %s (run __graft_entry__.build())" % LIB_PATH)
        L = C.CDLL(LIB_PATH)
        vp = C.c_void_p
        L.vc_create.argtypes = [C.POINTER(vp)]
        for n in ("vc_delete", "vc_init", "vc_start", "vc_stop", "vc_reset"):
            getattr(L, n).argtypes = [vp]
            getattr(L, n).restype = C.c_uint32
        L.vc_create.restype = C.c_uint32
        L.vc_destroy.argtypes = [vp]
        L.vc_destroy.restype = None
        L.vc_encode.argtypes = [vp, vp, C.c_uint32, C.POINTER(vp), C.POINTER(C.c_uint32)]
        L.vc_encode.restype = C.c_uint32
        L.vc_encode_addr.argtypes = [vp, C.c_uint64, C.c_uint32, C.POINTER(vp), C.POINTER(C.c_uint32)]
        L.vc_encode_addr.restype = C.c_uint32
        L.vc_parse_input_layout.argtypes = [C.c_char_p]
        L.vc_parse_input_device.argtypes = [C.c_char_p]
        L.vc_parse_refs.argtypes = [C.c_char_p]
        L.vc_parse_temporal_layers.argtypes = [C.c_char_p, C.POINTER(C.c_int32)]
        L.vc_last_temporal_id.argtypes = [vp]
        L.vc_parse_intra_refresh.argtypes = [C.c_char_p, C.c_int32, C.c_int32, C.c_int32, C.c_uint32, C.POINTER(C.c_int32)]
        L.vc_last_refresh_band.argtypes = [vp]
        L.vc_parse_damage.argtypes = [C.c_char_p]
        L.vc_set_next_damage.argtypes = [vp, C.POINTER(C.c_int32), C.c_int32]
        L.vc_last_upload.argtypes = [vp, C.POINTER(C.c_uint64), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(C.c_int32)]
        L.vc_parse_psnr.argtypes = [C.c_char_p]
        L.vc_parse_ssim.argtypes = [C.c_char_p]
        L.vc_last_ssim.argtypes = [vp, vp]
        L.vc_debug_quality_metrics_ok.argtypes = [C.c_uint32]
        L.vc_debug_quality_env.argtypes = [C.c_char_p]
        L.vc_debug_quality_env.restype = C.c_uint32
        L.vc_parse_source_size.argtypes = [C.c_char_p, C.c_char_p, C.c_uint32, C.c_uint32, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
        L.vc_last_quality.argtypes = [vp, vp]
        L.vc_debug_ref_counts.argtypes = [C.c_int32, C.c_int32, C.c_char_p, C.c_int32, C.POINTER(C.c_int32)]
        L.vc_debug_ref_counts.restype = None
        L.vc_last_qp.argtypes = [vp]
        i32p = C.POINTER(C.c_int32)
        L.vc_parse_colour.argtypes = [C.c_char_p, C.c_char_p, i32p, i32p]
        L.vc_colour.argtypes = [vp, i32p, i32p]
        L.vc_debug_parameter_sets.argtypes = [i32p, vp, C.c_int32]
        L.vc_debug_level.argtypes = [C.c_int32, C.c_int32]
        L.vc_scene_cuts.argtypes = [vp]
        L.vc_scene_cuts.restype = C.c_uint32
        L.vc_debug_recon_y.argtypes = [vp, vp, C.c_uint64, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
        L.vc_debug_recon_y.restype = C.c_int64
        L.vc_prop_set.argtypes = [C.c_char_p, C.c_char_p]
        L.vc_prop_set.restype = None
        L.vc_prop_get_int.argtypes = [C.c_char_p]
        L.vc_prop_get_str.argtypes = [C.c_char_p, C.c_char_p, C.c_int32]
        _lib = L
    return _lib


def prop_set(key, value):
    lib().vc_prop_set(key.encode(), str(value).encode())


def prop_get(key):
    buf = C.create_string_buffer(256)
    lib().vc_prop_get_str(key.encode(), buf, 256)
    return buf.value.decode()


def parse_input_layout(value):
    """what persist.vmi.video.encode.input = value selects: 0 I420, 1 NV12, 2 RGBA"""
    return lib().vc_parse_input_layout(str(value).encode())


def parse_input_device(value):
    """does persist.vmi.video.encode.inputmem = value select device memory?"""
    return bool(lib().vc_parse_input_device(str(value).encode()))


def parse_refs(value):
    """what persist.vmi.video.encode.refs = value selects: 2 or 3 reference pictures, else 1"""
    return lib().vc_parse_refs(str(value).encode())


def parse_temporal_layers(value):
    """what persist.vmi.video.encode.temporallayers = value selects: (layers, is the value junk?) - 2 for "2", 1 for "1" and for
    the unset key, 1 with the junk mark (one WARN line) for anything else"""
    junk = C.c_int32()
    n = lib().vc_parse_temporal_layers(str(value).encode(), C.byref(junk))
    return n, bool(junk.value)


def parse_intra_refresh(value, slices=0, refs=0, layers=1, height=1080):
    """what persist.vmi.video.encode.intrarefresh = value selects beside the other keys: (bands, one WARN line?) - n for a decimal
    2..32 the picture divides into that conflicts with nothing, 0 for the unset key, 0 with the mark for anything else"""
    warn = C.c_int32()
    n = lib().vc_parse_intra_refresh(str(value).encode(), slices, refs, layers, height, C.byref(warn))
    return n, bool(warn.value)


def parse_damage(value):
    """what persist.vmi.video.encode.damage = value selects: 1 for "detect", 0 for "off" and the unset key, -1 for anything else (one
    WARN line, "off" written back)"""
    return lib().vc_parse_damage(str(value).encode())


def parse_ssim(value):
    """does persist.vmi.video.encode.ssim = value turn the quality report on with both metrics?  "1" only"""
    return bool(lib().vc_parse_ssim(str(value).encode()))


def quality_metrics_ok(metrics):
    """does mi355x_h264_quality_enable_ex take `metrics`?  (the library's own rule, no device)"""
    return bool(lib().vc_debug_quality_metrics_ok(metrics))


def quality_env(value):
    """the metrics MI355X_H264_QUALITY = value turns on when an engine is created (None: the variable is not set)"""
    return int(lib().vc_debug_quality_env(None if value is None else str(value).encode()))


def parse_psnr(value):
    """does persist.vmi.video.encode.psnr = value turn the quality report on?  "1" only"""
    return bool(lib().vc_parse_psnr(str(value).encode()))


def parse_source_size(width, height, coded_width, coded_height):
    """what persist.vmi.video.encode.srcwidth = width and .srcheight = height select at a coded size: (SW, SH) when both are
    decimal numbers, even, 16 .. 4096, at least the coded size and at most 4 times it; None when neither key is set; False for
    anything else (the reference's behaviour, with a WARN line)"""
    sw, sh = C.c_int32(), C.c_int32()
    rc = lib().vc_parse_source_size(str(width).encode(), str(height).encode(), coded_width, coded_height, C.byref(sw), C.byref(sh))
    return (sw.value, sh.value) if rc > 0 else None if rc == 0 else False


def parse_colour(colour, rng):
    """what persist.vmi.video.encode.colour = colour and .range = rng select: (matrix code, full_range) when either is set and both
    are valid ("bt601" | "bt709", "limited" | "full"; the absent one: bt601 / limited); None when neither is set; False for
    anything else (the reference's behaviour, with a WARN line)"""
    m, f = C.c_int32(), C.c_int32()
    rc = lib().vc_parse_colour(str(colour).encode(), str(rng).encode(), C.byref(m), C.byref(f))
    return (m.value, f.value) if rc > 0 else None if rc == 0 else False


def parameter_sets(profile_idc, nrefs, width, height, fps=30, slices=1, disable_deblock=0, colour=None, chroma_loc=False):
    """the Annex-B SPS + PPS the library writes for such a stream, from the host code alone (media_amd/csrc/host_framing.h through
    the shim; no device): colour = (matrix code, full_range) for a described stream, chroma_loc for one of RGBA input"""
    import numpy as np
    mbw, mbh = (width + 15) // 16, (height + 15) // 16
    level = lib().vc_debug_level(mbw * mbh, fps)
    shape = (C.c_int32 * 14)(profile_idc, level, nrefs, mbw, mbh, width, height, slices, disable_deblock,
                             0 if colour is None else 1, 6 if colour is None else colour[0], 0 if colour is None else colour[1], int(bool(chroma_loc)), fps)
    buf = np.zeros(512, np.uint8)
    n = lib().vc_debug_parameter_sets(shape, buf.ctypes.data, buf.size)
    if n < 0:
        raise RuntimeError("parameter sets larger than %d bytes" % buf.size)
    return buf[:n].tobytes()


def ref_counts(nrefs, gop, n, forced=()):
    """the number of reference pictures of each of n pictures of a stream that searches nrefs, IDR every gop pictures and at the
    pictures in `forced` (the rule the engine and the stream hub share; 0 = an IDR picture)"""
    force = bytes(1 if i in forced else 0 for i in range(n))
    out = (C.c_int32 * n)()
    lib().vc_debug_ref_counts(nrefs, gop, force, n, out)
    return list(out)


def set_video_mode(width, height, fps=30, bitrate=5000000, gop=30, profile="baseline", fmt=3, qp=None, slices=None, input=None,
                   inputmem=None, refs=None, psnr=None, ssim=None, shared=None, srcwidth=None, srcheight=None, colour=None, range=None,
                   temporallayers=None, intrarefresh=None, damage=None):
    """fill the property store the way a 'video' mode cloud phone would"""
    prop_set("ro.vmi.demo.video.encode.format", fmt)
    prop_set("ro.sys.vmi.cloudphone", "video")
    prop_set("ro.hardware.width", width)
    prop_set("ro.hardware.height", height)
    prop_set("ro.hardware.fps", fps)
    prop_set("persist.vmi.video.encode.bitrate", bitrate)
    prop_set("persist.vmi.video.encode.gopsize", gop)
    prop_set("persist.vmi.video.encode.profile", profile)
    prop_set("persist.vmi.video.encode.param_adjusting", "0")
    prop_set("persist.vmi.video.encode.keyframe", "0")
    prop_set("persist.vmi.video.encode.qp", "" if qp is None else qp)
    prop_set("persist.vmi.video.encode.scenedetect", "1")
    prop_set("persist.vmi.video.encode.slices", "" if slices is None else slices)
    prop_set("persist.vmi.video.encode.input", "" if input is None else input)        # nv12 | rgba; else I420
    prop_set("persist.vmi.video.encode.inputmem", "" if inputmem is None else inputmem)   # device; else host memory
    prop_set("persist.vmi.video.encode.refs", "" if refs is None else refs)               # 2 | 3; else one reference picture
    prop_set("persist.vmi.video.encode.psnr", "" if psnr is None else psnr)               # 1: quality report; else off
    prop_set("persist.vmi.video.encode.ssim", "" if ssim is None else ssim)               # 1: the report with SSIM beside the SSE
    prop_set("persist.vmi.video.encode.srcwidth", "" if srcwidth is None else srcwidth)   # both set and valid: pictures of that
    prop_set("persist.vmi.video.encode.srcheight", "" if srcheight is None else srcheight)   # size, resampled to width x height
    prop_set("persist.vmi.video.encode.colour", "" if colour is None else colour)         # bt601 | bt709 } either one set and valid: a
    prop_set("persist.vmi.video.encode.range", "" if range is None else range)            # limited | full } described stream
    prop_set("persist.vmi.video.encode.temporallayers", "" if temporallayers is None else temporallayers)   # 2: two temporal layers
    prop_set("persist.vmi.video.encode.intrarefresh", "" if intrarefresh is None else intrarefresh)       # n: intra refresh, n bands
    prop_set("persist.vmi.video.encode.damage", "" if damage is None else damage)                         # detect: damage tiles; else off
    if shared is not None:
        prop_set("persist.vmi.video.encode.shared", shared)                               # 0: an engine of its own; else a stream


class VideoEncoder:
    """Create -> Init -> Start -> Encode x N -> Stop -> Destroy -> delete"""

    def __init__(self):
        self.h = C.c_void_p()
        self.rc_create = lib().vc_create(C.byref(self.h))

    def init(self):
        return lib().vc_init(self.h)

    def start(self):
        return lib().vc_start(self.h)

    def encode(self, data, size=None):
        import numpy as np
        a = np.ascontiguousarray(data, dtype=np.uint8)
        out, n = C.c_void_p(), C.c_uint32()
        rc = lib().vc_encode(self.h, a.ctypes.data, a.size if size is None else size, C.byref(out), C.byref(n))
        return rc, (C.string_at(out.value, n.value) if rc == SUCCESS else b"")

    def encode_addr(self, addr, size):
        """inputData = an address (a picture in device memory, persist.vmi.video.encode.inputmem = device), inputSize = size"""
        out, n = C.c_void_p(), C.c_uint32()
        rc = lib().vc_encode_addr(self.h, addr, size, C.byref(out), C.byref(n))
        return rc, (C.string_at(out.value, n.value) if rc == SUCCESS else b"")

    def stop(self):
        return lib().vc_stop(self.h)

    def destroy(self):
        lib().vc_destroy(self.h)

    def reset(self):
        return lib().vc_reset(self.h)

    def last_qp(self):
        return lib().vc_last_qp(self.h)

    def last_quality(self):
        """the quality record of the last picture that went out (persist.vmi.video.encode.psnr = 1) as capi.Encoder.quality() gives
        them, or None when there is none"""
        from media_amd import capi
        q = capi.Quality()
        if lib().vc_last_quality(self.h, C.byref(q)) != 0:
            return None
        return capi._quality_record(q)

    def last_ssim(self):
        """the SSIM record of the last picture that went out (persist.vmi.video.encode.ssim = 1) as a dict of `ssim`, `ssim_sum`,
        `ssim_windows` and `valid`, or None when there is none"""
        from media_amd import capi
        s = capi.Ssim()
        if lib().vc_last_ssim(self.h, C.byref(s)) != 0:
            return None
        return capi._with_ssim({"valid": bool(s.valid)}, s)

    def last_temporal_id(self):
        """temporal layer (0 / 1) of the last picture that went out (persist.vmi.video.encode.temporallayers = 2); -1 before the first"""
        return lib().vc_last_temporal_id(self.h)

    def last_refresh_band(self):
        """the all-intra band of the last picture that went out (persist.vmi.video.encode.intrarefresh = n); -1: none"""
        return lib().vc_last_refresh_band(self.h)

    def set_next_damage(self, rects):
        """VideoEncoderMI355X::SetNextDamage: [(x, y, w, h), ...] for the next picture only; True when taken"""
        flat = [int(v) for r in rects for v in r]
        arr = (C.c_int32 * max(1, len(flat)))(*flat)
        return lib().vc_set_next_damage(self.h, arr if rects else None, len(rects)) == 1

    def last_upload(self):
        """mi355x_h264_stream_last_upload of the object's stream as capi.Stream.last_upload gives it; None with an engine of its own"""
        from media_amd import capi
        b, t, tt, m = C.c_uint64(), C.c_uint32(), C.c_uint32(), C.c_int32()
        if lib().vc_last_upload(self.h, C.byref(b), C.byref(t), C.byref(tt), C.byref(m)) != 0:
            return None
        return {"bytes": b.value, "tiles": t.value, "tiles_total": tt.value, "mode": capi.UPLOAD_NAMES[m.value]}

    def scene_cuts(self):
        return lib().vc_scene_cuts(self.h)

    def colour(self):
        """(matrix code, full_range) the engine was opened with (persist.vmi.video.encode.colour / .range), or None"""
        m, f = C.c_int32(), C.c_int32()
        return (m.value, f.value) if lib().vc_colour(self.h, C.byref(m), C.byref(f)) == 1 else None

    def recon_y(self):
        """luma reconstruction of the last picture, coded size (measurement hook)"""
        import numpy as np
        cw, ch = C.c_int32(0), C.c_int32(0)
        buf = np.zeros(4096 * 4096, np.uint8)
        n = lib().vc_debug_recon_y(self.h, buf.ctypes.data, buf.size, C.byref(cw), C.byref(ch))
        if n < 0:
            raise RuntimeError("recon read failed")
        return buf[:n].reshape(ch.value, cw.value)

    def delete(self):
        rc = lib().vc_delete(self.h)
        self.h = C.c_void_p()
        return rc
