"""ctypes binding of the decoder peer's C ABI (include/mi355x_h264_dec.h): `Decoder` (GPU reconstruction; fails loudly without
a device), `DecoderGroup` (the next pictures of up to 64 streams of one coded size decoded in one step) and `Parser` (the host-side CAVLC / header parser alone, usable without a GPU: the CPU tests compare what it
recovers from a stream with the side information of the encoder that wrote it)."""
import ctypes as C
import numpy as np
from .capi import lib, EncoderError, MBINFO_DTYPE, LV_STRIDE, _mem_check, Colour, colour_struct

E_STREAM = -7
PIX_I420, PIX_NV12, PIX_NV21, PIX_RGBA = 0, 1, 2, 3   # output layouts (MI355X_H264_PIX_*)
_bound = False


class OutPic(C.Structure):
    """mi355x_h264_dec_out_pic: where a picture lies in an output (offset -1: the stream has none there)"""
    _fields_ = [("offset", C.c_int64), ("width", C.c_int32), ("height", C.c_int32), ("stride", C.c_int32), ("chroma_stride", C.c_int32),
                ("fresh", C.c_int32), ("colour", C.c_int32), ("serial", C.c_int64)]

    def as_dict(self):
        """(colour: matrix | full_range << 8 of the RGBA conversion that was applied; 0 for the other layouts)"""
        return {k: getattr(self, k) for k, _ in self._fields_}


COLOUR = ("described", "matrix", "full_range", "primaries", "transfer", "chroma_loc", "fps", "reorder")   # out[8] of mi355x_h264_dec_colour


def _colour_dict(fn, *args):
    v = (C.c_int32 * 8)()
    rc = fn(*args, v)
    if rc != 0:
        raise EncoderError("colour -> %d (no picture decoded yet?)" % rc)
    return dict(zip(COLOUR, list(v)))


def _set_rgba_colour(fn, colour, *args):
    c = colour_struct(colour)
    rc = fn(*args, None if c is None else C.byref(c))
    if rc != 0:
        err = EncoderError("set_rgba_colour(%r) -> %d" % (colour, rc))
        err.rc = rc
        raise err


def _bind():
    global _bound
    L = lib()
    if _bound:
        return L
    vp, sz, ip = C.c_void_p, C.c_size_t, C.POINTER(C.c_int)
    L.mi355x_h264_dec_create.argtypes = [C.c_int, C.POINTER(vp)]
    L.mi355x_h264_dec_destroy.argtypes = [vp]; L.mi355x_h264_dec_destroy.restype = None
    L.mi355x_h264_dec_last_error.argtypes = [vp]; L.mi355x_h264_dec_last_error.restype = C.c_char_p
    L.mi355x_h264_dec_decode.argtypes = [vp, vp, sz, ip]
    L.mi355x_h264_dec_picture_info.argtypes = [vp, ip, ip, ip, ip]
    L.mi355x_h264_dec_read_i420.argtypes = [vp, vp, sz]; L.mi355x_h264_dec_read_i420.restype = C.c_int64
    L.mi355x_h264_dec_read_i420_device.argtypes = [vp, vp, sz]; L.mi355x_h264_dec_read_i420_device.restype = C.c_int64
    L.mi355x_h264_dec_debug_plane.argtypes = [vp, C.c_int, vp, sz]; L.mi355x_h264_dec_debug_plane.restype = C.c_int64
    L.mi355x_h264_dec_sync.argtypes = [vp]
    L.mi355x_h264_dec_timing.argtypes = [vp, C.POINTER(C.c_uint64), C.POINTER(C.c_double), C.POINTER(C.c_double)]
    L.mi355x_h264_dec_last_step.argtypes = [vp, C.POINTER(C.c_int64), C.c_int]
    L.mi355x_h264_parser_create.restype = vp
    L.mi355x_h264_parser_destroy.argtypes = [vp]; L.mi355x_h264_parser_destroy.restype = None
    L.mi355x_h264_parser_parse.argtypes = [vp, vp, sz]
    L.mi355x_h264_parser_error.argtypes = [vp]; L.mi355x_h264_parser_error.restype = C.c_char_p
    L.mi355x_h264_parser_info.argtypes = [vp, C.POINTER(C.c_int32), C.c_int]
    L.mi355x_h264_parser_read.argtypes = [vp, C.c_int, vp, sz]; L.mi355x_h264_parser_read.restype = C.c_int64
    L.mi355x_h264_dec_group_create.argtypes = [C.c_int, C.c_int, C.POINTER(vp)]
    L.mi355x_h264_dec_group_destroy.argtypes = [vp]; L.mi355x_h264_dec_group_destroy.restype = None
    L.mi355x_h264_dec_group_decode.argtypes = [vp, vp, vp, ip, ip]
    L.mi355x_h264_dec_group_sync.argtypes = [vp]
    L.mi355x_h264_dec_group_last_error.argtypes = [vp, C.c_int]; L.mi355x_h264_dec_group_last_error.restype = C.c_char_p
    L.mi355x_h264_dec_group_picture_info.argtypes = [vp, C.c_int, ip, ip, ip, ip]
    L.mi355x_h264_dec_group_read_i420.argtypes = [vp, C.c_int, vp, sz]; L.mi355x_h264_dec_group_read_i420.restype = C.c_int64
    L.mi355x_h264_dec_group_read_i420_device.argtypes = [vp, C.c_int, vp, sz]; L.mi355x_h264_dec_group_read_i420_device.restype = C.c_int64
    L.mi355x_h264_dec_group_debug_plane.argtypes = [vp, C.c_int, C.c_int, vp, sz]; L.mi355x_h264_dec_group_debug_plane.restype = C.c_int64
    L.mi355x_h264_dec_group_last_step.argtypes = [vp, C.POINTER(C.c_int64), C.c_int]
    op = C.POINTER(OutPic)
    L.mi355x_h264_dec_read.argtypes = [vp, C.c_int, C.c_int, vp, sz, C.c_int, op]; L.mi355x_h264_dec_read.restype = C.c_int64
    L.mi355x_h264_dec_group_read_all.argtypes = [vp, C.c_int, C.c_int, vp, sz, C.c_int, op]; L.mi355x_h264_dec_group_read_all.restype = C.c_int64
    L.mi355x_h264_dec_group_set_output.argtypes = [vp, C.c_int, C.c_int]
    L.mi355x_h264_dec_group_output.argtypes = [vp, C.c_int, C.POINTER(vp), op]
    if hasattr(L, "mi355x_h264_dec_colour"):   # (an A/B library of an earlier build, MI355X_H264_LIB, has no colour descriptions)
        i8, cp = C.POINTER(C.c_int32), C.POINTER(Colour)
        L.mi355x_h264_dec_colour.argtypes = [vp, i8]
        L.mi355x_h264_dec_set_rgba_colour.argtypes = [vp, cp]
        L.mi355x_h264_dec_group_colour.argtypes = [vp, C.c_int, i8]
        L.mi355x_h264_dec_group_set_rgba_colour.argtypes = [vp, C.c_int, cp]
        L.mi355x_h264_parser_colour.argtypes = [vp, i8, C.c_int]
    if hasattr(L, "mi355x_h264_dec_set_output_size"):   # (likewise: an earlier build delivers at the native size only)
        L.mi355x_h264_dec_set_output_size.argtypes = [vp, C.c_int, C.c_int]
        L.mi355x_h264_dec_output_size.argtypes = [vp, ip, ip]
        L.mi355x_h264_dec_group_set_output_size.argtypes = [vp, C.c_int, C.c_int, C.c_int]
        L.mi355x_h264_dec_group_output_size.argtypes = [vp, C.c_int, ip, ip]
    if hasattr(L, "mi355x_h264_dec_set_loss_mode"):   # (likewise: an earlier build is strict)
        i6 = C.POINTER(C.c_int32)
        L.mi355x_h264_dec_set_loss_mode.argtypes = [vp, C.c_int]
        L.mi355x_h264_dec_damage.argtypes = [vp, i6]
        L.mi355x_h264_dec_damage_map.argtypes = [vp, vp, sz]; L.mi355x_h264_dec_damage_map.restype = C.c_int64
        L.mi355x_h264_dec_group_set_loss_mode.argtypes = [vp, C.c_int, C.c_int]
        L.mi355x_h264_dec_group_damage.argtypes = [vp, C.c_int, i6]
        L.mi355x_h264_dec_group_damage_map.argtypes = [vp, C.c_int, vp, sz]; L.mi355x_h264_dec_group_damage_map.restype = C.c_int64
        L.mi355x_h264_parser_set_loss_mode.argtypes = [vp, C.c_int]
        L.mi355x_h264_parser_loss.argtypes = [vp, i6]
    _bound = True
    return L


LOSS_STRICT, LOSS_CONCEAL = 0, 1   # MI355X_H264_LOSS_*
TAINTED, CONCEALED = 1, 2          # the bits of a damage-map byte
DAMAGE = ("tainted", "concealed", "gap", "recovery_frame_cnt", "since_loss", "joined")   # out[6] of mi355x_h264_dec_damage


def _loss_mode(mode):
    m = {"strict": LOSS_STRICT, "conceal": LOSS_CONCEAL}.get(mode, mode)
    if isinstance(m, str):
        raise ValueError("loss = %r: \"strict\" | \"conceal\"" % (mode,))
    return int(m)


def _set_loss_mode(fn, mode, *args):
    rc = fn(*args, _loss_mode(mode))
    if rc != 0:
        err = EncoderError("set_loss_mode(%r) -> %d" % (mode, rc))
        err.rc = rc
        raise err


def _damage(fn, *args):
    v = (C.c_int32 * 6)()
    rc = fn(*args, v)
    if rc != 0:
        raise EncoderError("damage -> %d" % rc)
    return dict(zip(DAMAGE, list(v)))


def _damage_map(fn, mbw, mbh, *args):
    a = np.empty((mbh, mbw), np.uint8)
    n = fn(*args, a.ctypes.data, a.nbytes)
    if n != a.nbytes:
        raise EncoderError("damage_map -> %d" % n)
    return a


def _set_output_size(fn, w, h, *args):
    rc = fn(*args, int(w), int(h))
    if rc != 0:
        err = EncoderError("set_output_size(%r, %r) -> %d (even, 2..4096, or 0, 0 for the native size)" % (w, h, rc))
        err.rc = rc
        raise err


def _output_size(fn, *args):
    w, h = C.c_int(0), C.c_int(0)
    rc = fn(*args, C.byref(w), C.byref(h))
    if rc != 0:
        raise EncoderError("output_size -> %d" % rc)
    return w.value, h.value


def _tensor_ready(tensor):
    """the gather kernel runs on the decoder's own stream, which does not wait for the default stream: whatever torch has queued
    on the tensor's device (the fill that made the tensor, say) must be complete before the kernel writes into it"""
    import torch
    torch.cuda.synchronize(tensor.device)


def _pic_bytes(p, layout):
    """bytes of a picture of an output in `layout` from its descriptor (include/mi355x_h264_dec.h states the packing)"""
    chroma_planes = {PIX_I420: 2, PIX_NV12: 1, PIX_NV21: 1, PIX_RGBA: 0}[layout]
    return p["stride"] * p["height"] + chroma_planes * p["chroma_stride"] * (p["height"] // 2)


class StreamError(EncoderError):
    """the access unit is damaged or outside the supported feature set"""


class Decoder:
    def __init__(self, device=0, loss="strict"):
        L = _bind()
        self.h = C.c_void_p()
        rc = L.mi355x_h264_dec_create(device, C.byref(self.h))
        if rc != 0:
            raise EncoderError("mi355x_h264_dec_create -> %d (no HIP device? there is no CPU reconstruction path)" % rc)
        if _loss_mode(loss) != LOSS_STRICT:
            self.set_loss_mode(loss)

    def set_loss_mode(self, mode):
        """"strict" (refuse what is damaged or missing, wait for an IDR picture) or "conceal" (include/mi355x_h264_dec.h, "loss mode")"""
        _set_loss_mode(lib().mi355x_h264_dec_set_loss_mode, mode, self.h)

    def damage(self):
        """what is known about the last picture: a dict of DAMAGE (tainted == 0: the picture is exact)"""
        return _damage(lib().mi355x_h264_dec_damage, self.h)

    def damage_map(self):
        """(mbh, mbw) bytes of the last picture: TAINTED | CONCEALED per macroblock"""
        _, _, cw, ch = self.info()
        return _damage_map(lib().mi355x_h264_dec_damage_map, cw // 16, ch // 16, self.h)

    def close(self):
        if self.h:
            lib().mi355x_h264_dec_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def decode(self, au):
        """one access unit (bytes); True when a picture was decoded"""
        got = C.c_int(0)
        buf = (C.c_uint8 * len(au)).from_buffer_copy(au)
        rc = lib().mi355x_h264_dec_decode(self.h, buf, len(au), C.byref(got))
        if rc != 0:
            msg = lib().mi355x_h264_dec_last_error(self.h).decode()
            raise (StreamError if rc == E_STREAM else EncoderError)("decode -> %d: %s" % (rc, msg))
        return bool(got.value)

    def info(self):
        v = [C.c_int(0) for _ in range(4)]
        if lib().mi355x_h264_dec_picture_info(self.h, *[C.byref(x) for x in v]) != 0:
            raise EncoderError("no picture decoded yet")
        return tuple(x.value for x in v)   # width, height, coded width, coded height

    def i420(self):
        w, h, _, _ = self.info()
        a = np.empty(w * h * 3 // 2, np.uint8)
        n = lib().mi355x_h264_dec_read_i420(self.h, a.ctypes.data, a.nbytes)
        if n != a.nbytes:
            raise EncoderError("read_i420 -> %d" % n)
        return a

    def i420_device(self, ptr, cap):
        return lib().mi355x_h264_dec_read_i420_device(self.h, ptr, cap)

    def read(self, layout, row_align=1, device_tensor=None):
        """the last picture in `layout` (PIX_*): (buffer, pic).  buffer is a numpy array of exactly the bytes used, or - with a
        torch uint8 tensor in device memory - that tensor, written in place (bytes used: pic["bytes"])"""
        pic = OutPic()
        need = lib().mi355x_h264_dec_read(self.h, layout, row_align, None, 0, 0, C.byref(pic))
        if need < 0:
            err = EncoderError("dec_read(layout %d, row_align %d) -> %d: %s" % (layout, row_align, need, lib().mi355x_h264_dec_last_error(self.h).decode()))
            err.rc = need
            raise err
        if device_tensor is None:
            buf = np.empty(need, np.uint8)
            n = lib().mi355x_h264_dec_read(self.h, layout, row_align, buf.ctypes.data, buf.nbytes, 0, C.byref(pic))
        else:
            buf = device_tensor
            _tensor_ready(buf)
            n = lib().mi355x_h264_dec_read(self.h, layout, row_align, buf.data_ptr(), buf.numel() * buf.element_size(), 1, C.byref(pic))
        if n != need:
            raise EncoderError("dec_read -> %d: %s" % (n, lib().mi355x_h264_dec_last_error(self.h).decode()))
        return buf, dict(pic.as_dict(), bytes=n)

    def set_output_size(self, w, h):
        """pictures are delivered by read() at w x h, resampled on the GPU, from the next read on (the same picture may be read
        at several sizes); 0, 0: at their own size again.  info(), i420() and plane() stay at the native size"""
        _set_output_size(lib().mi355x_h264_dec_set_output_size, w, h, self.h)

    def output_size(self):
        """(w, h) as set; (0, 0): the native size"""
        return _output_size(lib().mi355x_h264_dec_output_size, self.h)

    def colour(self):
        """what the sequence parameter set of the last picture says (mi355x_h264_dec_colour): a dict of COLOUR"""
        return _colour_dict(lib().mi355x_h264_dec_colour, self.h)

    def set_rgba_colour(self, colour):
        """RGBA output applies this variant from the next read on, whatever the stream says: ("bt709", "full") ...; None: follow
        the stream again"""
        _set_rgba_colour(lib().mi355x_h264_dec_set_rgba_colour, colour, self.h)

    def plane(self, p):
        """coded-size plane p of the last picture"""
        _, _, cw, ch = self.info()
        a = np.empty((ch // (2 if p else 1), cw // (2 if p else 1)), np.uint8)
        n = lib().mi355x_h264_dec_debug_plane(self.h, p, a.ctypes.data, a.nbytes)
        if n != a.nbytes:
            raise EncoderError("debug_plane -> %d" % n)
        return a

    def sync(self):
        """wait for the picture the last decode() launched"""
        rc = lib().mi355x_h264_dec_sync(self.h)
        if rc != 0:
            raise EncoderError("dec_sync -> %d: %s" % (rc, lib().mi355x_h264_dec_last_error(self.h).decode()))

    def mem_check(self):
        """(damaged regions, regions examined, report lines): mi355x_h264_dec_debug_mem_check (the guard mode of mi355x_h264.h)"""
        return _mem_check(lib().mi355x_h264_dec_debug_mem_check, self.h, lambda: lib().mi355x_h264_dec_last_error(self.h).decode())

    def last_step(self):
        """DecoderGroup.last_step() of the group of one stream behind this decoder"""
        v = (C.c_int64 * len(DecoderGroup.STEP))()
        n = lib().mi355x_h264_dec_last_step(self.h, v, len(v))
        return dict(zip(DecoderGroup.STEP[:n], list(v)[:n]))

    def timing(self):
        n, a, b = C.c_uint64(0), C.c_double(0), C.c_double(0)
        lib().mi355x_h264_dec_timing(self.h, C.byref(n), C.byref(a), C.byref(b))
        return n.value, a.value, b.value


class DecoderGroup:
    """`streams` decoders on one picture store: decode() takes the next access unit of every stream (None: the stream sits this step
    out) and reconstructs all their pictures in one set of transfers and launches"""
    STEP = ("serial", "pictures", "launches", "transfers", "parse_threads", "parse_us", "launch_us", "output_launches", "output_transfers",
            "read_launches", "read_transfers", "device_bytes", "pinned_bytes")

    def __init__(self, streams, device=0, loss=None):
        """loss: None (every stream strict), one mode for all streams, or a list with one mode per stream"""
        L = _bind()
        self.h = C.c_void_p()
        self.streams = streams
        rc = L.mi355x_h264_dec_group_create(device, streams, C.byref(self.h))
        if rc != 0:
            raise EncoderError("mi355x_h264_dec_group_create(%d streams) -> %d" % (streams, rc))
        if loss is not None:
            modes = [loss] * streams if isinstance(loss, (str, int)) else list(loss)
            if len(modes) != streams:
                raise EncoderError("loss: %d modes for %d streams" % (len(modes), streams))
            for i, m in enumerate(modes):
                if _loss_mode(m) != LOSS_STRICT:
                    self.set_loss_mode(i, m)

    def set_loss_mode(self, stream, mode):
        """as Decoder.set_loss_mode, for one stream of the group"""
        _set_loss_mode(lib().mi355x_h264_dec_group_set_loss_mode, mode, self.h, stream)

    def damage(self, stream):
        return _damage(lib().mi355x_h264_dec_group_damage, self.h, stream)

    def damage_map(self, stream):
        _, _, cw, ch = self.info(stream)
        return _damage_map(lib().mi355x_h264_dec_group_damage_map, cw // 16, ch // 16, self.h, stream)

    def close(self):
        if self.h:
            lib().mi355x_h264_dec_group_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def error(self, stream=-1):
        return lib().mi355x_h264_dec_group_last_error(self.h, stream).decode()

    def decode(self, aus):
        """aus: one entry per stream, bytes or None.  Returns [(rc, got)] per stream; raises when the step failed as a whole"""
        if len(aus) != self.streams:
            raise EncoderError("decode() takes %d access units (None for a stream that sits out), got %d" % (self.streams, len(aus)))
        n = self.streams
        keep = [None if a is None else (C.c_uint8 * max(1, len(a))).from_buffer_copy(a if len(a) else b"\0") for a in aus]
        ptrs = (C.c_void_p * n)(*[None if b is None else C.addressof(b) for b in keep])
        lens = (C.c_size_t * n)(*[0 if a is None else len(a) for a in aus])
        got, rc = (C.c_int * n)(), (C.c_int * n)()
        r = lib().mi355x_h264_dec_group_decode(self.h, ptrs, lens, got, rc)
        if r != 0:
            raise EncoderError("group decode -> %d: %s" % (r, self.error()))
        return [(rc[i], got[i]) for i in range(n)]

    def mem_check(self):
        """(damaged regions, regions examined, report lines): mi355x_h264_dec_group_debug_mem_check"""
        return _mem_check(lib().mi355x_h264_dec_group_debug_mem_check, self.h, self.error)

    def mem_poke(self, block, offset, value):
        """one byte of a guard region set from the host (value -1: put back); returns the call's code"""
        return lib().mi355x_h264_dec_group_debug_mem_poke(self.h, block.encode(), int(offset), int(value))

    def sync(self):
        rc = lib().mi355x_h264_dec_group_sync(self.h)
        if rc != 0:
            raise EncoderError("group sync -> %d: %s" % (rc, self.error()))

    def info(self, stream):
        v = [C.c_int(0) for _ in range(4)]
        if lib().mi355x_h264_dec_group_picture_info(self.h, stream, *[C.byref(x) for x in v]) != 0:
            raise EncoderError("stream %d has decoded no picture yet" % stream)
        return tuple(x.value for x in v)   # width, height, coded width, coded height

    def colour(self, stream):
        """what the sequence parameter set of the stream's last picture says (mi355x_h264_dec_group_colour): a dict of COLOUR"""
        return _colour_dict(lib().mi355x_h264_dec_group_colour, self.h, stream)

    def set_rgba_colour(self, stream, colour):
        """as Decoder.set_rgba_colour, for one stream of the group"""
        _set_rgba_colour(lib().mi355x_h264_dec_group_set_rgba_colour, colour, self.h, stream)

    def set_output_size(self, stream, w, h):
        """as Decoder.set_output_size, for one stream of the group (stream = -1: for every stream): what read_all() and the armed
        output() deliver.  A stream whose picture cannot be resampled to its size has offset -1 there, and error(stream) says why"""
        _set_output_size(lib().mi355x_h264_dec_group_set_output_size, w, h, self.h, stream)

    def output_size(self, stream):
        return _output_size(lib().mi355x_h264_dec_group_output_size, self.h, stream)

    def read_i420(self, stream):
        w, h, _, _ = self.info(stream)
        a = np.empty(w * h * 3 // 2, np.uint8)
        n = lib().mi355x_h264_dec_group_read_i420(self.h, stream, a.ctypes.data, a.nbytes)
        if n != a.nbytes:
            raise EncoderError("group read_i420 -> %d" % n)
        return a

    def read_i420_device(self, stream, tensor):
        """into a torch uint8 tensor in device memory; returns the bytes written"""
        n = lib().mi355x_h264_dec_group_read_i420_device(self.h, stream, tensor.data_ptr(), tensor.numel() * tensor.element_size())
        if n < 0:
            raise EncoderError("group read_i420_device -> %d" % n)
        return n

    def debug_planes(self, stream):
        """the three coded-size planes of the stream's last picture"""
        _, _, cw, ch = self.info(stream)
        out = []
        for p in range(3):
            a = np.empty((ch // (2 if p else 1), cw // (2 if p else 1)), np.uint8)
            n = lib().mi355x_h264_dec_group_debug_plane(self.h, stream, p, a.ctypes.data, a.nbytes)
            if n != a.nbytes:
                raise EncoderError("group debug_plane -> %d" % n)
            out.append(a)
        return out

    def last_step(self):
        """the last step; output_launches / output_transfers: what an armed step added (set_output); read_launches /
        read_transfers: what the last read_all call made; device_bytes / pinned_bytes: device and pinned host memory the group holds now"""
        v = (C.c_int64 * len(self.STEP))()
        n = lib().mi355x_h264_dec_group_last_step(self.h, v, len(v))
        return dict(zip(self.STEP[:n], list(v)[:n]))

    def read_all(self, layout, row_align=1, device_tensor=None, out=None):
        """every stream's last picture in one call: (buffer, pics).  buffer: a numpy array of exactly the bytes used (a view of
        `out`, a numpy uint8 array of the caller's that is large enough, when one is given: a fresh array of tens of megabytes
        per call costs more than the transfer), or the torch uint8 device tensor handed in, written in place; pics: one dict
        per stream (offset -1: no picture yet), and the bytes used as self.read_bytes"""
        pics = (OutPic * self.streams)()
        need = lib().mi355x_h264_dec_group_read_all(self.h, layout, row_align, None, 0, 0, pics)
        if need < 0:
            raise EncoderError("group read_all(layout %d, row_align %d) -> %d" % (layout, row_align, need))
        if device_tensor is None:
            buf = np.empty(need, np.uint8) if out is None else out[:need]
            if buf.size != need:
                raise EncoderError("group read_all: `out` holds %d bytes, %d are needed" % (buf.size, need))
            n = lib().mi355x_h264_dec_group_read_all(self.h, layout, row_align, buf.ctypes.data, buf.nbytes, 0, pics)
        else:
            buf = device_tensor
            _tensor_ready(buf)
            n = lib().mi355x_h264_dec_group_read_all(self.h, layout, row_align, buf.data_ptr(), buf.numel() * buf.element_size(), 1, pics)
        if n != need:
            raise EncoderError("group read_all -> %d: %s" % (n, self.error()))
        self.read_bytes = n
        return buf, [p.as_dict() for p in pics]

    def set_output(self, layout, row_align=1):
        """arm the group (layout -1: disarm): every step from the next one on also delivers its pictures in `layout` into one of
        two pinned sets; output() hands them out"""
        rc = lib().mi355x_h264_dec_group_set_output(self.h, layout, row_align)
        if rc != 0:
            raise EncoderError("group set_output(layout %d, row_align %d) -> %d" % (layout, row_align, rc))
        self._armed = layout

    def output(self, back=0):
        """(numpy view of the pinned set, pics) of the last armed step (back = 0: waits for it) or of the one before (back = 1:
        complete already).  The view is valid until the second decode() after that step"""
        pics = (OutPic * self.streams)()
        data = C.c_void_p()
        rc = lib().mi355x_h264_dec_group_output(self.h, back, C.byref(data), pics)
        if rc != 0:
            raise EncoderError("group output(back %d) -> %d: %s" % (back, rc, self.error()))
        out = [p.as_dict() for p in pics]
        used = max([p["offset"] + _pic_bytes(p, self._armed) for p in out if p["offset"] >= 0] + [0])
        view = np.ctypeslib.as_array(C.cast(data, C.POINTER(C.c_uint8)), shape=(max(used, 1),))[:used]
        return view, out


class Parser:
    INFO = ("mbw", "mbh", "width", "height", "idr", "qp", "slice_rows", "deblock_idc", "num_ref_active", "t8x8_mode", "has_pcm", "kinds",
            "cqo_cb", "cqo_cr", "filter_oa", "filter_ob", "one_qp", "ref_age0", "ref_age1", "ref_age2", "is_ref")

    def __init__(self):
        self.h = C.c_void_p(_bind().mi355x_h264_parser_create())

    def close(self):
        if self.h:
            lib().mi355x_h264_parser_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    LOSS = ("concealed", "gap", "joined", "recovery_frame_cnt", "lost")

    def set_loss_mode(self, mode):
        _set_loss_mode(lib().mi355x_h264_parser_set_loss_mode, mode, self.h)

    def loss(self):
        """what the conceal mode did to the last access unit (mi355x_h264_parser_loss): a dict of LOSS"""
        v = (C.c_int32 * 5)()
        if lib().mi355x_h264_parser_loss(self.h, v) != 0:
            raise EncoderError("parser_loss failed")
        return dict(zip(self.LOSS, list(v)))

    def concealed(self):
        """1 per macroblock of the last picture that was filled in (conceal mode)"""
        i = self.info()
        return self._read(8, np.empty(i["mbw"] * i["mbh"], np.uint8))

    def parse(self, au):
        buf = (C.c_uint8 * len(au)).from_buffer_copy(au)
        rc = lib().mi355x_h264_parser_parse(self.h, buf, len(au))
        if rc < 0:
            raise StreamError(lib().mi355x_h264_parser_error(self.h).decode())
        return rc == 1

    def info(self):
        v = (C.c_int32 * 21)()
        lib().mi355x_h264_parser_info(self.h, v, 21)
        return dict(zip(self.INFO, list(v)))

    def colour(self):
        """what the VUI of the active sequence parameter set says (mi355x_h264_parser_colour): a dict of COLOUR, plus `vui` (1: the
        set has a VUI that was read whole and in range) and `dec_buffering` (max_dec_frame_buffering or -1)"""
        v = (C.c_int32 * 10)()
        if lib().mi355x_h264_parser_colour(self.h, v, 10) != 10:
            raise EncoderError("parser_colour failed")
        return dict(zip(COLOUR + ("vui", "dec_buffering"), list(v)))

    def vectors4(self):
        """(vectors of the sixteen 4x4 blocks (n, 16, 2), raster order; ref_idx_l0 of the four quadrants (n, 4), 255 = intra)"""
        i = self.info()
        n = i["mbw"] * i["mbh"]
        return self._read(5, np.empty((n, 16, 2), np.int16)), self._read(6, np.empty((n, 4), np.uint8))

    def mbqp(self):
        """QP_Y of every macroblock of the last picture (0 for I_PCM)"""
        i = self.info()
        return self._read(4, np.empty(i["mbw"] * i["mbh"], np.uint8))

    def mbavail(self):
        """per macroblock of the last picture: the neighbours left, above, above-right, above-left in its slice (bits 0..3) and usable
        for intra prediction (bits 4..7)"""
        i = self.info()
        return self._read(7, np.empty(i["mbw"] * i["mbh"], np.uint8))

    def _read(self, what, arr):
        n = lib().mi355x_h264_parser_read(self.h, what, arr.ctypes.data, arr.nbytes)
        if n != arr.nbytes:
            raise EncoderError("parser_read(%d) -> %d" % (what, n))
        return arr

    def arrays(self):
        i = self.info()
        n = i["mbw"] * i["mbh"]
        return (self._read(0, np.empty(n, MBINFO_DTYPE)), self._read(1, np.empty((n, 8), np.int16)),
                self._read(2, np.empty((n, 16), np.uint8)), self._read(3, np.empty((n, LV_STRIDE), np.int16)))
