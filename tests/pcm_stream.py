"""An access unit whose every macroblock is I_PCM: chosen samples through a real decoder, untouched by prediction, transform or
loop filter (tests/test_value_cube_oracle.py, tests/test_gpu_dec_output_cube.py).  Written from ITU-T H.264 7.3 alone:

  SPS   Baseline (profile_idc 66), pic_order_cnt_type 2, one reference frame, frame_mbs_only_flag 1, optional frame cropping with
        left / right / top / bottom offsets (given in luma samples, even)
  PPS   CAVLC, deblocking_filter_control_present_flag 1
  slice one IDR I slice, frame_num 0, slice_qp_delta 0, disable_deblocking_filter_idc 1
  data  per macroblock: mb_type ue(25) = I_PCM, pcm_alignment_zero_bits, 256 luma + 64 Cb + 64 Cr bytes

The macroblocks are laid out with numpy and the NAL payload is escaped by the oracle's h264o_nal_escape (a 1024x1024 unit is
1.5 MB: no Python loop touches its bytes)."""
import numpy as np

from oracle_lib import lib as oracle, _ptr

START = b"\x00\x00\x00\x01"


class Bits:
    def __init__(self):
        self.b = []

    def u(self, n, v):
        self.b += [(v >> (n - 1 - i)) & 1 for i in range(n)]
        return self

    def ue(self, v):
        n = (v + 1).bit_length()
        return self.u(n - 1, 0).u(n, v + 1)

    def se(self, v):
        return self.ue(2 * v - 1 if v > 0 else -2 * v)

    def align(self, bit=0):
        while len(self.b) % 8:
            self.b.append(bit)
        return self

    def trailing(self):
        self.b.append(1)
        return self.align()

    def bytes(self):
        assert len(self.b) % 8 == 0
        return np.packbits(np.array(self.b, np.uint8)).tobytes()


def escape(rbsp):
    a = np.frombuffer(bytes(rbsp), np.uint8) if not isinstance(rbsp, np.ndarray) else np.ascontiguousarray(rbsp, dtype=np.uint8)
    out = np.empty(a.size + a.size // 2 + 8, np.uint8)
    n = oracle().h264o_nal_escape(_ptr(a), a.size, _ptr(out))
    return out[:n].tobytes()


def sps(mbw, mbh, crop=None, level_idc=40):
    b = Bits().u(8, 66).u(8, 0xC0).u(8, level_idc)   # Baseline, constraint_set0 / 1
    b.ue(0)                                          # seq_parameter_set_id
    b.ue(0)                                          # log2_max_frame_num_minus4
    b.ue(2)                                          # pic_order_cnt_type
    b.ue(1).u(1, 0)                                  # max_num_ref_frames, gaps_in_frame_num_value_allowed_flag
    b.ue(mbw - 1).ue(mbh - 1).u(1, 1).u(1, 1)        # size, frame_mbs_only_flag, direct_8x8_inference_flag
    if crop is None:
        b.u(1, 0)
    else:
        assert all(c >= 0 and c % 2 == 0 for c in crop)
        b.u(1, 1)
        for c in crop:                               # left, right, top, bottom: units of two luma samples (4:2:0 frames)
            b.ue(c // 2)
    b.u(1, 0)                                        # vui_parameters_present_flag
    return b"\x67" + escape(b.trailing().bytes())


def pps():
    b = Bits().ue(0).ue(0).u(1, 0).u(1, 0).ue(0)     # ids, CAVLC, bottom_field_pic_order_in_frame_present_flag, one slice group
    b.ue(0).ue(0).u(1, 0).u(2, 0)                    # default active references, no weighted prediction
    b.se(0).se(0).se(0)                              # pic_init_qp, pic_init_qs, chroma_qp_index_offset
    b.u(1, 1).u(1, 0).u(1, 0)                        # deblocking_filter_control_present_flag, constrained_intra_pred, redundant_pic_cnt
    return b"\x68" + escape(b.trailing().bytes())


def macroblocks(y, u, v):
    """the planes (coded size) as (macroblocks, 384): each macroblock's 256 luma, 64 Cb and 64 Cr samples in raster order"""
    ch, cw = y.shape
    mbh, mbw = ch // 16, cw // 16
    cut = lambda p, n: np.asarray(p, np.uint8).reshape(mbh, n, mbw, n).transpose(0, 2, 1, 3).reshape(mbh * mbw, n * n)
    return np.concatenate([cut(y, 16), cut(u, 8), cut(v, 8)], axis=1)


def idr_slice(y, u, v):
    mbs = macroblocks(y, u, v)
    head = Bits().ue(0).ue(7).ue(0)                  # first_mb_in_slice, slice_type I (all slices), pic_parameter_set_id
    head.u(4, 0).ue(0)                               # frame_num, idr_pic_id
    head.u(1, 0).u(1, 0)                             # no_output_of_prior_pics_flag, long_term_reference_flag
    head.se(0).ue(1)                                 # slice_qp_delta, disable_deblocking_filter_idc
    first = head.ue(25).align().bytes()              # the first macroblock's mb_type and pcm_alignment_zero_bits
    # every other macroblock starts on a byte: ue(25) = 0000 11010, then seven alignment bits = 0x0D 0x00
    body = np.empty((len(mbs), 2 + 384), np.uint8)
    body[:, 0], body[:, 1] = 0x0D, 0x00
    body[:, 2:] = mbs
    rbsp = np.concatenate([np.frombuffer(first, np.uint8), body.reshape(-1)[2:], np.array([0x80], np.uint8)])
    return b"\x65" + escape(rbsp)


def access_unit(y, u, v, crop=None):
    """y (ch, cw), u, v (ch / 2, cw / 2): coded-size planes, multiples of 16; crop = (left, right, top, bottom) in luma samples
    or None.  Returns the Annex-B access unit: SPS, PPS, one IDR slice of I_PCM macroblocks"""
    ch, cw = y.shape
    assert cw % 16 == 0 and ch % 16 == 0 and u.shape == v.shape == (ch // 2, cw // 2)
    return START + sps(cw // 16, ch // 16, crop) + START + pps() + START + idr_slice(y, u, v)


def cropped_unit(planes, cw, ch, left, top, seed):
    """the picture (Y, U, V) of any even size as the cropped picture of a coded cw x ch unit whose other samples are noise:
    (access unit, coded planes)"""
    import value_cube as vcube
    h, w = planes[0].shape
    coded = vcube.embed(planes, cw, ch, left, top, seed)
    return access_unit(*coded, crop=(left, cw - w - left, top, ch - h - top)), coded
