"""slice_header() (7.3.3) of the streams this encoder and the oracle encoder write, read and rewritten bit by bit: shared by
tests/dec_loss.py (loss stand-ins) and tests/deblock_cells.py (re-headed pictures).  The parameter sets of those streams:
log2_max_frame_num 8, pic_order_cnt_type 2, pic_init_qp 26, CAVLC, deblocking_filter_control_present_flag 1, one picture parameter
set (id 0).  Nothing of the decoder under test is used here."""
from collections import namedtuple
import numpy as np
from temporal import Bits, pack, ue_bits, se_bits, escape, unescape

FN_BITS = 8

# qd_pos / end_pos: the bit of the RBSP at which slice_qp_delta starts / at which slice_data() starts
Hdr = namedtuple("Hdr", "nal first_mb slice_type frame_num fn_pos idr ref_idc nact qp idc oa ob qd_pos end_pos")


def read_header(nal):
    """slice_header() of a slice NAL unit (header byte first) as this encoder and the oracle write it"""
    r = Bits(unescape(nal[1:])[:24])
    idr, ref_idc = (nal[0] & 31) == 5, (nal[0] >> 5) & 3
    first, st = r.ue(), r.ue()
    assert r.ue() == 0, "pic_parameter_set_id"
    fn_pos = r.p
    fn = r.u(FN_BITS)
    nact = None
    if idr:
        r.ue()
    if st % 5 == 0:
        if r.u(1):
            nact = r.ue() + 1
        assert r.u(1) == 0, "ref_pic_list_modification_flag_l0"
    if ref_idc:
        r.u(2 if idr else 1)
    qd_pos = r.p
    k = r.ue()
    qp = 26 + ((k + 1) // 2 if k & 1 else -(k // 2))
    idc = r.ue()
    oa = ob = 0
    if idc != 1:
        k = r.ue(); oa = (k + 1) // 2 if k & 1 else -(k // 2)
        k = r.ue(); ob = (k + 1) // 2 if k & 1 else -(k // 2)
    return Hdr(nal[0], first, st, fn, fn_pos, idr, ref_idc, nact, qp, idc, oa, ob, qd_pos, r.p)


def bits_of(nal):
    return np.unpackbits(np.frombuffer(unescape(nal[1:]), np.uint8)).tolist()


def rbsp(nal_hdr, bits):
    """bits up to and including the stop bit, aligned anew"""
    stop = len(bits) - 1 - bits[::-1].index(1)
    b = bits[:stop + 1]
    return bytes([nal_hdr]) + escape(pack(b + [0] * (-len(b) % 8)))


def rehead(nal, qp, idc, oa, ob):
    """the slice NAL unit with another slice_qp_delta (SliceQP_Y = qp), disable_deblocking_filter_idc, slice_alpha_c0_offset_div2
    and slice_beta_offset_div2 (7.3.3); everything in front of slice_qp_delta and all of slice_data() as it was.  CAVLC slice data
    is not aligned, so it may start at any bit - except for pcm_alignment_zero_bit: a slice with an I_PCM macroblock keeps its
    meaning only if the header's length stays the same modulo 8 (the caller's business)"""
    assert 0 <= qp <= 51 and idc in (0, 1, 2) and -6 <= oa <= 6 and -6 <= ob <= 6
    h, bits = read_header(nal), bits_of(nal)
    new = se_bits(qp - 26) + ue_bits(idc) + (se_bits(oa) + se_bits(ob) if idc != 1 else [])
    return rbsp(nal[0], bits[:h.qd_pos] + new + bits[h.end_pos:])
