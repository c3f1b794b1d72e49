"""The decoder's conceal mode restated (include/mi355x_h264_dec.h, "loss mode"): what is missing is decoded as if an all-P_Skip slice
had arrived in its place.  This module holds the streams, the case list, a spec-literal writer of that slice (7.3.3 for this
encoder's parameter sets, ue(mb_skip_run), rbsp_trailing_bits) and of an all-skip picture, and the COMPOSITION: the stream with the
lost NAL units replaced by their stand-ins, which the oracle's independent decoder decodes without knowing of loss.  Shared by
tests/test_dec_loss_oracle.py (CPU), tests/test_dec_loss_host.py (CPU) and tests/test_gpu_dec_loss.py; nothing of the decoder under
test is used here.

The parameter sets of every stream here: log2_max_frame_num 8, pic_order_cnt_type 2, pic_init_qp 26, CAVLC,
deblocking_filter_control_present_flag 1, one picture parameter set (id 0).

Everything is deterministic; what is computed is computed once per process, shared and never changed."""
import base64
import functools
import json
import os
from collections import namedtuple
import numpy as np
import intra_refresh as ir
import temporal as tl
from temporal import Bits, pack, ue_bits, se_bits, escape, unescape, nal_units, annexb
from slice_header import FN_BITS, Hdr, read_header, bits_of as _bits, rbsp as _rbsp

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "dec_loss_streams.json")
TAINTED, CONCEALED = 1, 2


# ---------------------------------------------------------------- slice headers of this encoder's streams

def skip_slice(first_mb, count, frame_num, ref_idc, nact, qp, idc, oa=0, ob=0):
    """the NAL unit of ONE P slice of `count` macroblocks from first_mb on, all P_Skip: slice_header (7.3.3), slice_data (7.3.4) =
    one mb_skip_run, rbsp_slice_trailing_bits"""
    b = ue_bits(first_mb) + ue_bits(5) + ue_bits(0)                     # first_mb_in_slice, slice_type P (all slices), pic_parameter_set_id
    b += [(frame_num >> k) & 1 for k in range(FN_BITS - 1, -1, -1)]     # frame_num
    b += [0] if nact is None else [1] + ue_bits(nact - 1)               # num_ref_idx_active_override_flag, num_ref_idx_l0_active_minus1
    b += [0]                                                            # ref_pic_list_modification_flag_l0
    if ref_idc:
        b += [0]                                                        # adaptive_ref_pic_marking_mode_flag
    b += se_bits(qp - 26)                                               # slice_qp_delta
    b += ue_bits(idc)                                                   # disable_deblocking_filter_idc
    if idc != 1:
        b += se_bits(oa) + se_bits(ob)                                  # slice_alpha_c0_offset_div2, slice_beta_offset_div2
    b += ue_bits(count)                                                 # mb_skip_run
    b += [1]                                                            # rbsp_stop_one_bit
    b += [0] * (-len(b) % 8)                                            # rbsp_alignment_zero_bit
    return bytes([(ref_idc << 5) | 1]) + escape(pack(b))


def rewrite_frame_num(nal, frame_num):
    rbsp = unescape(nal[1:])
    h = read_header(nal)
    bits = np.unpackbits(np.frombuffer(rbsp, np.uint8)).tolist()
    bits[h.fn_pos:h.fn_pos + FN_BITS] = [(frame_num >> k) & 1 for k in range(FN_BITS - 1, -1, -1)]
    return bytes([nal[0]]) + escape(pack(bits))


def renumber_sps(nal, sps_id):
    """a Baseline SPS (seq_parameter_set_id follows the three bytes profile, constraints, level) under another id"""
    bits = _bits(nal)
    r = Bits(unescape(nal[1:]))
    r.u(24)
    r.ue()
    return _rbsp(nal[0], bits[:24] + ue_bits(sps_id) + bits[r.p:])


def renumber_pps(nal, pps_id, sps_id):
    bits = _bits(nal)
    r = Bits(unescape(nal[1:]))
    r.ue(), r.ue()
    return _rbsp(nal[0], ue_bits(pps_id) + ue_bits(sps_id) + bits[r.p:])


def restart_slice(nal, first_mb, pps_id):
    """a slice NAL unit with another first_mb_in_slice and pic_parameter_set_id"""
    bits = _bits(nal)
    r = Bits(unescape(nal[1:]))
    r.ue()
    st = r.ue()
    r.ue()
    return _rbsp(nal[0], ue_bits(first_mb) + ue_bits(st) + ue_bits(pps_id) + bits[r.p:])


def other_size_unit():
    """damage that names a LARGER picture: the second access unit of the 48x64 stream, with the 64x96 stream's parameter sets as
    ids 1 in front, its own slice 0, and its slice 1 re-addressed to macroblock 20 under picture parameter set 1 - an address
    inside the 24 macroblocks of that other size and outside the 12 of the picture.  Returns (the units to feed before, the unit)"""
    small, big = stream("ir2_48x64"), stream("ir3_64x96")
    sets = [n for n in nal_units(big.aus[0]) if (n[0] & 31) in (7, 8)]
    sps1, pps1 = renumber_sps(sets[0], 1), renumber_pps(sets[1], 1, 1)
    _, sl = slices_of(small.aus[1])
    return (small.aus[0],), annexb([sps1, pps1, sl[0], restart_slice(sl[1], 20, 1)])


def grey_idr(mbw, mbh):
    """an IDR picture of I_PCM macroblocks, every sample 128, under the streams' parameter sets (tests/pcm_stream.py writes such
    slices for parameter sets of its own): frame_num 0, slice_qp_delta 0, disable_deblocking_filter_idc 1"""
    b = ue_bits(0) + ue_bits(7) + ue_bits(0) + [0] * FN_BITS + ue_bits(0) + [0, 0] + se_bits(0) + ue_bits(1)
    out = bytearray()
    for m in range(mbw * mbh):
        b += ue_bits(25)                                                # mb_type I_PCM
        b += [0] * (-len(b) % 8)                                        # pcm_alignment_zero_bit
        out += pack(b) + bytes([128]) * 384
        b = []
    return b"\x65" + escape(bytes(out) + b"\x80")


# ---------------------------------------------------------------- the streams

Stream = namedtuple("Stream", "name w h aus n bands")     # aus: the access units; n: refresh bands (0: no intra refresh); bands: k per picture


def _content(w, h, pictures, seed=0):
    return [tl.frame("accel", w, h, i, seed) for i in range(pictures)]


@functools.lru_cache(maxsize=None)
def stream(name):
    from oracle_lib import OracleEncoder
    if name.startswith("ir"):
        rec = json.load(open(GOLDEN))[name]
        c = ir.Case(*rec["case"])
        return Stream(name, c.w, c.h, tuple(base64.b64decode(a) for a in rec["aus"]), c.n, tuple(rec["bands"]))
    if name in ("tl2_48x48", "tl2_refs3_112x64"):
        c = tl.BY_NAME["accel_48x48" if name == "tl2_48x48" else "refs3_112x64_main"]
        return Stream(name, c.w, c.h, tuple(p.au for p in tl.expected(c)), 0, ())
    kw = {"one_34x18": dict(w=34, h=18, pictures=8, qp=24), "refs3_64x64": dict(w=64, h=64, pictures=12, qp=26, refs=3),
          "idr2_64x64": dict(w=64, h=64, pictures=10, qp=26, gop=4)}[name]
    w, h, pictures = kw.pop("w"), kw.pop("h"), kw.pop("pictures")
    enc = OracleEncoder(w, h, **dict(dict(gop=1000), **kw))
    aus = tuple(enc.encode(f)[0] for f in _content(w, h, pictures))
    enc.close()
    return Stream(name, w, h, aus, 0, ())


def slices_of(au):
    """(other NAL units in front, slice NAL units)"""
    nals = nal_units(au)
    return [n for n in nals if (n[0] & 31) not in (1, 5)], [n for n in nals if (n[0] & 31) in (1, 5)]


def parameter_sets(s):
    return annexb([n for n in nal_units(s.aus[0]) if (n[0] & 31) in (7, 8)])


# ---------------------------------------------------------------- the cases

# loss: {picture: ("drop", slice numbers) | ("flip", slice number, byte of the NAL unit, bit) | ("lose",)}
#   drop: those slice NAL units do not arrive;  flip: one bit of a slice's data arrives flipped (the slice then fails to parse: the
#   CPU test asserts that);  lose: the access unit does not arrive at all
# join: None, or the picture the decoder starts at, having been fed the parameter sets alone before
Case = namedtuple("Case", "name stream loss join kind")


def case(name, stream, loss, join=None, kind="slice"):
    return Case(name, stream, tuple(sorted(loss.items())), join, kind)


CASES = (
    case("ir3_lose_band1", "ir3_64x96", {3: ("drop", (1,))}),
    case("ir3_lose_first", "ir3_64x96", {5: ("drop", (0,))}),
    case("ir3_lose_two", "ir3_64x96", {3: ("drop", (1, 2))}),
    case("ir3_flip", "ir3_64x96", {6: ("flip", 2, 11, 1)}),
    case("ir2_lose_last", "ir2_48x64", {2: ("drop", (1,))}),
    case("one_lose_only", "one_34x18", {3: ("flip", 0, 10, 0)}, kind="gap"),
    case("refs3_gap1", "refs3_64x64", {5: ("lose",)}, kind="gap"),
    case("refs3_gap2", "refs3_64x64", {5: ("lose",), 6: ("lose",)}, kind="gap"),
    case("refs3_gap4", "refs3_64x64", {5: ("lose",), 6: ("lose",), 7: ("lose",), 8: ("lose",)}, kind="gap"),
    case("tl2_lose_layer1", "tl2_48x48", {3: ("lose",)}, kind="nonref"),
    # a gap met by a NON-reference picture under three reference pictures: the gap is taken in once, the picture behind finds none
    case("tl2_refs3_gap_then_nonref", "tl2_refs3_112x64", {6: ("lose",)}, kind="gap"),
    case("idr2_lose_idr", "idr2_64x64", {4: ("lose",)}, kind="gap"),
    case("ir2_join_at_recovery", "ir2_48x64", {}, 3, "join"),
    case("ir2_join_before", "ir2_48x64", {}, 1, "join"),
    case("ir3_join_at_recovery", "ir3_64x96", {}, 4, "join"),
    case("ir3_join_before", "ir3_64x96", {}, 2, "join"),
)
BY_NAME = {c.name: c for c in CASES}

# fed: what the decoder under test is given - per step an access unit, or None (nothing arrives)
# got: per step, whether a picture must come out;  ref: per step the index into `composed` of the picture that must come out
# composed: the access units for the oracle;  orig: per step the picture of the ORIGINAL stream it is (the lossless decode), or None
# concealed / gap: per step, macroblocks the test removed from that picture / reference pictures missing in front of it
Plan = namedtuple("Plan", "fed got ref composed orig concealed gap first_loss")


def _flip(nal, byte, bit):
    a = bytearray(nal)
    a[byte] ^= 1 << bit
    return bytes(a)


@functools.lru_cache(maxsize=None)
def plan(c):
    s = stream(c.stream)
    mbw, mbh = (s.w + 15) // 16, (s.h + 15) // 16
    nmb = mbw * mbh
    fed, got, ref, composed, orig, concealed, gap = [], [], [], [], [], [], []
    start, shift = 0, 0
    if c.join is not None:
        # the decoder gets the parameter sets, then the stream from picture `join` on; the oracle gets a grey IDR picture in front and
        # frame_num counted from it
        start = c.join
        fed.append(parameter_sets(s)); got.append(False); ref.append(None); orig.append(None); concealed.append(0); gap.append(0)
        composed.append(parameter_sets(s) + annexb([grey_idr(mbw, mbh)]))
        shift = 1 - read_header(slices_of(s.aus[start])[1][0]).frame_num
        last_qp = 26
    last_qp = last_qp if c.join is not None else None   # slice QP of the last slice of the previous picture of the composed stream
    nact = None             # num_ref_idx override of the last P slice seen
    arrived_fn = None       # frame_num (the stream's own) of the last reference picture that arrived
    fn_shift = 0            # (a lost IDR picture: the frame_num of what follows goes on counting)
    prev_fn = 0
    for i in range(start, len(s.aus)):
        other, sl = slices_of(s.aus[i])
        hs = [read_header(n) for n in sl]
        act = dict(c.loss).get(i)
        if hs[0].idr and not (act and act[0] == "lose"):
            fn_shift = 0
        fn = (hs[0].frame_num + shift + fn_shift) & 255
        if act and (act[0] == "lose" or (act[0] == "flip" and len(sl) == 1)):
            # the whole picture is lost: nothing comes out; a reference picture is stood in for by an all-skip picture
            fed.append(None if act[0] == "lose" else annexb(other + [_flip(sl[0], act[2], act[3])]))
            got.append(False); ref.append(None); orig.append(i); concealed.append(0); gap.append(0)
            if hs[0].ref_idc:
                if hs[0].idr:
                    fn = (prev_fn + 1) & 255
                    fn_shift = fn
                composed.append(annexb([skip_slice(0, nmb, fn, 2, nact, last_qp, 2 if len(sl) > 1 else hs[0].idc)]))
                prev_fn = fn
            continue
        lost = set(act[1]) if act and act[0] == "drop" else ({act[1]} if act else set())
        keep_fed = [(_flip(n, act[2], act[3]) if act and act[0] == "flip" and k == act[1] else n) for k, n in enumerate(sl)
                    if not (act and act[0] == "drop" and k in lost)]
        out, k, removed, qp_prev = list(other), 0, 0, last_qp
        pic_nact = next((h.nact for kk, h in enumerate(hs) if kk not in lost and h.slice_type % 5 == 0), nact)   # the fill's list is the received P slices'
        g = 0 if arrived_fn is None or hs[0].idr else (hs[0].frame_num - arrived_fn - 1) & 255                  # 7.4.3, on the stream's own frame_num
        if g:                                        # (8.2.5.2: PrevRefFrameNum is then the last missing picture's, whatever this picture is)
            arrived_fn = (hs[0].frame_num - 1) & 255
        while k < len(sl):
            if k not in lost:
                out.append(sl[k] if not (shift or fn_shift) else rewrite_frame_num(sl[k], fn))
                qp_prev = hs[k].qp
                if hs[k].slice_type % 5 == 0:
                    nact = hs[k].nact
                k += 1
                continue
            j = k
            while j < len(sl) and j in lost:
                j += 1
            first, end = hs[k].first_mb, hs[j].first_mb if j < len(sl) else nmb
            out.append(skip_slice(first, end - first, fn, hs[k].ref_idc, pic_nact, qp_prev, hs[k].idc, hs[k].oa, hs[k].ob))
            removed += end - first
            k = j
        fed.append(annexb(other + keep_fed)); got.append(True); ref.append(len(composed)); orig.append(i); concealed.append(removed); gap.append(g)
        composed.append(annexb(out))
        last_qp = qp_prev
        if hs[0].ref_idc:
            prev_fn = fn
            arrived_fn = hs[0].frame_num
    loss_steps = [k for k in range(len(fed)) if concealed[k] or gap[k] or (c.join is not None and k == 1)]
    return Plan(tuple(fed), tuple(got), tuple(ref), tuple(composed), tuple(orig), tuple(concealed), tuple(gap), loss_steps[0] if loss_steps else None)


@functools.lru_cache(maxsize=None)
def oracle_planes(aus):
    """the oracle decoder's (Y, U, V) coded planes per access unit of the tuple `aus` (None where a unit holds no picture)"""
    from oracle_lib import OracleDecoder
    dec, out = OracleDecoder(), []
    for au in aus:
        rc = dec.decode(au)
        out.append(tuple(dec.plane(p) for p in range(3)) if rc == 1 else None)
    dec.close()
    for pic in out:
        for a in pic or ():
            a.setflags(write=False)
    return tuple(out)


def expected(c):
    """per step: the planes the decoder under test must deliver (None: no picture)"""
    p = plan(c)
    planes = oracle_planes(p.composed)
    return tuple(None if r is None else planes[r] for r in p.ref)


def lossless(c):
    """per step: the planes of the lossless decode of that picture (None: the step is no picture of the original stream)"""
    p = plan(c)
    planes = oracle_planes(stream(c.stream).aus)
    return tuple(None if o is None else planes[o] for o in p.orig)


def mb_equal(a, b, mbw, mbh):
    """(mbh, mbw) bool: the macroblock's samples are equal in Y, U and V"""
    eq = np.ones((mbh, mbw), bool)
    for p in range(3):
        n = 16 if p == 0 else 8
        eq &= (a[p] == b[p]).reshape(mbh, n, mbw, n).all(axis=(1, 3))
    return eq


def recovery_step(c):
    """the step at which an intra-refresh case is exact again: the picture with k = n - 1 of the first refresh cycle that starts
    after the loss (a join at a picture with k = 0 starts one there)"""
    s, p = stream(c.stream), plan(c)
    i = p.orig[p.first_loss]
    start = i if (c.join is not None and s.bands[i] == 0) else next(j for j in range(i + 1, len(s.aus)) if s.bands[j] == 0)
    return p.orig.index(start + s.n - 1)
