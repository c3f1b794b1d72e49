"""Two temporal layers (include/mi355x_h264.h, "temporal layers"): the restatement and the cases that tests/test_temporal_oracle.py
(CPU: the composition holds on the oracle alone, and what the case list holds), tests/test_temporal_host.py (CPU: the host code's
sequence rule) and tests/test_gpu_temporal.py (GPU) share.

The oracle knows nothing of layers and need not.  Number a GOP's pictures from its IDR picture at position 0; the odd positions are
layer 1.  Then
  A. the layer-0 access units are what OracleEncoder(gop = ceil(gop / 2)) writes for the layer-0 pictures alone;
  B. a layer-1 picture is the LAST picture of a fresh oracle encoder fed this GOP's layer-0 pictures up to the preceding one and
     then the picture itself - its MbInfo, vectors, levels and both reconstructions exactly, its access unit after rewrite_nonref():
     the slice header loses adaptive_ref_pic_marking_mode_flag, nal_ref_idc becomes 0;
  C. the composed stream decodes to those reconstructions, and so does its base layer alone.

Everything is deterministic; what is computed is computed once per process, shared and never changed."""
import functools
from collections import namedtuple
import numpy as np
from large_batch import StagesOf
from media_amd import synth

MB_IPCM = 3


# ---------------------------------------------------------------- the sequence rule

Seq = namedtuple("Seq", "idr layer slot frame_num nref nal_hdr")


def sequence(layers, gop, nrefs, pictures, forced=(), failed=()):
    """what every picture of a stream is: Seq(idr, layer, ring slot written, frame_num, usable reference pictures, first byte of its
    slice NAL units).  forced: pictures before which an IDR picture is forced; failed: pictures that do not go out (refused or
    failed on the device) - they move nothing, and the next picture is an IDR picture.  The ring has nrefs + 1 slots"""
    nrefs = max(nrefs, 1)
    nbuf = nrefs + 1
    out, pos, cur, frame_num, refs, force = [], 0, 0, 0, 0, False
    for i in range(pictures):
        idr = i == 0 or pos >= gop or i in forced or force
        if idr:
            pos, frame_num, refs, force = 0, 0, 0, False
        layer = pos & 1 if layers == 2 else 0
        out.append(Seq(idr, layer, cur, frame_num, 0 if idr else min(nrefs, refs), 0x65 if idr else 0x01 if layer else 0x41))
        if i in failed:
            force = True
            continue
        if layer == 0:
            cur, frame_num, refs = (cur + 1) % nbuf, (frame_num + 1) & 255, refs + 1
        pos += 1
    return out


# ---------------------------------------------------------------- bits

class Bits:
    """MSB-first bit string over a bytes object (reader) / a list of bits (writer)"""

    def __init__(self, data):
        self.b = np.unpackbits(np.frombuffer(bytes(data), np.uint8)).tolist()
        self.p = 0

    def u(self, n):
        v = 0
        for _ in range(n):
            v = (v << 1) | self.b[self.p]
            self.p += 1
        return v

    def ue(self):
        z = 0
        while self.b[self.p] == 0:
            z += 1
            self.p += 1
        return self.u(z + 1) - 1


def pack(bits):
    assert len(bits) % 8 == 0
    return np.packbits(np.array(bits, np.uint8)).tobytes()


def ue_bits(v):
    x = v + 1
    n = x.bit_length() - 1
    return [0] * n + [(x >> k) & 1 for k in range(n, -1, -1)]


def se_bits(v):
    return ue_bits(2 * v - 1 if v > 0 else -2 * v)


def slice_header_bits(idr, nonref, frame_num, idr_id, nact, nrefs, qp, no_filter, slices):
    """slice_header() of 7.3.3 from slice_type on, as this encoder writes it (first_mb_in_slice is the slice's own): a bit list"""
    b = ue_bits(7 if idr else 5) + ue_bits(0) + [(frame_num >> k) & 1 for k in range(7, -1, -1)]
    if idr:
        b += ue_bits(idr_id)
    else:
        b += ([1] + ue_bits(nact - 1)) if nact != nrefs else [0]
        b += [0]                                    # ref_pic_list_modification_flag_l0
    if idr:
        b += [0, 0]                                 # no_output_of_prior_pics_flag, long_term_reference_flag
    elif not nonref:
        b += [0]                                    # adaptive_ref_pic_marking_mode_flag
    b += se_bits(qp - 26)
    b += ue_bits(1 if no_filter else 2 if slices > 1 else 0)
    if not no_filter:
        b += se_bits(0) + se_bits(0)
    return b


def unescape(nal):
    out, zeros = bytearray(), 0
    for v in nal:
        if zeros >= 2 and v == 3:
            zeros = 0
            continue
        out.append(v)
        zeros = zeros + 1 if v == 0 else 0
    return bytes(out)


def escape(rbsp):
    out, zeros = bytearray(), 0
    for v in rbsp:
        if zeros == 2 and v <= 3:
            out.append(3)
            zeros = 0
        out.append(v)
        zeros = zeros + 1 if v == 0 else 0
    return bytes(out)


def nal_units(stream):
    """the NAL units of an Annex-B byte string (four-byte start codes), header byte first"""
    parts = bytes(stream).split(b"\x00\x00\x00\x01")
    assert parts[0] == b"", "the stream starts with a start code"
    return parts[1:]


def annexb(nals):
    return b"".join(b"\x00\x00\x00\x01" + n for n in nals)


# ---------------------------------------------------------------- rewrite X

Rewritten = namedtuple("Rewritten", "au slices")     # slices: per slice (branch "plain" | "pcm", bytes before, bytes after, escapes after)


def rewrite_nonref(au, mb_types, mb_bitpos, nmb):
    """the access unit of a P picture a reference encoder wrote, as the same picture coded as a NON-reference picture: every slice
    NAL unit loses adaptive_ref_pic_marking_mode_flag and gets nal_ref_idc 0.  mb_types, mb_bitpos: MbInfo.type and the first bit of
    every macroblock in its slice's RBSP (h264o_enc_mb_bitpos), which tell where a slice's first I_PCM macroblock lies"""
    nals = nal_units(au)
    firsts = []
    for n in nals:
        assert n[0] == 0x41, "a P picture of nal_ref_idc 2: slice NAL units only (header %#x)" % n[0]
        firsts.append(Bits(unescape(n[1:])[:8]).ue())
    out, facts = [], []
    for k, n in enumerate(nals):
        rbsp = unescape(n[1:])                                              # 1. undo the emulation prevention
        r = Bits(rbsp)
        first = r.ue()                                                      # 2. up to the list-modification flag
        assert r.ue() == 5 and r.ue() == 0
        r.u(8)
        if r.u(1):
            r.ue()
        assert r.u(1) == 0, "ref_pic_list_modification_flag_l0"
        cut = r.p
        assert r.b[cut] == 0, "adaptive_ref_pic_marking_mode_flag"
        end = firsts[k + 1] if k + 1 < len(nals) else nmb
        pcm = [m for m in range(first, end) if mb_types[m] == MB_IPCM]
        if not pcm:                                                         # 3. everything behind moves up; stop bit and alignment anew
            stop = len(r.b) - 1 - r.b[::-1].index(1)
            bits = r.b[:cut] + r.b[cut + 1:stop] + [1]
            new = pack(bits + [0] * (-len(bits) % 8))
        else:                                                               # 4. up to the end of the first I_PCM macroblock's mb_type
            r.p = int(mb_bitpos[pcm[0]])
            r.ue()                                                          # mb_skip_run
            assert r.ue() == 30, "mb_type of I_PCM in a P slice"
            q = r.p
            samples = (q + 7) // 8                                          # the first pcm_sample_luma byte
            assert not any(r.b[q:8 * samples]), "pcm_alignment_zero_bit"
            bits = r.b[:cut] + r.b[cut + 1:q]
            new = pack(bits + [0] * (-len(bits) % 8)) + rbsp[samples:]
        esc = escape(new)                                                   # 5. emulation prevention back, nal_ref_idc 0
        out.append(bytes([0x01]) + esc)
        facts.append(("pcm" if pcm else "plain", len(n), 1 + len(esc), len(esc) - len(new), bool(pcm) and pcm[0] > first))
    return Rewritten(annexb(out), tuple(facts))


# ---------------------------------------------------------------- content

SPEEDS = (1, 3, 2, 5, 1, 4, 2, 6, 3, 1, 5, 2, 4, 1, 3, 6)       # the content's speed changes with every picture


def _noise(w, h, seed):
    return (synth._hash_u32(seed, w * h) & np.uint32(255)).astype(np.uint8).reshape(h, w)


def frame(content, w, h, i, seed):
    """tight I420 picture i.  accel: a panning texture whose step per picture follows SPEEDS - the vector of a layer-1 picture (one
    step back) differs from that of the layer-0 picture before it (two steps back); split: two layers drifting apart by quarter
    samples at such steps; noise: white noise with rows of zeros (every macroblock becomes I_PCM at a low QP, and the zeros ask for
    emulation prevention); tail: the accel picture whose lower right part is such noise (I_PCM behind ordinary macroblocks)"""
    t = sum(SPEEDS[k % len(SPEEDS)] for k in range(i)) + seed
    if content == "accel":
        return synth.frame_s1(w, h, t, noise=2, motion=(1, 1))
    if content == "split":
        return synth.frame_split(w, h, t)
    if content == "cut3":                            # a scene cut at picture 3, an odd position: the panning texture, then its inverted mirror image at twice the contrast
        f = synth.frame_s1(w, h, t, noise=2, motion=(1, 1))
        if i < 3:
            return f
        n = w * h
        y, u, v = f[:n].reshape(h, w), f[n:n * 5 // 4].reshape(h // 2, w // 2), f[n * 5 // 4:].reshape(h // 2, w // 2)
        y2 = np.clip((127 - y[::-1, ::-1].astype(np.int32)) * 2 + 128, 0, 255).astype(np.uint8)      # (twice the contrast: no match anywhere)
        return np.concatenate([y2.ravel(), u[::-1, ::-1].ravel(), (255 - v[::-1, ::-1]).ravel()])
    ysz = w * h
    if content == "noise":
        f = np.concatenate([_noise(w, h, 100 + 3 * i + seed).ravel(), _noise(w // 2, h // 2, 101 + 3 * i + seed).ravel(), _noise(w // 2, h // 2, 102 + 3 * i + seed).ravel()])
        y = f[:ysz].reshape(h, w)
        y[3::8, :] = 0
        f[ysz:].reshape(h, w // 2)[2::5, :] = 0
        return f
    if content == "tail":
        f = synth.frame_s1(w, h, t, noise=2, motion=(1, 1)).copy()
        y, u, v = f[:ysz].reshape(h, w), f[ysz:ysz * 5 // 4].reshape(h // 2, w // 2), f[ysz * 5 // 4:].reshape(h // 2, w // 2)
        if i > 0:                                    # (the IDR picture stays plain: the P pictures then have something to refer to)
            y0, x0 = (h // 32) * 16, (w // 32) * 16
            y[y0:, x0:] = _noise(w, h, 200 + i)[y0:, x0:]
            u[y0 // 2:, x0 // 2:] = _noise(w // 2, h // 2, 300 + i)[y0 // 2:, x0 // 2:]
            v[y0 // 2:, x0 // 2:] = _noise(w // 2, h // 2, 400 + i)[y0 // 2:, x0 // 2:]
        return f
    raise KeyError(content)


# ---------------------------------------------------------------- the cases

Case = namedtuple("Case", "name content w h prof refs slices qp gop pictures search deblock forced qps seed")


def case(name, content, w, h, prof=66, refs=0, slices=0, qp=26, gop=30, pictures=9, search=1, deblock=True, forced=(), qps=(), seed=0):
    return Case(name, content, w, h, prof, refs, slices, qp, gop, pictures, search, deblock, tuple(forced), tuple(qps), seed)


CASES = (
    case("one_mb_16x16", "accel", 16, 16, qp=24, pictures=7),                                   # one macroblock: every neighbour is missing
    case("accel_48x48", "accel", 48, 48, qp=26, pictures=9),
    case("odd_gop_96x80_high", "split", 96, 80, prof=100, slices=2, qp=24, gop=7, pictures=12, forced=(9,)),   # GOP of odd length; IDR forced behind a layer-1 picture
    case("refs3_112x64_main", "accel", 112, 64, prof=77, refs=3, qp=30, pictures=10),           # reference counts 1, 2, 3
    case("exhaustive_34x18", "accel", 34, 18, qp=20, pictures=6, search=0, deblock=False),
    case("noise_48x32", "noise", 48, 32, qp=10, pictures=7),                                    # every layer-1 macroblock is I_PCM
    case("tail_80x64", "tail", 80, 64, qp=10, pictures=6),                                      # I_PCM behind ordinary macroblocks of one slice
    case("four_slices_64x128_main", "accel", 64, 128, prof=77, slices=4, qp=28, gop=6, pictures=9, qps=((4, 22), (7, 34))),
    case("accel_208x160", "accel", 208, 160, qp=27, gop=8, pictures=11, refs=2),
)
BY_NAME = {c.name: c for c in CASES}
# the plugin surface (GOP lengths from 30): a scene cut on a layer-1 picture, which the plugin class codes again as an IDR picture
PLUGIN = case("plugin_cut_64x48", "cut3", 64, 48, qp=30, gop=30, pictures=8)
SCENE_CUT_COST_PER_MB = 3000     # VideoEncoderMI355X::Rc::kSceneCutCostPerMb
SEEDED = tuple(c for c in CASES if c.search == 1 and c.content != "noise")     # (noise: no layer-1 macroblock has a vector)


@functools.lru_cache(maxsize=None)
def frames(c):
    out = tuple(frame(c.content, c.w, c.h, i, c.seed) for i in range(c.pictures))
    for f in out:
        f.setflags(write=False)
    return out


def seq_of(c, layers=2):
    return sequence(layers, c.gop, c.refs, c.pictures, c.forced)


def qp_of(c, i):
    qp = c.qp
    for at, v in c.qps:
        if at <= i:
            qp = v
    return qp


def oracle_for(c, gop):
    from oracle_lib import OracleEncoder
    return OracleEncoder(c.w, c.h, qp=c.qp, gop=gop, profile_idc=c.prof, slices=c.slices, refs=c.refs, search=c.search,
                         disable_deblock=0 if c.deblock else 1)


# prev_mv: (mvx, mvy) the preceding layer-0 picture left (layer 1 only); cost: the scene-change statistic (h264o_enc_last_me_cost)
Pic = namedtuple("Pic", "au idr layer stages prev_mv rewritten cost")


def compose(c, fr, idr_id=0):
    """the two-layer stream of the pictures fr driven as the case says, composed from the unchanged oracle as A and B say: a tuple
    of Pic.  idr_id: idr_pic_id of the first IDR picture (a batch item's)"""
    seq = sequence(2, c.gop, c.refs, len(fr), c.forced)
    nmb = ((c.w + 15) // 16) * ((c.h + 15) // 16)
    base = oracle_for(c, (c.gop + 1) // 2)
    base.set_idr_id(idr_id)
    out, gop0 = [], []                       # gop0: this GOP's layer-0 pictures so far
    for i, s in enumerate(seq):
        if s.layer == 0:
            base.set_qp(qp_of(c, i))
            au, idr = base.encode(fr[i], force_idr=i in c.forced)
            assert idr == s.idr, "%s picture %d: the base layer's IDR pictures are the stream's" % (c.name, i)
            gop0 = [i] if idr else gop0 + [i]
            out.append(Pic(au, idr, 0, StagesOf(base), None, None, base.me_cost()))
            continue
        one = oracle_for(c, 1 << 20)
        for j in gop0:
            one.set_qp(qp_of(c, j))
            one.encode(fr[j])
        mb0 = one.mbinfo()
        one.set_qp(qp_of(c, i))
        au, idr = one.encode(fr[i])
        assert not idr
        rw = rewrite_nonref(au, one.mbinfo()["type"], one.mb_bitpos(), nmb)
        out.append(Pic(rw.au, False, 1, StagesOf(one), (mb0["mvx"].copy(), mb0["mvy"].copy()), rw, one.me_cost()))
        one.close()
    base.close()
    return tuple(out)


@functools.lru_cache(maxsize=None)
def expected(c):
    """the two-layer stream of the case"""
    return compose(c, frames(c))


@functools.lru_cache(maxsize=None)
def expected_one_layer(c):
    """the ordinary stream of the case's pictures (layers off): (access unit, idr) per picture"""
    orc, out = oracle_for(c, c.gop), []
    for i, f in enumerate(frames(c)):
        orc.set_qp(qp_of(c, i))
        out.append(orc.encode(f, force_idr=i in c.forced))
    orc.close()
    return tuple(out)


def stream_of(c):
    return b"".join(p.au for p in expected(c))
