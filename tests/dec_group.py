"""Decoder groups (include/mi355x_h264_dec.h mi355x_h264_dec_group_*, media_amd.h264dec.DecoderGroup): the case list that
tests/test_dec_group_oracle.py (CPU: what the list holds) and tests/test_gpu_dec_group.py (GPU) share.  A case is a picture size
and a list of streams; step t of a case hands every stream its picture t.  The streams come from the oracle's random-syntax
generator (h264o_enc_random_picture) with different profiles, slice shapes, reference counts, feature bits and GOP lengths, so that
one step holds IDR pictures, P pictures and all-intra non-IDR pictures of streams whose ring positions, reference lists, offsets and
filter controls differ; a few come from the oracle ENCODER (kind "enc").  The expected samples are the oracle decoder's."""
import hashlib
from collections import namedtuple

from media_amd import synth
from oracle_lib import OracleEncoder, OracleDecoder

N, T, PS = OracleEncoder.RAND_NONREF, OracleEncoder.RAND_SLICE_TYPES, OracleEncoder.RAND_PARAMETER_SETS
QP, CQ, FO, PCM, IDC, SUB, CUT, REO, OH, BIG = 1, 2, 4, 8, 16, 32, 64, 128, 256, 512

# kind "rand": prof, slices, refs, features, gop, seed;  kind "enc": prof, slices, refs, content name, gop, qp
Stream = namedtuple("Stream", "kind prof slices refs arg gop seed")
Case = namedtuple("Case", "name w h pictures streams")


def R(prof, slices, refs, features, gop, seed):
    return Stream("rand", prof, slices, refs, features, gop, seed)


def E(prof, slices, refs, content, gop, qp):
    return Stream("enc", prof, slices, refs, content, gop, qp)


# twelve streams at 96x80 (6 x 5 macroblocks): every line says what it is there for
TWELVE = [
    R(100, 0, 3, QP | CQ | FO | PCM | IDC | SUB | BIG, 5, 1),          # High: second chroma offset, 8x8 transform, large levels, one slice
    R(66, 2, 1, QP | IDC | FO, 4, 2),                                   # bands of rows, one reference
    R(77, 0, 2, QP | SUB | CUT | IDC | BIG, 6, 3),                      # slices cut at arbitrary macroblocks, two references
    R(66, 0, 3, N | REO | QP | OH, 7, 4),                               # non-reference pictures, list modification
    R(100, 3, 3, N | T | PS | QP | CQ | FO | IDC | SUB | REO | OH, 5, 5),  # everything at picture level, PPS switches
    R(66, 0, 3, REO | SUB | QP, 12, 6),                                 # long GOP: three references in use, reordered
    R(77, 2, 2, T | QP | FO | IDC, 6, 7),                               # all-intra non-IDR pictures
    R(100, 0, 1, PCM | QP | CQ | BIG, 3, 8),
    R(66, 0, 3, N | OH | QP, 5, 9),                                     # non-reference pictures around the IDR pictures (gop 5)
    R(100, 2, 3, PS | CQ | FO | IDC | QP, 4, 10),
    E(66, 0, 2, "s1", 4, 28),                                           # the oracle encoder's own streams
    E(100, 2, 1, "cut", 5, 30),
]
ONE = [TWELVE[0]]
# forty streams at 32x32 (2 x 2 macroblocks): more items than the row wavefronts hold at a time, so their workgroups walk
FORTY = [R((66, 77, 100)[i % 3], (0, 2)[i % 2], 1 + i % 3, (QP | IDC | FO | SUB | ((N | OH) if i % 4 == 1 else 0) | (REO if i % 5 == 2 else 0) | (T if i % 7 == 3 else 0) |
                                                           (CQ if i % 3 == 2 else 0) | (PCM if i % 6 == 0 else 0)), 3 + i % 4, 100 + i) for i in range(40)]
CASES = [
    Case("one_96x80", 96, 80, 8, ONE),
    Case("twelve_96x80", 96, 80, 8, TWELVE),
    Case("forty_32x32", 32, 32, 6, FORTY),
    Case("four_176x144", 176, 144, 6, [R(100, 3, 3, QP | CQ | FO | IDC | SUB | REO | BIG, 4, 31), R(66, 0, 2, N | OH | QP | CUT | SUB, 5, 32),
                                       E(77, 3, 3, "split", 3, 26), R(77, 0, 1, T | PCM | QP | IDC, 6, 33)]),
    Case("five_64x48", 64, 48, 12, [R(66, 0, 3, N | REO | OH | QP, 6, 41), R(100, 0, 2, PS | CQ | SUB, 4, 42), R(77, 2, 1, IDC | FO, 5, 43),
                                    E(66, 0, 1, "s3", 6, 30), R(100, 0, 3, BIG | PCM | QP | SUB | REO, 7, 44)]),
]
BY_NAME = {c.name: c for c in CASES}

_cache = {}
_facts = {}


def _picture_facts(enc, dec, idr, rand, mbw):
    """what one picture holds, from sources that share nothing with the product's parser: the writer's counters and side
    information (h264o_hits since the reset before this picture, mbinfo(), levels(), random_last()) and the oracle's independent
    decoder's statistics (macroblock kinds, QPs, vectors and reference index per 4x4 block, RefPicList0, nal_ref_idc)"""
    import numpy as np
    from oracle_lib import lib
    import ctypes as C
    hits = enc.hits()
    mb, lv = enc.mbinfo(), enc.levels().reshape(-1, 416).astype(np.int32)
    kinds, qps = dec.mb_kinds(), dec.mb_qps()
    inter = kinds == OracleDecoder.KIND_INTER
    sub8 = ref_gt0 = 0
    x, y, r = C.c_int(0), C.c_int(0), C.c_int(0)
    for addr in np.nonzero(inter)[0]:
        v = []
        for b in range(16):
            lib().h264o_dec_mb_mv(dec.h, int(addr), b, C.byref(x), C.byref(y), C.byref(r))
            v.append((x.value, y.value, r.value))
        # raster 4x4 blocks of quadrant q: a partition below 8x8 shows as two vectors inside one quadrant
        quads = [[v[4 * (2 * (q >> 1) + j) + 2 * (q & 1) + i] for j in range(2) for i in range(2)] for q in range(4)]
        sub8 += any(len({(a, b) for a, b, _ in quad}) > 1 for quad in quads)
        ref_gt0 += any(c > 0 for _, _, c in v)
    notpcm = mb["type"] != 3
    f = {"idr": bool(idr), "is_ref": bool(dec.last_is_ref), "has_inter": bool((inter | (kinds == OracleDecoder.KIND_SKIP)).any()),
         "has_intra": bool(np.isin(kinds, (OracleDecoder.KIND_I4, OracleDecoder.KIND_I16, OracleDecoder.KIND_IPCM)).any()),
         "pcm_written": int(hits["mb_kind"][3]), "pcm_decoded": int((kinds == OracleDecoder.KIND_IPCM).sum()),
         "p8x8_written": int(hits["mb_type"][1][3]), "sub8": int(sub8), "ref_gt0": int(ref_gt0),
         "qps": sorted({int(q) for q, k in zip(qps, kinds) if k != OracleDecoder.KIND_IPCM}), "mbqp": qps.astype(np.uint8),
         # transform_size_8x8_flag = 1 as the writer's side information has it; in a P_8x8 macroblock the flag is only sent (and the
         # 8x8 transform only used) when no quadrant is split further, which the side information does not say: counted apart
         "t8_written": int((np.isin(mb["type"], (1, 5, 6)) & (mb["i16_mode"] == 1) & ((mb["cbp"] & 15) != 0)).sum()),
         "t8_p8x8_at_most": int(((mb["type"] == 7) & (mb["i16_mode"] == 1) & ((mb["cbp"] & 15) != 0)).sum()),
         "big": int((np.abs(lv[notpcm]) > 127).sum()), "ref_ages": dec.ref_ages(),
         "nonref_before_idr": int(hits["nonref_before_idr"]), "nonref_after_idr": int(hits["nonref_after_idr"]),
         "pps_switch": int(hits["pps_switches"]), "rand": rand}
    return f


def stream_pictures(case, k):
    """stream k of the case: [(access unit, [oracle decoder's three coded planes], its cropped I420 picture, (width, height))];
    stream_facts(case, k) holds what each picture contains"""
    key = (case.name, k)
    if key in _cache:
        return _cache[key]
    import numpy as np
    s = case.streams[k]
    dec = OracleDecoder()
    out, facts = [], []
    rand = s.kind == "rand"
    if rand:
        enc = OracleEncoder(case.w, case.h, qp=30, gop=s.gop, profile_idc=s.prof, slices=s.slices, refs=s.refs)
        frames = [None] * case.pictures
    else:
        enc = OracleEncoder(case.w, case.h, qp=s.seed, gop=s.gop, profile_idc=s.prof, slices=s.slices, refs=s.refs)
        frames = synth.sequence(s.arg, case.w, case.h, case.pictures)
    for i, f in enumerate(frames):
        enc.hits_reset()
        if rand:
            au, idr, _ = enc.random_picture(7919 * s.seed + 104729 * i, features=s.arg)
        else:
            au, idr = enc.encode(f)[0], i % s.gop == 0
        assert dec.decode(au) == 1
        out.append((au, [dec.plane(p).copy() for p in range(3)], np.concatenate([dec.cropped(p).ravel() for p in range(3)]), tuple(dec.size)))
        facts.append(_picture_facts(enc, dec, idr, rand, (case.w + 15) // 16))
    enc.close()
    dec.close()
    _cache[key] = out
    _facts[key] = facts
    return out


def stream_facts(case, k):
    stream_pictures(case, k)
    return _facts[(case.name, k)]


def digest(planes):
    return hashlib.sha256(b"".join(p.tobytes() for p in planes)).hexdigest()
