"""Random streams at the ends of the QP, level and vector ranges (oracle/h264_enc.c h264o_enc_random_picture, feature 131072;
oracle/h264_oracle.h says what it draws).  The case list and the helpers that tests/test_range_ends_oracle.py (CPU: what the
list holds, and that every stream is conforming) and tests/test_gpu_range_ends.py (GPU) share.  Everything a case is said to hold
comes from sources that share nothing with the product: the writer's counters and side information, and the statistics of the
oracle's independent decoder (h264o_dec_stat)."""
from collections import namedtuple

import numpy as np

from oracle_lib import OracleEncoder, OracleDecoder, LV_LUMA_DC, LV_LUMA, LV_CHROMA_DC, LV_CHROMA_AC

RE = OracleEncoder.RAND_RANGE_ENDS
BASE = 1 | 2 | 4 | 8 | 16 | 32 | 64 | 128    # QPs, chroma offsets, filter offsets, I_PCM, every idc, partitions down to 4x4, slices cut anywhere, list modification
PICTURES, GOP = 12, 5                         # IDR pictures 0, 5, 10; picture 5 carries many large levels, picture 9 very many
QP_ENDS = (0, 1, 2, 3, 49, 50, 51)
MV_LIMITS = (-8192, 8191, -2048, 2047)        # A.3.1 at the level_idc the streams write, quarter samples

# name, width, height, profile_idc, slices, refs, features, floors.  The floors were measured on the oracle (the generator is
# deterministic, so they are what the case holds; tests/test_range_ends_oracle.py asserts them):
#   end_qp     coded (non-skip, non-I_PCM) macroblocks whose QP_Y is one of QP_ENDS
#   p15_max    levels of level_prefix 15 with an all-ones suffix (the largest magnitude it codes), all suffixLengths together
#   p16        levels of level_prefix 16 (High only)
#   byte_edge  levels of exactly +-127, +-128, +-129
#   at_limit   vector components written exactly at a limit of A.3.1 (the least of the four limits)
#   outside    predicted partitions whose reference samples lie wholly outside the picture (the least of the four sides)
#   mvd_over   mvd_l0 components of magnitude above 8192
#   large      the most levels outside -128 .. 127 in one picture
Case = namedtuple("Case", "name w h prof slices refs features floors")
CASES = [
    Case("16x16_baseline", 16, 16, 66, 0, 1, RE | BASE, dict(end_qp=6, p15_max=0, p16=0, byte_edge=1, at_limit=0, outside=3, mvd_over=1, large=0)),
    Case("16x16_main", 16, 16, 77, 0, 2, RE | BASE, dict(end_qp=6, p15_max=1, p16=0, byte_edge=2, at_limit=0, outside=3, mvd_over=0, large=1)),
    Case("48x48_baseline", 48, 48, 66, 0, 2, RE | BASE, dict(end_qp=61, p15_max=7, p16=0, byte_edge=1592, at_limit=1, outside=10, mvd_over=4, large=959)),
    Case("48x48_main", 48, 48, 77, 2, 3, RE | BASE, dict(end_qp=60, p15_max=3, p16=0, byte_edge=1927, at_limit=2, outside=14, mvd_over=1, large=1405)),
    Case("96x80_baseline", 96, 80, 66, 0, 3, RE | BASE, dict(end_qp=195, p15_max=17, p16=0, byte_edge=7377, at_limit=8, outside=32, mvd_over=14, large=5441)),
    Case("96x80_main", 96, 80, 77, 3, 2, RE | BASE, dict(end_qp=179, p15_max=15, p16=0, byte_edge=7287, at_limit=8, outside=44, mvd_over=14, large=4560)),
    Case("96x80_main_constrained", 96, 80, 77, 0, 1, RE | BASE | 1024, dict(end_qp=180, p15_max=12, p16=0, byte_edge=7042, at_limit=11, outside=57, mvd_over=16, large=4900)),
    # without 32 / 64: whole partitions with one reference index per macroblock, written from the generator's side information
    # (the 16x8 / 8x16 directional predictors of the encoder's own 8.4.1.3), slices in bands of rows
    Case("96x80_main_whole_partitions", 96, 80, 77, 2, 3, RE | 1 | 2 | 4 | 8 | 16 | 128, dict(end_qp=153, p15_max=9, p16=0, byte_edge=5418, at_limit=7, outside=26, mvd_over=13, large=3133)),
    Case("112x64_high", 112, 64, 100, 0, 3, RE | BASE, dict(end_qp=164, p15_max=3, p16=6, byte_edge=4974, at_limit=7, outside=56, mvd_over=6, large=3011)),
    Case("112x64_high_bands", 112, 64, 100, 2, 3, RE | BASE, dict(end_qp=177, p15_max=13, p16=6, byte_edge=6674, at_limit=15, outside=57, mvd_over=34, large=4201)),
]
BY_NAME = {c.name: c for c in CASES}

# One decoder group of four 96x80 streams, step t = picture t of each.  The third stream is written WITHOUT the new bit (large
# levels of feature 512 only) and sits between streams with it.  The lists of large levels start at 1 024 entries and grow to
# twice what did not fit plus 1 024: GROUP_GROWTH are the steps at which the step's large levels outgrow the list, GROUP_LARGE the
# number of them per step (measured on the oracle; asserted by the CPU test).  At the first growth step no stream alone carries
# 1 024, two together do.
GROUP = [
    Case("group_0_baseline", 96, 80, 66, 0, 3, RE | BASE, None),
    Case("group_1_high", 96, 80, 100, 0, 2, RE | BASE, None),
    Case("group_2_plain", 96, 80, 77, 2, 2, BASE | 512, None),
    Case("group_3_main", 96, 80, 77, 0, 1, RE | BASE, None),
]
GROUP_GROWTH = (5, 9)
GROUP_LARGE = (21, 22, 65, 14, 25, 2516, 36, 53, 19, 11746, 8, 29)

Picture = namedtuple("Picture", "au idr mbqp mb levels planes stats hits max_level_prefix kinds mv4")
_cache = {}


def seed(case, i):
    return 6700417 * i + 131 * case.w + 7 * case.prof + 13 * case.slices + case.refs + (case.features & 0xFFFF) + 31 * len(case.name)


def stream(case):
    """the case's pictures: access unit, is_idr, QP_Y per macroblock, the writer's mbinfo and levels, the oracle decoder's three
    coded planes, its statistics, the writer's counters for this picture, the decoder's greatest level_prefix, its macroblock kinds
    and its (x, y, ref_idx_l0) of every 4x4 block (raster order; meaningful for inter macroblocks)"""
    if case.name in _cache:
        return _cache[case.name]
    enc = OracleEncoder(case.w, case.h, qp=30, gop=GOP, profile_idc=case.prof, slices=case.slices, refs=case.refs)
    dec = OracleDecoder()
    out = []
    for i in range(PICTURES):
        enc.hits_reset()
        au, idr, mbqp = enc.random_picture(seed(case, i), features=case.features)
        assert dec.decode(au) == 1, "%s picture %d: the independent decoder decodes every picture" % (case.name, i)
        out.append(Picture(au, idr, mbqp, enc.mbinfo(), enc.levels().astype(np.int32), [dec.plane(p) for p in range(3)], dec.stats(),
                           enc.hits(), dec.max_level_prefix, dec.mb_kinds(),
                           np.array([[dec.mb_mv(a, b) for b in range(16)] for a in range(len(mbqp))], np.int32)))
    enc.close()
    dec.close()
    _cache[case.name] = out
    return out


def large_levels(pic):
    """levels of the picture that do not fit the signed byte the product's upload gives each (-128 does)"""
    return int(((pic.levels > 127) | (pic.levels < -128)).sum())


def residual_kinds(pic):
    """per macroblock, which residual the dequantiser really works on (non-zero levels in lists the stream carries): 4x4 luma,
    8x8 luma, Intra16x16 DC, chroma DC, chroma AC - boolean arrays.  An inter macroblock of type P_8x8 sends
    transform_size_8x8_flag only when no quadrant is split, which the side information does not say: it counts for neither luma
    kind.  (i16_mode of an inter macroblock is its transform_size_8x8_flag.)"""
    mb, lv = pic.mb, pic.levels
    t, cbp = mb["type"], mb["cbp"].astype(np.int32)
    coded = ~np.isin(t, (2, 3))
    luma = coded & ((cbp & 15) != 0) & (np.abs(lv[:, LV_LUMA:LV_CHROMA_DC]).sum(axis=1) > 0)
    t8 = np.isin(t, (1, 5, 6)) & (mb["i16_mode"] == 1)
    t4 = (t == 4) | (np.isin(t, (1, 5, 6)) & (mb["i16_mode"] == 0)) | (t == 0)
    return {"luma4x4": luma & t4, "luma8x8": luma & t8,
            "i16_dc": (t == 0) & (np.abs(lv[:, LV_LUMA_DC:LV_LUMA]).sum(axis=1) > 0),
            "chroma_dc": coded & ((cbp >> 4) >= 1) & (np.abs(lv[:, LV_CHROMA_DC:LV_CHROMA_AC]).sum(axis=1) > 0),
            "chroma_ac": coded & ((cbp >> 4) == 2) & (np.abs(lv[:, LV_CHROMA_AC:]).sum(axis=1) > 0)}


def measure(case):
    """the quantities the floors are about, over the case's pictures"""
    pics = stream(case)
    m = dict(end_qp=0, p15_max=0, p16=0, byte_edge=0, mvd_over=0, large=0)
    limits, sides = np.zeros(4, np.int64), np.zeros(4, np.int64)
    for p in pics:
        coded = ~np.isin(p.mb["type"], (2, 3))
        m["end_qp"] += int((coded & np.isin(p.mbqp, QP_ENDS)).sum())
        m["p15_max"] += int(p.hits["re_prefix15_max"].sum())
        m["p16"] += int(p.hits["re_prefix16"].sum())
        m["byte_edge"] += int(np.isin(np.abs(p.levels), (127, 128, 129)).sum())
        m["mvd_over"] += int(p.hits["re_mvd_over_8192"])
        m["large"] = max(m["large"], large_levels(p))
        limits += p.hits["re_mv_limit"].astype(np.int64)
        sides += np.array([p.stats[k] for k in ("out_left", "out_right", "out_top", "out_bottom")], np.int64)
    m["at_limit"], m["outside"] = int(limits.min()), int(sides.min())
    return m
