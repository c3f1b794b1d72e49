"""The case list of the stream-hub matrix: which streams, of which content, geometry, options and per-picture QPs, are opened
together on one shared engine.  tests/test_stream_matrix_oracle.py proves on the CPU oracle alone that the list reaches what it
is meant to reach; tests/test_gpu_stream_matrix.py runs the same list through capi.Stream (the IND = true kernels).

A case is a Spec (one stream); a group is a list of Specs of ONE geometry and configuration, so that the hub puts them on one
engine and their pictures share lockstep steps.  Everything is deterministic: contents are seeded, the random sizes are drawn
from a seeded generator the way test_randomized_configurations draws its own."""
import random
from collections import namedtuple
import numpy as np
import adversarial
from media_amd import synth

Spec = namedtuple("Spec", "kind w h prof gop qps slices search nodeblock nv12_device start force_idr_at")


def spec(kind, w, h, prof, gop, qps, slices=0, search=1, nodeblock=0, nv12_device=False, start=0, force_idr_at=()):
    return Spec(kind, w, h, prof, gop, tuple(qps), slices, search, nodeblock, nv12_device, start, tuple(force_idr_at))


SYNTH_KINDS = ("s1", "scroll", "split", "cut", "s3", "ramp", "s2")
KINDS = tuple(adversarial.GENERATORS) + SYNTH_KINDS


def _noise(w, h, index):
    """black / white noise: at QP 10 every macroblock outgrows CAVLC and goes I_PCM, in IDR and in P pictures"""
    rng = np.random.default_rng(1000 + index)
    return (rng.integers(0, 2, w * h * 3 // 2, dtype=np.uint8) * 255).astype(np.uint8)


def _flip(w, h, index):
    """another scene every picture (the panning texture and its mirrored, inverted twin of synth's `cut` in turn): every P picture
    finds no match and hands macroblocks to the intra pass"""
    return synth.frame_s1(w, h, index) if index % 2 == 0 else synth.frame_cut(w, h, index + 2)


def frames(s):
    """the pictures of a stream: tight I420, one per entry of s.qps"""
    n = len(s.qps)
    if s.kind in adversarial.GENERATORS:
        return adversarial.sequence(s.kind, s.w, s.h, n, start=s.start)
    if s.kind == "noise":
        return [_noise(s.w, s.h, s.start + i) for i in range(n)]
    if s.kind == "flip":
        return [_flip(s.w, s.h, s.start + i) for i in range(n)]
    return synth.sequence(s.kind, s.w, s.h, n, start=s.start)


def is_idr(s, i, state):
    """picture type of picture i by the encoder's rule (first picture, GOP length, forced); state: a dict kept per stream"""
    idr = i == 0 or i in s.force_idr_at or state.get("in_gop", 0) >= s.gop
    state["in_gop"] = 1 if idr else state["in_gop"] + 1
    return idr


# ---------------------------------------------------------------- 1. every QP, in shared steps

ALL_QP_STREAMS = 21
ALL_QP_GOP = 4


def all_qp_walk(k):
    """QPs of the eight pictures (IDR P P P | IDR P P P) of stream k, base b = 10 + 2k: b and b + 1 each in an IDR and in a P
    picture (21 streams: every QP 10..51), one P picture at a range end, and in the second GOP the walk 10 -> 51 -> 10 (odd
    streams 51 -> 10 -> 51, so that the range ends sit BESIDE each other in a step)"""
    b = 10 + 2 * k
    lo, hi = (10, 51) if k % 2 == 0 else (51, 10)
    return (b, b + 1, lo, b, b + 1, lo, hi, lo)


def all_qps(prof):
    """21 streams of adversarial.SIZE, a different content each (`cut` cuts at its picture 2, a P picture)"""
    w, h = adversarial.SIZE
    return [spec(KINDS[k % len(KINDS)], w, h, prof, ALL_QP_GOP, all_qp_walk(k), start=0 if KINDS[k % len(KINDS)] == "cut" else k)
            for k in range(ALL_QP_STREAMS)]


# ---------------------------------------------------------------- 2. the saturation matrix, one reference picture

SAT_QPS = (10, 51)
SAT_PROFILES = (66, 100)


def saturation(prof):
    """every adversarial content at QP 10 and at QP 51, adversarial.PICTURES pictures of one GOP: twelve streams of one engine"""
    w, h = adversarial.SIZE
    return [spec(kind, w, h, prof, adversarial.GOP, (qp,) * adversarial.PICTURES) for kind in adversarial.GENERATORS for qp in SAT_QPS]


# What a stream can reach of the counters tests/test_gpu_saturation.py pins: the oracle's counts on saturation(66) +
# saturation(100), per content, less about a tenth (that file's convention), computed by tests/test_stream_matrix_oracle.py
# (print_counts()).  One reference picture, QP 10 and 51 only - these are not the three-reference numbers.
FLOOR_KEYS = ("frac_x", "frac_y", "frac_xy", "mv_outside", "mc_clipped", "i16_plane_clamped", "chroma_plane_clamped", "pcm",
              "lp15_qp10_12", "lp15_qp49_51", "tc16")
FLOORS = {}   # filled below


# ---------------------------------------------------------------- 3. per-item flags beside each other

FLAGS_SIZE = (352, 288)
FLAGS_PICTURES = 6
FLAGS_IDLE = 3          # streams opened and never used: they raise the P share (hub_sched.h, p_share) to five pictures


def flags(order):
    """two I_PCM streams (noise at QP 10: slice header idc 1, not filtered), two static ones (all P_Skip) and two whose every
    P picture has intra macroblocks; `order` permutes the opening order, and with it the batch items"""
    w, h = FLAGS_SIZE
    base = [spec("noise", w, h, 66, 30, (10,) * FLAGS_PICTURES), spec("s2", w, h, 66, 30, (40,) * FLAGS_PICTURES),
            spec("flip", w, h, 66, 30, (28,) * FLAGS_PICTURES), spec("noise", w, h, 66, 30, (10,) * FLAGS_PICTURES, start=50),
            spec("s2", w, h, 66, 30, (46,) * FLAGS_PICTURES), spec("flip", w, h, 66, 30, (36,) * FLAGS_PICTURES, start=4)]
    return [base[i] for i in order]


FLAGS_ORDERS = ((0, 1, 2, 3, 4, 5), (5, 2, 4, 1, 3, 0))


# ---------------------------------------------------------------- 4. geometry sweep

FIXED_SIZES = ((16, 16), (32, 16), (16, 48), (18, 18), (50, 34), (130, 98), (2048, 16), adversarial.SIZE)
RANDOM_SIZES = 24
GEOMETRY_PICTURES = 4


def geometry():
    """groups of three streams: the fixed sizes (one macroblock, one row, one column, crops, odd macroblock counts, wide and
    flat), then seeded random even sizes; loop filter on / off, search 0 / 1, slices 0 / 3, I420 from the host or NV12 from device
    memory, profile and QPs drawn per group"""
    rng = random.Random(20261017)
    groups = []
    for c in range(len(FIXED_SIZES) + RANDOM_SIZES):
        w, h = FIXED_SIZES[c] if c < len(FIXED_SIZES) else (2 * rng.randint(8, 200), 2 * rng.randint(8, 150))
        nodb, search, slices, nv12 = c & 1, (c >> 1) & 1, 3 * ((c >> 2) & 1), (c >> 3) & 1
        if c >= 16:
            nodb, search, slices, nv12 = int(rng.random() < 0.5), int(rng.random() < 0.5), 3 * int(rng.random() < 0.5), rng.random() < 0.5
        prof = rng.choice([66, 77, 100])
        gop = rng.choice([2, 3, 5])
        kinds = ["ramp" if c % 8 == 7 else rng.choice(["s1", "scroll", "split", "glyphs", "contrast", "checker"]), rng.choice(["s1", "s3", "cut", "bars"]),
                 rng.choice(["scroll", "split", "gradient", "s2"])]
        group = []
        for k, kind in enumerate(kinds):
            q0 = rng.choice([10, 14, 22, 26, 31, 37, 44, 51])
            qps = tuple(min(51, max(10, q0 + ((i * (k + 2)) % 5) - 2)) for i in range(GEOMETRY_PICTURES))
            group.append(spec(kind, w, h, prof, gop, qps, slices=slices, search=search, nodeblock=nodb, nv12_device=bool(nv12),
                              start=0 if kind == "cut" else 3 * k))
        groups.append(group)
    return groups


# ---------------------------------------------------------------- 5. both forms of the loop filter, indirect

FILTER_FORM_SIZES = ((176, 112), (64, 16), (16, 64))
FILTER_FORM_STREAMS = 30      # P share (30 + 2) / 3 = 10 pictures: steps of eight or more take k_deblock_pairs


def filter_forms(w, h):
    return [spec(KINDS[k % len(KINDS)], w, h, 66, 3, tuple(min(51, 12 + k + 9 * (i % 2)) for i in range(5)), start=0 if KINDS[k % len(KINDS)] == "cut" else k)
            for k in range(FILTER_FORM_STREAMS)]


# ---------------------------------------------------------------- 6. forced IDR and churn

def churn():
    """five streams; stream 1 is forced to an IDR picture at its picture 3 while the others go on"""
    w, h = adversarial.SIZE
    return [spec(kind, w, h, 100, 30, tuple(qp0 + (i % 3) for i in range(8)), force_idr_at=(3,) if k == 1 else (), start=0 if kind == "cut" else k)
            for k, (kind, qp0) in enumerate((("s1", 24), ("glyphs", 12), ("scroll", 33), ("cut", 45), ("split", 28)))]


CHURN_CLOSE_AT, CHURN_CLOSE_STREAM = 5, 2      # before picture 5, stream 2 closes and CHURN_NEWCOMER opens on its item
CHURN_NEWCOMER = spec("contrast", adversarial.SIZE[0], adversarial.SIZE[1], 100, 30, (49, 10, 51))


# ---------------------------------------------------------------- 7. full size, once

def full_size():
    return [spec(kind, 1920, 1080, 66, 30, (qp,) * 3, start=k) for k, (kind, qp) in enumerate((("s1", 26), ("glyphs", 40), ("s1", 18), ("glyphs", 31)))]


def oracle_for(s):
    from oracle_lib import OracleEncoder
    return OracleEncoder(s.w, s.h, qp=s.qps[0], gop=s.gop, profile_idc=s.prof, disable_deblock=s.nodeblock, slices=s.slices, search=s.search)


def tally(cov, qp, mbinfo, max_level_prefix, before):
    """adversarial.tally for pictures of any QP: its level_prefix 15 counters are those of the range ends only"""
    lp = max_level_prefix if (qp <= 12 or qp >= 49) else 0
    adversarial.tally(cov, qp, mbinfo, lp, before, cov)


def short_of_floors(kind, cov):
    return ["%s %d < %d" % (k, cov.get(k, 0), v) for k, v in FLOORS[kind].items() if cov.get(k, 0) < v]


def cpu_groups():
    """what the oracle-side test runs: the groups that carry the QP, content and flag coverage (the geometry groups, the
    filter-form groups and the full-size group are checked as lists: their sizes are asserted, their pictures are not coded)"""
    return [all_qps(66), all_qps(100), saturation(66), saturation(100), flags(FLAGS_ORDERS[0])]


FLOORS.update({
    "glyphs": {"frac_x": 333, "frac_y": 317, "frac_xy": 290, "mv_outside": 180, "mc_clipped": 369, "pcm": 222, "lp15_qp10_12": 10, "lp15_qp49_51": 1, "tc16": 590},
    "checker": {"frac_x": 203, "frac_y": 78, "frac_xy": 68, "mv_outside": 96, "mc_clipped": 226, "pcm": 521, "lp15_qp10_12": 10, "lp15_qp49_51": 3, "tc16": 154},
    "gradient": {"frac_y": 54, "frac_xy": 29, "mv_outside": 14, "i16_plane_clamped": 23, "chroma_plane_clamped": 126, "pcm": 4, "lp15_qp10_12": 10, "lp15_qp49_51": 7, "tc16": 3},
    "flat_flip": {"lp15_qp10_12": 9, "lp15_qp49_51": 9},
    "contrast": {"frac_x": 340, "frac_y": 286, "frac_xy": 1151, "mv_outside": 128, "mc_clipped": 99, "pcm": 703, "lp15_qp10_12": 10, "tc16": 113},
    "bars": {"frac_x": 138, "frac_y": 50, "frac_xy": 10, "mc_clipped": 22, "lp15_qp10_12": 10, "lp15_qp49_51": 1},
})
