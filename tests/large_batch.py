"""The case list of the large lockstep steps: 25 to 64 pictures in one step, the sizes every published throughput figure comes
from (two engines of 32 closed GOPs, MAX_BATCH 64, a stream hub of up to 64 streams) and no other test reaches.
tests/test_large_batch_oracle.py proves on the CPU oracle alone that the list holds what it claims;
tests/test_gpu_large_batch.py runs it on the GPU and compares bytes, stages and statistics.

Above 24 pictures the IDR row wavefront (k_intra_rows) no longer holds all pictures of a step at once: workgroup (row, y) codes
pictures y, y + 24, y + 48 one after the other.  The pictures are small (64x48 = 4x3 macroblocks, 96x80, 176x144 with slices): a
few macroblocks each way are what the wavefronts need to have rows above and neighbours to the right; the subject is the COUNT.

Every item of a step has content of its own (a start offset per item, or another kind), so an item coded from another item's
arrays, hand-off area or header produces other bytes than the oracle's.  Everything is deterministic."""
import functools
import os
import re
from collections import namedtuple
import numpy as np
import adversarial
import stream_matrix as sm
from media_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# ---------------------------------------------------------------- content

PCM_KIND = "checker"    # the adversarial generator that outgrows CAVLC (I_PCM) at the QPs of the cases below
# one of each per eight items: ordinary motion (s1 - every sixteenth item s3 in its place - and scroll), a cut (Intra4x4 macroblocks
# in a P picture), partitions (split), a still picture (all P_Skip), the I_PCM content, ramps (gradient: Intra16x16 macroblocks in
# P pictures) and a new scene every picture (flip: every P picture is mostly intra)
PATTERN = ("s1", "cut", "split", "still", PCM_KIND, "gradient", "scroll", "flip")


def pictures(kind, w, h, n, start):
    """n tight I420 pictures of one item.  `cut` is synth's cut with a start: two pictures of the panning texture, then its
    mirrored, inverted twin; `still` repeats one picture of flat macroblocks (a level per macroblock and plane: the first picture is
    coded all but exactly, the others are all P_Skip at every QP); `patch` is a still picture in which, from the second picture on, one
    macroblock per picture (`start` picks which) shows another scene: that macroblock goes intra, the others are skipped"""
    if kind == "cut":
        return [synth.frame_s1(w, h, start + i) if i < 2 else synth.frame_cut(w, h, start + i) for i in range(n)]
    if kind == "still":
        mbw, mbh = w // 16, h // 16
        planes = [np.kron((16 + (adversarial._hash(start + seed, np.arange(mbw * mbh)) % 28) * 8).astype(np.uint8).reshape(mbh, mbw), np.ones((b, b), np.uint8))
                  for seed, b in ((0, 16), (500, 8), (900, 8))]
        return [np.concatenate([p.ravel() for p in planes])] * n
    if kind == "patch":
        out = []
        for i in range(n):
            f = synth.frame_s1(w, h, 1000 + start).copy()
            if i:
                other = synth.frame_cut(w, h, start + 7 * i + 2)
                mbw, mbh = w // 16, h // 16
                for k in range(1 + start % PATCH_MAX):
                    m = (5 * start + 3 * i + 7 * k) % (mbw * mbh)
                    _copy_mb(f, other, w, h, m % mbw, m // mbw)
            out.append(f)
        return out
    return sm.frames(sm.spec(kind, w, h, 66, 1, (26,) * n, start=start))


PATCH_MAX = 3   # a `patch` item replaces one to three macroblocks per P picture


def _copy_mb(dst, src, w, h, mx, my):
    y0, c0, c1 = 0, w * h, w * h * 5 // 4
    for r in range(16):
        o = y0 + (16 * my + r) * w + 16 * mx
        dst[o:o + 16] = src[o:o + 16]
    for base in (c0, c1):
        for r in range(8):
            o = base + (8 * my + r) * (w // 2) + 8 * mx
            dst[o:o + 8] = src[o:o + 8]


# ---------------------------------------------------------------- the direct cases (capi.Encoder(batch=G), encode_gops_device)

Case = namedtuple("Case", "name w h prof refs slices qp gop G calls kinds late")
# kinds: (kind, start) per item; late: the kinds that must lie at an item index >= 24 (and >= 48 when G >= 56)


def _items(G, rot=0, pattern=PATTERN):
    """item g takes pattern[(g + rot) % len]; its start offset is its own (`gradient` saturates at large picture indices: its
    starts stay small)"""
    kinds = [pattern[(g + rot) % len(pattern)] for g in range(G)]
    return tuple(("s3" if k == "s1" and g % 16 < 8 else k, 1 + 2 * (g // 8) if k == "gradient" else 3 * g + 1) for g, k in enumerate(kinds))


def case(name, w, h, prof, refs, slices, qp, gop, G, calls=2, kinds=None, late=None, rot=0):
    kinds = kinds or _items(G, rot)
    if late is None:
        late = frozenset(k for k, _ in kinds[24:])
    return Case(name, w, h, prof, refs, slices, qp, gop, G, calls, tuple(kinds), frozenset(late))


WALK_CASES = (
    case("baseline_64", 64, 48, 66, 0, 0, 12, 5, 64),          # MAX_BATCH: the walk 24 + 24 + 16
    case("high_40", 96, 80, 100, 0, 0, 12, 4, 40),             # k_tq8; 24 + 16: the second pass is not full
    case("main_2refs_25", 96, 80, 77, 2, 0, 12, 5, 25, rot=1),  # 24 + 1: item 24, the one picture walked to, holds the cut
    case("slices_32", 176, 144, 66, 0, 3, 12, 4, 32),          # three slices: three wavefronts per picture side by side
)

# the schedule switch (engine.h: p_intra_x16 against 16 * PINTRA_SPARSE_MBS).  sparse: one to three intra macroblocks per P
# picture in every fourth item, none in the others - the picture-walking launches of k_i4_decide / k_pintra_rows / the bS 4
# loop filter.  dense: every P picture of every item is mostly intra - all pictures resident, from the second call on
SPARSE = case("sparse_32", 96, 80, 66, 0, 0, 27, 4, 32, calls=3, late=(),
              kinds=tuple(("patch", g) if g % 4 == 1 else ("still", g) if g % 4 == 3 else ("scroll", 2 * g) for g in range(32)))
DENSE = case("dense_32", 96, 80, 66, 0, 0, 27, 4, 32, calls=3, late=(), kinds=tuple(("flip", 2 * g) for g in range(32)))
DIRECT_CASES = WALK_CASES + (SPARSE, DENSE)

# other slot counts (MI355X_H264_INTRA_SLOTS / MI355X_H264_PINTRA_SLOTS are read once per process: a fresh child process each,
# tests/large_batch_child.py).  The same walk with other remainders, cheap
SLOTS3_CASES = tuple(case("slots3_%s_%d" % (n, G), 64, 48, prof, 0, 0, 12, 4, G, late=())
                     for G in (8, 7) for n, prof in (("baseline", 66), ("high", 100)))          # 3 + 3 + 2 and 3 + 3 + 1
SLOTS1_CASE = case("slots1_4", 64, 48, 66, 0, 0, 12, 4, 4, late=())                                # every picture but the first is walked to
PSLOTS3_CASE = case("pslots3_dense_8", 96, 80, 66, 0, 0, 27, 4, 8, late=(), kinds=tuple(("flip", 2 * g) for g in range(8)))
CHILD_VARIANTS = {
    # name: (environment, direct cases)
    "intra_slots_3": ({"MI355X_H264_INTRA_SLOTS": "3"}, SLOTS3_CASES),
    # (the two variables act on different launches - IDR steps and P steps - and are independent of each other)
    "intra_slots_1_pintra_slots_3": ({"MI355X_H264_INTRA_SLOTS": "1", "MI355X_H264_PINTRA_SLOTS": "3"}, (SLOTS1_CASE, PSLOTS3_CASE)),
}


def by_name(name):
    for c in DIRECT_CASES + SLOTS3_CASES + (SLOTS1_CASE, PSLOTS3_CASE):
        if c.name == name:
            return c
    raise KeyError(name)


def frames(c, call, g):
    """the closed GOP of item g in call `call` (each call brings new pictures)"""
    kind, start = c.kinds[g]
    return pictures(kind, c.w, c.h, c.gop, start + (1 if kind == "gradient" else 11) * call)


def oracle_for(c):
    from oracle_lib import OracleEncoder
    return OracleEncoder(c.w, c.h, qp=c.qp, gop=c.gop, profile_idc=c.prof, slices=c.slices, refs=c.refs)


Pic = namedtuple("Pic", "au idr mbinfo mvq decision me_cost all_skip")
Stages = namedtuple("Stages", "mbinfo levels mvq mbaux pre recon")


class StagesOf:
    """what test_gpu_parity._compare_all reads of an oracle, kept from the moment the oracle had coded the picture"""

    def __init__(self, orc):
        self.s = Stages(orc.mbinfo(), orc.levels(), orc.mvq(), orc.mbaux(), [orc.recon_pre(p) for p in range(3)], [orc.recon(p) for p in range(3)])

    def mbinfo(self): return self.s.mbinfo
    def levels(self): return self.s.levels
    def mvq(self): return self.s.mvq
    def mbaux(self): return self.s.mbaux
    def recon_pre(self, p): return self.s.pre[p]
    def recon(self, p): return self.s.recon[p]


@functools.lru_cache(maxsize=None)
def expected(c, decode=False):
    """the oracle's serial stream of the case: one encoder codes the closed GOPs of call 0 item 0, item 1, .. then call 1 ..
    (idr_pic_id runs on, as the engine's does).  Returns (pics, stages): pics[call][g] = the GOP's Pic list, stages[call] = the
    stages of item 0's last picture.  decode: every access unit is also decoded by the independent decoder and held against
    the encoder's reconstruction.  Computed once per process and shared; nobody changes it"""
    from oracle_lib import OracleDecoder
    orc = oracle_for(c)
    dec = OracleDecoder() if decode else None
    pics, stages = [], []
    for call in range(c.calls):
        per_item = []
        for g in range(c.G):
            gop = []
            for i, f in enumerate(frames(c, call, g)):
                au, idr = orc.encode(f)
                assert idr == (i == 0), "closed GOPs"
                mb = orc.mbinfo()
                if dec:
                    assert dec.decode(au) == 1, (c.name, call, g, i)
                    for p in range(3):
                        assert np.array_equal(dec.plane(p), orc.recon(p)), "%s call %d item %d picture %d: decoder plane %d" % (c.name, call, g, i, p)
                gop.append(Pic(au, idr, mb, orc.mvq(), None if idr else orc.p_decision(), orc.me_cost(), (not idr) and bool((mb["type"] == 2).all())))
            if g == 0:
                stages.append(StagesOf(orc))
            per_item.append(gop)
        pics.append(per_item)
    orc.close()
    if dec:
        dec.close()
    return pics, stages


# ---------------------------------------------------------------- the schedule switch, restated

def _constant(name, text):
    m = re.search(r"\b%s\s*=\s*(\d+)" % name, text)
    assert m, "engine.h no longer defines %s" % name
    return int(m.group(1))


def engine_constants():
    """NSLOT, PINTRA_SPARSE_MBS and the default MI355X_H264_INTRA_SLOTS, read from media_amd/csrc/engine.h"""
    text = open(os.path.join(ROOT, "media_amd", "csrc", "engine.h")).read()
    m = re.search(r'getenv\("MI355X_H264_INTRA_SLOTS"\)\)\)\s*:\s*(\d+);', text)
    assert m, "engine.h: the default of MI355X_H264_INTRA_SLOTS"
    assert "e->p_intra_x16 = (3 * e->p_intra_x16 + 16 * (searched - tq_coded)) / 4;" in text, "engine.h: the running mean is no longer the one restated here"
    assert text.count("e->p_intra_x16 > 16u * PINTRA_SPARSE_MBS") == 2, "engine.h: the threshold of the schedule switch"
    return {"NSLOT": _constant("NSLOT", text), "PINTRA_SPARSE_MBS": _constant("PINTRA_SPARSE_MBS", text), "INTRA_SLOTS": int(m.group(1))}


def to_intra(pic):
    """macroblocks of a P picture the motion stage handed to the intra pass: what the device counts as searched - tq_coded"""
    return int((pic.decision == 1).sum())


def schedule(c, pics, k=None):
    """The running mean of engine.h (finish_item), restated: p <- (3 p + 16 x) / 4 in integers for every finished item of a P
    picture, x its macroblocks handed to the intra pass, item 0 first.  A call keeps NSLOT - 1 pictures in flight (run_pipeline):
    picture i is submitted when pictures 0 .. i - NSLOT + 1 of the call have been finished, and the mean as it stands then picks
    the grids of the step.  Returns [(call, picture, mean at its submission)] for every P picture; dense is mean > 16 * PINTRA_SPARSE_MBS"""
    k = k or engine_constants()
    p, out = 0, []

    def fold(call, i):
        nonlocal p
        if i:   # (IDR pictures leave the mean alone)
            for g in range(c.G):
                p = (3 * p + 16 * to_intra(pics[call][g][i])) // 4

    for call in range(c.calls):
        for i in range(c.gop):
            if i >= k["NSLOT"] - 1:
                fold(call, i - (k["NSLOT"] - 1))
            if i:
                out.append((call, i, p))
        for i in range(max(0, c.gop - (k["NSLOT"] - 1)), c.gop):
            fold(call, i)
    return out


# ---------------------------------------------------------------- the hub groups (capi.Stream through tools/stream_tick.cpp)

HUB_SIZE = (64, 48)
HUB_PICTURES, HUB_GOP = 6, 3     # a second IDR picture arrives while P steps are in flight
HUB_ITEMS = 64                   # MI355X_H264_HUB_ITEMS (default 32), set before the group's first stream opens
HUB_KINDS = ("s1", "flip", "split", "bars", PCM_KIND, "s3", "scroll", "gradient", "glyphs", "noise", "contrast", "ramp")


def hub_group(n, prof=66, nv12_device=False):
    """n streams of one engine, a QP of its own each (10 .. 51, then again), contents in turn"""
    w, h = HUB_SIZE
    out = []
    for k in range(n):
        kind = HUB_KINDS[k % len(HUB_KINDS)]
        out.append(sm.spec(kind, w, h, prof, HUB_GOP, (10 + k % 42,) * HUB_PICTURES, nv12_device=nv12_device, start=k // 12 if kind == "gradient" else k))
    return out


HUB_GROUPS = {"48_nv12_device_high": lambda: hub_group(48, 100, True), "64_baseline": lambda: hub_group(64, 66)}

# the indirect walk (k_intra_rows<true>): a child process with two intra slots and twelve streams.  The first stream to arrive
# leads an IDR step alone and the next IDR step takes whatever queued meanwhile (hub_sched.h), so of twelve pictures that start
# together the second step holds most of the other eleven
HUB_WALK_SLOTS, HUB_WALK_STREAMS = 2, 12


# ---------------------------------------------------------------- running a direct case on the GPU

def expected_stats(c, pics, call, nmb):
    """what mi355x_h264_stats holds after one call, from the case's geometry and the oracle's decisions.  Per step submit_step
    records: an IDR step one k_intra_rows launch; a P step one k_me launch per reference picture it may use (min(refs,
    pictures since the IDR)) and one k_tq / k_tq8 launch; every step four entropy launches and one loop-filter launch - each
    over every macroblock of every item.
    searched (me_searched_mbs) are the macroblocks none of k_me's two "nothing left to code" tests settled; the oracle's seeded
    search restates those tests exactly (oracle/h264_enc.c, mv_all_zero at the zero vector and at the previous vector rounded to
    whole samples, first reference picture only - k_me settles under rf == 0 only), so the count is an equality, not a bound.
    searched - tq_coded are the macroblocks k_me marked for the intra pass (bit 15 of me_cost).  The mark is set when k_me
    decides and is never taken back: a marked macroblock that outgrows CAVLC in k_pintra_rows and becomes I_PCM keeps it, an
    inter macroblock that k_tq turns into I_PCM never had it.  MbInfo.type == I_PCM does not tell the two apart; the oracle's
    record of the decision (OracleEncoder.p_decision) does"""
    p_pics = [p for g in range(c.G) for p in pics[call][g][1:]]
    all_mbs = nmb * c.G
    return {"frames": c.gop * c.G, "p_mbs": (c.gop - 1) * all_mbs,
            "to_intra": sum(to_intra(p) for p in p_pics),
            "searched": sum(int((p.decision != 2).sum()) for p in p_pics),
            "not_skipped_or_coded": sum(int(((p.mbinfo["type"] != 2) & ~((p.mbinfo["type"] == 1) & (p.mbinfo["cbp"] == 0))).sum()) for p in p_pics),
            "kernels": {"intra": (1, all_mbs), "me": (sum(min(max(c.refs, 1), i) for i in range(1, c.gop)), (c.gop - 1) * all_mbs),
                        "tq": (c.gop - 1, (c.gop - 1) * all_mbs), "cavlc": (4 * c.gop, c.gop * all_mbs), "deblock": (c.gop, c.gop * all_mbs)}}


def run_direct(c, after_call=None):
    """the case on capi.Encoder(batch = G): per call, every item's closed GOP against the oracle's serial stream (bytes and
    sizes[]), the per-item scene-change statistic and the statistics counters.  after_call(enc, call, stages) may compare the
    stages of item 0.  Returns the list of differences found (empty: the GPU coded what the oracle coded)"""
    import torch
    from media_amd import capi
    pics, stages = expected(c)
    bad = []
    enc = capi.Encoder(c.w, c.h, qp=c.qp, gop=c.gop, profile_idc=c.prof, slices=c.slices, refs=c.refs, batch=c.G)
    try:
        enc.keep_pre(True)
        enc.stats_enable(True)
        fbytes = c.w * c.h * 3 // 2
        cap = 2 * c.gop * fbytes + 4096     # (an I_PCM picture is a little larger than its samples)
        out, sizes, gb = np.zeros(c.G * cap, np.uint8), np.zeros(c.G * c.gop, np.uint32), np.zeros(c.G, np.uint64)
        for call in range(c.calls):
            dev = torch.from_numpy(np.stack([f for g in range(c.G) for f in frames(c, call, g)])).cuda()
            enc.encode_gops_device(dev.data_ptr(), fbytes, c.gop * fbytes, c.gop, out, cap, sizes, gb)
            for g in range(c.G):
                want = [p.au for p in pics[call][g]]
                if out[g * cap: g * cap + int(gb[g])].tobytes() != b"".join(want):
                    bad.append("call %d item %d (%s): the GOP's bytes differ from the oracle's" % (call, g, c.kinds[g][0]))
                if [int(x) for x in sizes[g * c.gop:(g + 1) * c.gop]] != [len(x) for x in want]:
                    bad.append("call %d item %d (%s): sizes[]" % (call, g, c.kinds[g][0]))
            cost = enc.me_cost()
            for g in range(c.G):
                if int(cost[g]) != pics[call][g][-1].me_cost:
                    bad.append("call %d item %d: me_cost %d, the oracle's %d" % (call, g, int(cost[g]), pics[call][g][-1].me_cost))
            st, want = enc.stats(reset=True), expected_stats(c, pics, call, enc.nmb)
            print("%s call %d: stats %s" % (c.name, call, {k: v for k, v in st.items() if k != "kernels"}))
            got = {"frames": st["frames"], "p_mbs": st["p_mbs"], "to_intra": st["me_searched_mbs"] - st["tq_coded_mbs"], "searched": st["me_searched_mbs"]}
            for key, v in got.items():
                if v != want[key]:
                    bad.append("call %d: statistics %s = %d, expected %d" % (call, key, v, want[key]))
            if not st["tq_coded_mbs"] <= st["me_searched_mbs"] <= st["p_mbs"]:
                bad.append("call %d: tq_coded_mbs <= me_searched_mbs <= p_mbs does not hold: %s" % (call, st))
            if st["me_searched_mbs"] < want["not_skipped_or_coded"]:
                bad.append("call %d: me_searched_mbs %d below the %d macroblocks that were coded" % (call, st["me_searched_mbs"], want["not_skipped_or_coded"]))
            for name, (launches, mbs) in want["kernels"].items():
                if (st["kernels"][name]["launches"], st["kernels"][name]["mbs"]) != (launches, mbs):
                    bad.append("call %d: kernel %s launches / mbs %s, expected %s" % (call, name, (st["kernels"][name]["launches"], st["kernels"][name]["mbs"]), (launches, mbs)))
            if after_call:
                after_call(enc, call, stages[call])
            del dev
    finally:
        enc.close()
    return bad
