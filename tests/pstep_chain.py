"""Inputs and expectations of tests/test_gpu_pstep_chain.py: closed GOPs of four pictures for the encoder's own lockstep steps
(capi.Encoder(batch = G), encode_gops_device) and for a batch-1 encoder, coded by ONE oracle as the consecutive GOPs of one stream
(item 0 of call 0, item 1, .., then call 1: idr_pic_id runs on as the engine's does).

The subject is the chain of a P step between the motion search and the loop filter (media_amd/csrc/engine.h submit_step): the
intra pass as one launch that decides as it goes and asks a flag of the whole STEP first (k_intra.h k_pintra_rows<.., DECIDE>), and
the motion-search lock given back by k_tq's first wave (k_tq.h tq_turn_release).  What can go wrong: a step whose flag is not
raised although one picture has marked macroblocks (they stay undecided and uncoded), a picture without marked macroblocks walked
as if it had some in a step whose flag is up, a macroblock decided from another item's source, Intra4x4 modes that do not reach
the entropy coder, a lock that is not given back.

Kinds: s1 (motion), s2 (a still picture: every P macroblock is P_Skip), split (partitions), cut2 / cut3 (the scene changes at
picture 2 / 3 of the GOP: that P picture has Intra4x4 macroblocks; the other P pictures of the GOP have no intra
macroblock, so a step of cut2 and cut3 items has the step's flag up and half the pictures' flags down, the other half in the
next step), patch (a still picture with one to three macroblocks of another scene per P picture: sparse intra), gradient (ramps:
Intra16x16 and Intra4x4 macroblocks in every P picture)."""
import functools
import numpy as np
import large_batch
from media_amd import synth
from oracle_lib import OracleEncoder

QP, GOP = 26, 4
MB_I16, MB_IPCM, MB_I4 = 0, 3, 4
# width, height: one macroblock; two beside each other; one column of three rows; 3 x 5 (an odd number of rows: the last pair wave
# of the filter has an upper row only); 11 x 9 (more than one wave per picture in every kernel, the XCD map of k_tq)
SIZES = ((16, 16), (32, 16), (16, 48), (48, 80), (176, 144))
PATTERN = ("s1", "s2", "cut2", "split", "cut3", "patch", "gradient", "cut2")   # item g of call c codes PATTERN[(g + c) % 8]


def pictures(kind, w, h, start):
    """the GOP pictures of one item, tight I420"""
    if kind in ("cut2", "cut3"):
        at = int(kind[3])
        return [synth.frame_s1(w, h, start + i) if i < at else synth.frame_cut(w, h, start + i + 2) for i in range(GOP)]
    if kind in ("s1", "s2", "split"):
        return synth.sequence(kind, w, h, GOP, start)
    return large_batch.pictures(kind, w, h, GOP, start)


def kinds_of(call, G, pattern=PATTERN):
    kinds = [pattern[(g + call) % len(pattern)] for g in range(G)]   # (`gradient` saturates at large picture indices: its starts stay small)
    return tuple((k, 1 + 2 * call if k == "gradient" else 5 * call + 3 * g + 1) for g, k in enumerate(kinds))


def frames(w, h, call, G, pattern=PATTERN):
    """[item][picture]"""
    return [pictures(k, w, h, s) for k, s in kinds_of(call, G, pattern)]


@functools.lru_cache(maxsize=None)
def expected(w, h, G, calls, slices=0, pattern=PATTERN):
    """out[call][item][picture] = dict(au, pre, post, types): the oracle's access unit, its reconstruction before and after the loop
    filter, the macroblock types.  Computed once per configuration and shared; nobody changes it"""
    orc = OracleEncoder(w, h, qp=QP, gop=GOP, slices=slices)
    out = []
    for call in range(calls):
        per_item = []
        for gop in frames(w, h, call, G, pattern):
            pics = []
            for i, f in enumerate(gop):
                au, idr = orc.encode(f)
                assert idr == (i == 0), "closed GOPs"
                planes = tuple(orc.recon(p) for p in range(3)) + tuple(orc.recon_pre(p) for p in range(3))
                for a in planes:
                    a.setflags(write=False)
                pics.append({"au": au, "post": planes[:3], "pre": planes[3:], "types": orc.mbinfo()["type"].copy()})
            per_item.append(pics)
        out.append(per_item)
    orc.close()
    return out


def intra_mbs(pic):
    return int(np.isin(pic["types"], (MB_I16, MB_IPCM, MB_I4)).sum())


def same(got, want, what):
    bad = np.argwhere(got != want)
    assert bad.size == 0, "%s: first differing sample (row, column) %s" % (what, bad[0])


def run_batch(w, h, G, calls, slices=0, pattern=PATTERN, enc=None):
    """the calls on capi.Encoder(batch = G): every item's GOP byte for byte, and item 0's last picture before and after the filter
    (PATTERN gives item 0 another kind in every call)"""
    import torch
    from media_amd import capi
    want = expected(w, h, G, calls, slices, pattern)
    fbytes = w * h * 3 // 2
    cap = 2 * GOP * fbytes + 4096
    own = enc is None
    if own:
        enc = capi.Encoder(w, h, qp=QP, gop=GOP, slices=slices, batch=G)
    try:
        enc.keep_pre()
        out, sizes, gb = np.zeros(G * cap, np.uint8), np.zeros(G * GOP, np.uint32), np.zeros(G, np.uint64)
        for call in range(calls):
            dev = torch.from_numpy(np.stack([f for gop in frames(w, h, call, G, pattern) for f in gop])).cuda()
            enc.encode_gops_device(dev.data_ptr(), fbytes, GOP * fbytes, GOP, out, cap, sizes, gb)
            kinds = kinds_of(call, G, pattern)
            for g in range(G):
                aus = [p["au"] for p in want[call][g]]
                assert [int(x) for x in sizes[g * GOP:(g + 1) * GOP]] == [len(a) for a in aus], "call %d item %d (%s): sizes[]" % (call, g, kinds[g][0])
                assert out[g * cap: g * cap + int(gb[g])].tobytes() == b"".join(aus), "call %d item %d (%s): the GOP's bytes" % (call, g, kinds[g][0])
            for p in range(3):
                same(enc.debug_read(capi.DBG_PRE_Y + p), want[call][0][-1]["pre"][p], "call %d item 0 (%s) plane %d before the filter" % (call, kinds[0][0], p))
                same(enc.debug_read(capi.DBG_RECON_Y + p), want[call][0][-1]["post"][p], "call %d item 0 (%s) plane %d" % (call, kinds[0][0], p))
            del dev
    finally:
        if own:
            enc.close()
