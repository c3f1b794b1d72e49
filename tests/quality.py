"""The quality report (include/mi355x_h264.h, "quality report"): the definition restated in numpy, the case list, and the oracle's
expected records - what tests/test_quality_oracle.py (CPU: what the list holds) and tests/test_gpu_quality.py (GPU) share.

The definition, from the issue's text and not from the kernel.  Each of the three planes is compared sample by sample; Y, Cb, Cr
are reported in the order Y, U, V; the difference (src - rec) is squared and summed.  src is the picture the encoder kernels
read: the caller's samples for I420 and NV12 input, the I420 picture the RGBA conversion wrote for RGBA input.  rec is the
reconstruction that becomes the next reference, after the loop filter (an unfiltered picture as it stands).  Only display samples
count: luma x < width, y < height, chroma x < width / 2, y < height / 2.  A band instance counts the macroblock rows of its own
band.  Per picture: sse[3]; a map[mbh][mbw] whose entry is the macroblock's SSE over its display samples, the three planes
added, 0 outside the band.  The GPU's reconstruction equals the oracle's bit for bit, so the expected values are integer
arithmetic on the test's own input and OracleEncoder.recon(): nothing here has a tolerance.

Everything is deterministic; what is computed is computed once per process, shared and never changed."""
import functools
import math
from collections import namedtuple
import numpy as np
import ref_mix as rm
from media_amd import synth

Record = namedtuple("Record", "sse samples map")


def i420_planes(f, w, h):
    """(Y, U, V) of a tight I420 picture"""
    f = np.asarray(f, dtype=np.uint8)
    ysz, csz = w * h, (w // 2) * (h // 2)
    return f[:ysz].reshape(h, w), f[ysz:ysz + csz].reshape(h // 2, w // 2), f[ysz + csz:ysz + 2 * csz].reshape(h // 2, w // 2)


def nv12_planes(f, w, h):
    """(Y, U, V) of a tight NV12 picture: the interleaved plane taken apart"""
    f = np.asarray(f, dtype=np.uint8)
    uv = f[w * h: w * h * 3 // 2].reshape(h // 2, w // 2, 2)
    return f[: w * h].reshape(h, w), uv[:, :, 0], uv[:, :, 1]


def band_rows(h, slices, band_index=0, band_count=0):
    """(first macroblock row, rows) of a band instance: the rule of include/mi355x_h264.h (`slices`: bands of ceil(rows / n) rows,
    at least two rows each; band_index of band_count takes a contiguous run of whole slices)"""
    mbh = (h + 15) // 16
    if band_count <= 1:
        return 0, mbh
    n = min(max(slices, 1), max(1, mbh // 2))
    per = -(-mbh // n)
    nsl = -(-mbh // per)
    s0, s1 = band_index * nsl // band_count, (band_index + 1) * nsl // band_count
    return s0 * per, min(mbh, s1 * per) - s0 * per


def expected(src_planes, rec_planes, w, h, row0=0, rows=None):
    """Record of one picture.  src_planes: (Y, U, V) of the display size; rec_planes: (Y, U, V) of the coded size (or larger than
    the display size); row0, rows: the macroblock rows that count (a band instance's; default: all)"""
    mbw, mbh = (w + 15) // 16, (h + 15) // 16
    rows = mbh - row0 if rows is None else rows
    sse, samples = [0, 0, 0], [0, 0, 0]
    mp = np.zeros((mbh, mbw), np.uint64)
    for p in range(3):
        pw, ph, b = (w, h, 16) if p == 0 else (w // 2, h // 2, 8)
        d = src_planes[p][:ph, :pw].astype(np.int64) - rec_planes[p][:ph, :pw].astype(np.int64)   # display samples only
        sq = d * d
        y0, y1 = min(ph, row0 * b), min(ph, (row0 + rows) * b)
        sq[:y0] = 0
        sq[y1:] = 0
        sse[p] = int(sq.sum())
        samples[p] = (y1 - y0) * pw
        pad = np.zeros((mbh * b, mbw * b), np.int64)
        pad[:ph, :pw] = sq
        mp += pad.reshape(mbh, b, mbw, b).sum(axis=(1, 3)).astype(np.uint64)
    assert int(mp.sum()) == sum(sse) and int(mp.max()) <= 384 * 65025
    m = mp.astype(np.uint32)
    m.setflags(write=False)
    return Record(tuple(sse), tuple(samples), m)


def psnr(sse, samples):
    """10 * log10(255^2 * samples / sse); an SSE of 0 gives inf"""
    return math.inf if sse == 0 else 10.0 * math.log10(65025.0 * samples / sse)


def add(a, b):
    """the sum of two band records"""
    return Record(tuple(x + y for x, y in zip(a.sse, b.sse)), tuple(x + y for x, y in zip(a.samples, b.samples)), a.map + b.map)


# ---------------------------------------------------------------- content

def frame_rgba(w, h, i):
    """RGBA picture i: three pans of the synthetic texture as R, G, B, alpha 255; (h, w, 4) uint8"""
    r = synth._texture(w, h, -3 * i, -i, 1)
    g = synth._texture(w, h, 2 * i + 17, -2 * i + 5, 1)
    b = 255 - synth._texture(w, h, i + 40, 3 * i + 9, 1)
    a = np.full((h, w), 255, np.int32)
    return np.ascontiguousarray(np.clip(np.stack([r, g, b, a], axis=2), 0, 255).astype(np.uint8))


def frame_noise(w, h, i):
    return synth.frame_s3(w, h, i)


def frame_big_noise(w, h, i):
    """the 1080p picture of the issue: numpy.random.default_rng(1).integers(0, 256, w * h * 3 // 2)"""
    return np.random.default_rng(1 + i).integers(0, 256, w * h * 3 // 2).astype(np.uint8)


def frame_refs(w, h, i):
    c = rm.BY_NAME["split_48x48"]
    assert (w, h) == (c.w, c.h)
    return rm.frame_ref_mix(c.base, w, h, c.start + i, c.refs, c.seed)


def frame_plugin(w, h, i):
    """two pictures of the pan, then a cut to the pan averaged with noise: the P picture after the cut finds no match (the plugin's
    scene-change rule), and the IDR picture that replaces it is coded with an error (pure noise would go out as I_PCM, without one)"""
    f = synth.frame_s1(w, h, i)
    return f if i < 2 else ((f.astype(np.int32) + synth.frame_s3(w, h, i)) // 2).astype(np.uint8)


CONTENT = {"plugin": frame_plugin, "s1": synth.frame_s1, "scroll": synth.frame_scroll, "cut": synth.frame_cut, "split": synth.frame_split, "ramp": synth.frame_ramp,
           "noise": frame_noise, "big_noise": frame_big_noise, "refs": frame_refs}

# ---------------------------------------------------------------- the cases

Case = namedtuple("Case", "name kind w h qp gop pictures layout nodeblock slices refs prof start")


def case(name, kind, w, h, qp, gop, pictures, layout="i420", nodeblock=0, slices=0, refs=0, prof=66, start=0):
    return Case(name, kind, w, h, qp, gop, pictures, layout, nodeblock, slices, refs, prof, start)


CROP = case("crop_34x18", "s1", 34, 18, 30, 4, 5)                     # partial macroblocks on both axes, width % 4 == 2; IDR P P P IDR
PCM = case("pcm_48x48", "noise", 48, 48, 10, 4, 2)                     # I_PCM macroblocks: the picture is not filtered
NODEBLOCK = case("nodeblock_48x32", "s1", 48, 32, 34, 4, 3, nodeblock=1)
NV12 = case("nv12_50x34", "s1", 50, 34, 28, 4, 3, layout="nv12")
RGBA = case("rgba_40x24", "rgba", 40, 24, 28, 4, 3, layout="rgba")
# (the issue asks for at least 6 pictures; with the four ring slots of refs = 3 it takes eight to rewrite every slot once)
REFS3 = case("refs3_48x48", "refs", 48, 48, 26, 8, 8, refs=3)
SLICES = case("slices_96x80", "s1", 96, 80, 30, 4, 3, slices=2)
BIG = case("noise_1080p", "big_noise", 1920, 1080, 51, 4, 1)
# lockstep: three closed GOPs of three pictures, a content of its own each; four pictures back to back
GOPS = tuple(case("gops_64x48_%d" % g, kind, 64, 48, 28, 3, 3, start=st) for g, (kind, st) in enumerate((("s1", 0), ("scroll", 5), ("cut", 1))))
BATCH4 = case("batch4_64x48", "cut", 64, 48, 28, 30, 4)
# the hub: five streams of different content and QP
HUB_QPS = (20, 26, 32, 38, 44)
HUB = tuple(case("hub_64x48_%d" % k, kind, 64, 48, qp, 4, 6, start=st)
            for k, (qp, (kind, st)) in enumerate(zip(HUB_QPS, (("s1", 0), ("scroll", 3), ("cut", 0), ("split", 2), ("s1", 11)))))
HUB_DEVICE = 1        # this stream hands its pictures over in device memory
HUB_SITS_OUT = (3, 2)  # (stream, tick): the stream delivers no picture in that tick, so positions differ from items afterwards
SINGLE = (CROP, PCM, NODEBLOCK, NV12, RGBA, REFS3, SLICES)
PLUGIN = case("plugin_64x48", "plugin", 64, 48, 30, 30, 3)     # (the plugin surface takes GOP lengths from 30); the cut is picture 2
SCENE_CUT_COST_PER_MB = 3000     # VideoEncoderMI355X::Rc::kSceneCutCostPerMb


@functools.lru_cache(maxsize=None)
def frames(c):
    """the pictures as the caller hands them over: tight I420, tight NV12, or (h, w, 4) RGBA"""
    if c.layout == "rgba":
        out = tuple(frame_rgba(c.w, c.h, c.start + i) for i in range(c.pictures))
    else:
        out = tuple(np.ascontiguousarray(CONTENT[c.kind](c.w, c.h, c.start + i), dtype=np.uint8) for i in range(c.pictures))
        if c.layout == "nv12":
            out = tuple(rm.to_nv12(f, c.w, c.h) for f in out)
    for f in out:
        f.setflags(write=False)
    return out


def source_planes(c, f):
    """(Y, U, V) the encoder kernels read for the handed-over picture f, and the tight I420 picture the oracle codes"""
    from oracle_lib import rgba_to_i420
    if c.layout == "rgba":
        i420 = rgba_to_i420(f, c.w, c.h)
        return i420_planes(i420, c.w, c.h), i420
    if c.layout == "nv12":
        planes = nv12_planes(f, c.w, c.h)
        return planes, np.concatenate([np.ascontiguousarray(p).ravel() for p in planes])
    return i420_planes(f, c.w, c.h), f


def oracle_for(c, qp=None, **kw):
    from oracle_lib import OracleEncoder
    return OracleEncoder(c.w, c.h, qp=c.qp if qp is None else qp, gop=c.gop, profile_idc=c.prof, disable_deblock=c.nodeblock, slices=c.slices,
                         refs=c.refs, **kw)


Pic = namedtuple("Pic", "au idr rec coded mbtypes")   # rec: the Record; coded: the Record over the CODED size (replicated samples counted)


def _coded_record(c, src, recon):
    """what a comparison over the coded size would give: the source replicated to the coded size (the cropping test's foil)"""
    cw, ch = recon[0].shape[1], recon[0].shape[0]
    ext = [np.pad(s, ((0, (ch >> (p > 0)) - s.shape[0]), (0, (cw >> (p > 0)) - s.shape[1])), mode="edge") for p, s in enumerate(src)]
    return expected(ext, recon, cw, ch)


@functools.lru_cache(maxsize=None)
def oracle_run(c, qps=None, force_idr_at=()):
    """the oracle's stream of the case, a tuple of Pic; qps: a QP per picture (set before it)"""
    orc = oracle_for(c, qp=None if qps is None else qps[0])
    out = []
    for i, f in enumerate(frames(c)):
        if qps is not None and i:
            orc.set_qp(qps[i])
        src, i420 = source_planes(c, f)
        au, idr = orc.encode(i420, force_idr=i in force_idr_at)
        recon = tuple(orc.recon(p) for p in range(3))
        out.append(Pic(au, idr, expected(src, recon, c.w, c.h), _coded_record(c, src, recon), orc.mbinfo()["type"].copy()))
    orc.close()
    return tuple(out)


@functools.lru_cache(maxsize=None)
def oracle_bands(c, world=2):
    """`world` band instances of the oracle with halo swaps after every picture: per picture, (access unit put together, [Record per band])"""
    parts = [oracle_for(c, band_index=r, band_count=world) for r in range(world)]
    buf = np.zeros(parts[0].halo_bytes(), np.uint8)
    out = []
    for f in frames(c):
        src, i420 = source_planes(c, f)
        au = b"".join(p.encode(i420)[0] for p in parts)
        recs = []
        for r, p in enumerate(parts):
            row0, rows = band_rows(c.h, c.slices, r, world)
            recs.append(expected(src, tuple(p.recon(k) for k in range(3)), c.w, c.h, row0, rows))
        for r in range(world):
            if r > 0:
                parts[r].halo_export(0, buf.ctypes.data)
                parts[r - 1].halo_import(1, buf.ctypes.data)
            if r < world - 1:
                parts[r].halo_export(1, buf.ctypes.data)
                parts[r + 1].halo_import(0, buf.ctypes.data)
        out.append((au, tuple(recs)))
    for p in parts:
        p.close()
    return tuple(out)


@functools.lru_cache(maxsize=None)
def oracle_gops():
    """the lockstep batch: one oracle codes the closed GOP of item 0, item 1, .. (idr_pic_id runs on, as the engine's does)"""
    orc = oracle_for(GOPS[0])
    out = []
    for c in GOPS:
        gop = []
        for i, f in enumerate(frames(c)):
            src, i420 = source_planes(c, f)
            au, idr = orc.encode(i420, force_idr=i == 0)
            assert idr == (i == 0)
            gop.append(Pic(au, idr, expected(src, tuple(orc.recon(p) for p in range(3)), c.w, c.h), None, None))
        out.append(tuple(gop))
    orc.close()
    return tuple(out)


def plugin_replay(c, qps):
    """the plugin class's pictures on the oracle: picture i at QP qps[i]; a P picture whose motion cost exceeds the scene-change
    threshold is coded again as an IDR picture, and that is the picture that goes out.  A tuple of (Pic, was it re-coded)"""
    orc = oracle_for(c)
    nmb = ((c.w + 15) // 16) * ((c.h + 15) // 16)
    out = []
    for i, f in enumerate(frames(c)):
        orc.set_qp(qps[i])
        src, i420 = source_planes(c, f)
        au, idr = orc.encode(i420)
        cut = not idr and orc.me_cost() > SCENE_CUT_COST_PER_MB * nmb
        if cut:
            au, idr = orc.encode(i420, force_idr=True)
        out.append((Pic(au, idr, expected(src, tuple(orc.recon(p) for p in range(3)), c.w, c.h), None, None), cut))
    orc.close()
    return tuple(out)


def ring_rewrites(refs, pictures):
    """per ring slot of an encoder that keeps max(refs, 1) + 1 reconstructions: how often a picture was compared in it AFTER the slot
    had held an earlier picture (the slot of picture i is i mod slots)"""
    slots = max(refs, 1) + 1
    return [max(0, len(range(s, pictures, slots)) - 1) for s in range(slots)]
