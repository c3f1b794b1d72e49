"""The sub-sample stage of the motion search (media_amd/csrc/k_me.h sections 3, 4, 4b and the prediction write-out: the
half-sample plane build, round 0 with its single tap, round 1 and the partition path with the tap table in LDS) against the CPU
oracle, bit for bit: access units, MbInfo, quadrant vectors, levels, pre-filter and final planes.

128x96 is the smallest picture with macroblocks on both window-load paths (the fixed pattern needs mx in 2..5 and my in 2..3;
every macroblock at the picture edge takes the clamped one) and with plane grids that reach the window rows and columns next
to the clamped apron.  Contents:
  pan     S1 (pan + noise) at QP 26: fractional vectors, winners of the seeded test and of the exhaustive pass
  phases  `scroll` with a sub-sample pan.  synth's own `scroll` pans by whole samples, (+4, +2) per picture, and has no
          fractional pan to set; on the oracle its winners at this size and QP 24 reach 15 of the 16 phases (none at
          mvx & 3 = 3, mvy & 3 = 2; 201 of 288 on integer positions; seeded and exhaustive alike), the fractional ones only where
          the search misses the pan.  So the same noise-free texture is evaluated on a 4x finer grid and panned in 32x32
          tiles, each tile by its own quarter-sample step, another one every picture:
          every one of the 16 quarter-sample phases wins somewhere (asserted on the oracle alone, without a GPU, too)
  noise   S3 noise at QP 40 (at low QP its macroblocks go I_PCM): every searched macroblock's cost is far above PART_TEST_MIN,
          so the partition path runs (its `eval` looks the taps up per lane), partitions win here and there (the write-out
          takes its per-quadrant branch) and most macroblocks are handed to the intra pass
Each with the seeded and the exhaustive integer search, frame by frame (batch 1) and as a lockstep batch of 8 GOPs; one
stream of the hub (the IND = true instantiation) on top."""
import functools
import numpy as np
import pytest
import stream_matrix as sm
from media_amd import synth
from oracle_lib import OracleEncoder

W, H, GOP, G = 128, 96, 7, 8      # 1 IDR + 6 P pictures per GOP; 8 GOPs in a lockstep batch
QP = {"pan": 26, "phases": 24, "noise": 40}
KINDS = ("pan", "phases", "noise")


def _phase_step(tile, k):
    """quarter-sample step (x, y) of tile `tile` between pictures k and k + 1: walks all 16 phases, tiles 5 apart"""
    n = (5 * tile + k) % 16
    return n & 3, n >> 2


def frame_phases(index):
    """synth's noise-free texture (frame_s1 with noise = 0, what `scroll` is made of), evaluated on a 4x finer grid and
    sub-sampled, so that a shift by quarter samples is a true shift, in 32x32 tiles; tile t has moved by the sum of its first
    `index` steps.  Static chroma (the first picture's)."""
    y = np.empty((H, W), np.uint8)
    for ty in range(H // 32):
        for tx in range(W // 32):
            t = ty * (W // 32) + tx
            ox = sum(_phase_step(t, k)[0] for k in range(index))
            oy = sum(_phase_step(t, k)[1] for k in range(index))
            fine = synth.frame_s1(4 * W, 4 * H, 1, noise=0, motion=(ox - 37 * t, oy))[: 16 * W * H].reshape(4 * H, 4 * W)[::4, ::4]
            y[32 * ty: 32 * ty + 32, 32 * tx: 32 * tx + 32] = fine[32 * ty: 32 * ty + 32, 32 * tx: 32 * tx + 32]
    return np.concatenate([y.ravel(), synth.frame_s1(W, H, 0, noise=0)[W * H:]])


def _frames(kind, count):
    if kind == "pan":
        return synth.sequence("s1", W, H, count)
    if kind == "noise":
        return synth.sequence("s3", W, H, count)
    return [frame_phases(i % GOP) for i in range(count)]   # every GOP of the batch: the same walk from its own IDR picture


@functools.lru_cache(maxsize=None)
def reference(kind, search):
    """the oracle's G GOPs, computed once per (content, search mode): frames, access units and, for the first GOP (what the
    frame-by-frame test compares), nothing more than the encoder itself - the stage comparison replays it"""
    frames = _frames(kind, G * GOP)
    orc = OracleEncoder(W, H, qp=QP[kind], gop=GOP, search=search)
    aus, phases, types = [], np.zeros(16, np.int64), np.zeros(8, np.int64)
    for f in frames:
        au, idr = orc.encode(f)
        aus.append(au)
        if not idr:
            mb = orc.mbinfo().reshape(-1)
            inter = np.isin(mb["type"], (1, 2, 5, 6, 7))
            types += np.bincount(mb["type"], minlength=8)[:8]
            phases += np.bincount((mb["mvy"][inter] & 3) * 4 + (mb["mvx"][inter] & 3), minlength=16)
    orc.close()
    return frames, aus, phases, types


@pytest.mark.parametrize("search", [1, 0], ids=["seeded", "exhaustive"])
def test_content_reaches_what_it_is_meant_to_reach(search):
    """no GPU: the oracle alone shows that the `phases` content makes every quarter-sample phase win, that `pan` has
    fractional vectors and that partitions win on `noise`"""
    _, _, phases, _ = reference("phases", search)
    print("phases: winners per (mvy & 3) * 4 + (mvx & 3):", phases.tolist())
    assert (phases > 0).all(), phases.tolist()
    _, _, pan, _ = reference("pan", search)
    assert pan[1:].sum() > 0 and pan[0] > 0, pan.tolist()
    _, _, _, types = reference("noise", search)
    print("noise: macroblock types of the P pictures:", types.tolist())
    assert types[5] + types[6] + types[7] > 0, types.tolist()


@pytest.mark.gpu
@pytest.mark.parametrize("search", [1, 0], ids=["seeded", "exhaustive"])
@pytest.mark.parametrize("kind", KINDS)
def test_frame_by_frame_every_stage(kind, search):
    from media_amd import capi
    from test_gpu_parity import _compare_all
    frames, aus, _, _ = reference(kind, search)
    enc = capi.Encoder(W, H, qp=QP[kind], gop=GOP, search=search)
    enc.keep_pre(True)
    orc = OracleEncoder(W, H, qp=QP[kind], gop=GOP, search=search)
    seen = np.zeros(16, np.int64)
    for i in range(GOP + 1):          # one GOP and the IDR picture after it
        au, _ = enc.encode(frames[i])
        want, idr = orc.encode(frames[i])
        assert want == aus[i]
        assert au == want, "%s picture %d: access unit" % (kind, i)
        _compare_all(enc, orc, "%s picture %d" % (kind, i))
        if not idr:
            mb = enc.debug_read(capi.DBG_MBINFO).reshape(-1)
            inter = np.isin(mb["type"], (1, 2, 5, 6, 7))
            seen += np.bincount((mb["mvy"][inter] & 3) * 4 + (mb["mvx"][inter] & 3), minlength=16)
    if kind == "phases":   # all 16 values of (mvx & 3, mvy & 3) among the GPU's winning vectors
        assert (seen > 0).all(), seen.tolist()
    enc.close()
    orc.close()


@pytest.mark.gpu
@pytest.mark.parametrize("search", [1, 0], ids=["seeded", "exhaustive"])
@pytest.mark.parametrize("kind", KINDS)
def test_lockstep_batch_of_eight(kind, search):
    import torch
    from media_amd import capi
    frames, aus, _, _ = reference(kind, search)
    fbytes = W * H * 3 // 2
    dev = torch.from_numpy(np.stack(frames)).cuda()
    enc = capi.Encoder(W, H, qp=QP[kind], gop=GOP, batch=G, search=search)
    cap = 2 * GOP * fbytes
    out, sizes, gb = np.zeros(G * cap, np.uint8), np.zeros(G * GOP, np.uint32), np.zeros(G, np.uint64)
    enc.encode_gops_device(dev.data_ptr(), fbytes, GOP * fbytes, GOP, out, cap, sizes, gb)
    for g in range(G):
        assert out[g * cap: g * cap + int(gb[g])].tobytes() == b"".join(aus[g * GOP:(g + 1) * GOP]), "%s GOP %d" % (kind, g)
        assert [int(x) for x in sizes[g * GOP:(g + 1) * GOP]] == [len(a) for a in aus[g * GOP:(g + 1) * GOP]]
    enc.close()


@pytest.mark.gpu
def test_one_stream_of_the_hub():
    """the IND = true instantiation: one stream of the hub, the `phases` content, every stage"""
    from media_amd import capi
    from test_gpu_parity import _compare_all
    s = sm.spec("s1", W, H, 66, GOP, (QP["phases"],) * GOP)
    frames, aus, _, _ = reference("phases", s.search)
    stream = capi.Stream(s.w, s.h, qp=s.qps[0], gop=s.gop, profile_idc=s.prof, search=s.search)
    stream.keep_pre(True)
    orc = sm.oracle_for(s)
    for i in range(GOP):
        au = stream.encode(frames[i])[0]
        assert orc.encode(frames[i])[0] == aus[i]
        assert au == aus[i], "picture %d: access unit" % i
        _compare_all(stream, orc, "hub picture %d" % i)
    stream.close()
    orc.close()
