"""The "nothing left to code" tests of the motion search (media_amd/csrc/k_me.h section 1) and the cheap exact rejects in front
of them - the luma block sums, the chroma DC - against the CPU oracle, bit for bit: access units, MbInfo, quadrant vectors, me_cost,
pre-filter and final planes (and the levels the entropy coder reads, through test_gpu_parity's _compare_all).

128x96 is the smallest picture with macroblocks on both window-load paths.  1 IDR + 4 P pictures; a lockstep batch of 4 GOPs.
Every content is built so that a particular exit of section 1 is taken (thresholds of QP 26: a luma block sum of 44, a chroma DC
Hadamard output of 87):
  static      synth's s2: the zero-vector test hits
  pan         S1 (pan + noise): the zero-vector test is turned down by the luma block sums; the test at the rounded previous vector
              sees hits, luma block sums, chroma DC and transform rejections side by side
  scroll      a whole-sample pan: the previous-vector test hits nearly everywhere
  luma_ac     every P picture is the oracle's own reconstruction of the picture before it plus a luma pattern (+a +a -a -a along
              every row of every 4x4 block, 24 a >= thr_inter[2]): all block sums are zero, the transform turns the macroblock down
  luma_edge   the reconstruction plus flat luma offsets that give every 4x4 block a residual sum of exactly thr_inter[0] - 1 in the
              even macroblocks (they settle) and exactly thr_inter[0] in the odd ones (the block sums turn them down)
  chroma_dc   luma equal to the reconstruction; a Cb offset whose 8x8 sum - the first 2x2 Hadamard output - is thr_dc_inter - 1 in
              the even macroblocks (they settle) and thr_dc_inter in the odd ones (the chroma DC turns them down)
  chroma_ac   luma equal, the zero-sum pattern in both chroma planes: luma and chroma DC pass, the transform turns it down
  pan10/pan51 `pan` where the thresholds are smallest and largest
Each with the seeded and the exhaustive search, frame by frame, as the lockstep batch and as one stream of the hub (IND = true).
The first test needs no GPU: a numpy restatement of the block sums and of the chroma DC on the oracle's source and reference
planes, beside the oracle's own settled / searched decision, shows that every content reaches its class and that no macroblock
the restated checks turn down is one the oracle settled.  It also asserts that on these contents the luma SAD shortcut (P.sad_nz) never
turns down a test that the block sums and the chroma DC let through (`sad_only` = 0): what k_me.h says of it."""
import functools
import numpy as np
import pytest
import stream_matrix as sm
from media_amd import synth
from oracle_lib import OracleEncoder

W, H, GOP, G = 128, 96, 5, 4      # 1 IDR + 4 P pictures per GOP; 4 GOPs in a lockstep batch
MBW, MBH = W // 16, H // 16
KINDS = ("static", "pan", "scroll", "luma_ac", "luma_edge", "chroma_dc", "chroma_ac", "pan10", "pan51")
QP = {k: 26 for k in KINDS}
QP.update(pan10=10, pan51=51)
SYNTH = {"static": "s2", "pan": "s1", "scroll": "scroll", "pan10": "s1", "pan51": "s1"}
SEARCH = pytest.mark.parametrize("search", [1, 0], ids=["seeded", "exhaustive"])

# quantiser constants (8.5.9, the encoder's usual multiplier table), position classes even/even, odd/odd, mixed; QPc of QPy (table 8-15)
MF = ((13107, 5243, 8066), (11916, 4660, 7490), (10082, 4194, 6554), (9362, 3647, 5825), (8192, 3355, 5243), (7282, 2893, 4559))
CHROMA_QP = tuple(range(30)) + (29, 30, 31, 32, 32, 33, 34, 34, 35, 35, 36, 36, 37, 37, 37, 38, 38, 38, 39, 39, 39, 39)


def thr_inter(qp, c):
    """smallest |coefficient| of position class c whose inter-rounded level is non-zero: (|w| * mf + f) >> qbits != 0"""
    qbits = 15 + qp // 6
    return ((1 << qbits) - (1 << qbits) // 6 + MF[qp % 6][c] - 1) // MF[qp % 6][c]


def thr_dc_inter(qpc):
    """the same for an output of the chroma DC's 2x2 Hadamard: (|f| * mf + 2 f_inter) >> (qbits + 1) != 0"""
    qbits = 15 + qpc // 6
    return ((1 << (qbits + 1)) - 2 * ((1 << qbits) // 6) + MF[qpc % 6][0] - 1) // MF[qpc % 6][0]


def sad_nz(qp):
    """the luma SAD from which a macroblock cannot quantise to nothing (host_framing.h fill_qp): the exact shortcut that the
    kernel keeps behind the block sums and the chroma DC"""
    t0, t1, t2 = (float(thr_inter(qp, c)) for c in range(3))
    return int(np.ceil(64.0 * np.sqrt(4 * t0 * t0 / 16.0 + 4 * t1 * t1 / 100.0 + 8 * t2 * t2 / 40.0))) + 1


def _spread(total, n):
    """n non-negative offsets that differ by one at most and add up to total"""
    return np.array([total // n + (1 if i < total % n else 0) for i in range(n)], np.int32)


def _pattern(kind, qp):
    """what a P picture of a reconstruction-based content adds to the reconstruction: (luma, Cb, Cr) as int32 planes"""
    y, u, v = np.zeros((H, W), np.int32), np.zeros((H // 2, W // 2), np.int32), np.zeros((H // 2, W // 2), np.int32)
    qpc = CHROMA_QP[qp]
    ac = np.tile(np.array([1, 1, -1, -1], np.int32), W // 4)
    if kind == "luma_ac":
        y[:] = (thr_inter(qp, 2) // 24 + 1) * ac
    elif kind == "chroma_ac":
        u[:] = v[:] = (thr_inter(qpc, 2) // 24 + 1) * ac[: W // 2]
    else:
        for my in range(MBH):
            for mx in range(MBW):
                odd = (my * MBW + mx) & 1
                if kind == "luma_edge":
                    blk = _spread(thr_inter(qp, 0) - 1 + odd, 16).reshape(4, 4)
                    y[16 * my: 16 * my + 16, 16 * mx: 16 * mx + 16] = np.tile(blk, (4, 4))
                else:   # chroma_dc
                    u[8 * my: 8 * my + 8, 8 * mx: 8 * mx + 8] = _spread(thr_dc_inter(qpc) - 1 + odd, 64).reshape(8, 8)
    return y, u, v


# ---------------------------------------------------------------- the restated checks

def _pred(ref, x0, y0, n, vx, vy, chroma):
    """n x n prediction samples at (x0, y0) + vector (vx, vy): luma whole samples (vx, vy: multiples of 4 quarter samples), chroma
    the 1/8-sample bilinear of 8.4.2.2.2; reference samples clamped at the picture edge"""
    h, w = ref.shape
    sh, fm = (3, 7) if chroma else (2, 3)
    fx, fy = vx & fm, vy & fm
    xs, ys = x0 + (vx >> sh) + np.arange(n + 1), y0 + (vy >> sh) + np.arange(n + 1)
    t = ref[np.clip(ys, 0, h - 1)][:, np.clip(xs, 0, w - 1)].astype(np.int32)
    a, b, c, d = t[:n, :n], t[:n, 1:], t[1:, :n], t[1:, 1:]
    if not chroma:
        assert fx == 0 and fy == 0
        return a
    return ((8 - fx) * (8 - fy) * a + fx * (8 - fy) * b + (8 - fx) * fy * c + fx * fy * d + 32) >> 6


def _gate(src, ref, mx, my, vx, vy, qp):
    """the cheap checks of one test, in the kernel's order: "sums" some luma 4x4 block's |residual sum| >= thr_inter[0],
    "cdc" an output of a chroma plane's 2x2 Hadamard of the block sums >= thr_dc_inter, else "pass" - or "pass+sad" where the
    luma SAD shortcut would still have turned the macroblock down"""
    y = d = src[0][16 * my: 16 * my + 16, 16 * mx: 16 * mx + 16].astype(np.int32) - _pred(ref[0], 16 * mx, 16 * my, 16, vx, vy, False)
    if np.abs(d.reshape(4, 4, 4, 4).sum(axis=(1, 3))).max() >= thr_inter(qp, 0):
        return "sums"
    for p in (1, 2):
        d = src[p][8 * my: 8 * my + 8, 8 * mx: 8 * mx + 8].astype(np.int32) - _pred(ref[p], 8 * mx, 8 * my, 8, vx, vy, True)
        b = d.reshape(2, 4, 2, 4).sum(axis=(1, 3))
        f = (b[0, 0] + b[0, 1] + b[1, 0] + b[1, 1], b[0, 0] - b[0, 1] + b[1, 0] - b[1, 1],
             b[0, 0] + b[0, 1] - b[1, 0] - b[1, 1], b[0, 0] - b[0, 1] - b[1, 0] + b[1, 1])
        if max(abs(int(x)) for x in f) >= thr_dc_inter(CHROMA_QP[qp]):
            return "cdc"
    return "pass+sad" if np.abs(y).sum() >= sad_nz(qp) else "pass"


CLASSES = ("t1_hit", "t1_sums", "t1_cdc", "t1_transform", "t2_tried", "t2_hit", "t2_sums", "t2_cdc", "t2_transform", "sad_only")


def _classify(src, ref, prev_mb, mb, decision, qp, tally):
    """one P picture: which exit of section 1 every macroblock takes.  src / ref: (Y, Cb, Cr) planes; prev_mb: MbInfo before the
    picture (its vectors seed the second test), mb / decision: the oracle's result.  Returns what contradicts the restated checks."""
    bad = []
    for i in range(MBW * MBH):
        my, mx = divmod(i, MBW)
        settled = decision[i] == OracleEncoder.P_SETTLED
        mv = (int(mb["mvx"][i]), int(mb["mvy"][i]))
        g1 = _gate(src, ref, mx, my, 0, 0, qp)
        if g1 == "pass+sad":
            g1, tally["sad_only"] = "pass", tally["sad_only"] + 1
        if settled and mv == (0, 0):
            tally["t1_hit"] += 1
            if g1 != "pass":
                bad.append("macroblock %d settled at the zero vector, restated check: %s" % (i, g1))
            continue
        tally["t1_" + ("transform" if g1 == "pass" else g1)] += 1
        rv = (((int(prev_mb["mvx"][i]) + 2) >> 2) * 4, ((int(prev_mb["mvy"][i]) + 2) >> 2) * 4)
        if rv == (0, 0):
            if settled:
                bad.append("macroblock %d settled at %s without a previous vector" % (i, mv))
            continue
        tally["t2_tried"] += 1
        g2 = _gate(src, ref, mx, my, rv[0], rv[1], qp)
        if g2 == "pass+sad":
            g2, tally["sad_only"] = "pass", tally["sad_only"] + 1
        if settled:
            tally["t2_hit"] += 1
            if g2 != "pass" or mv != rv:
                bad.append("macroblock %d settled at %s, rounded previous vector %s, restated check: %s" % (i, mv, rv, g2))
        else:
            tally["t2_" + ("transform" if g2 == "pass" else g2)] += 1
    return bad


def _planes(frame):
    f = np.asarray(frame, np.uint8)
    return f[: W * H].reshape(H, W), f[W * H: W * H * 5 // 4].reshape(H // 2, W // 2), f[W * H * 5 // 4:].reshape(H // 2, W // 2)


@functools.lru_cache(maxsize=None)
def reference(kind, search):
    """the oracle's G GOPs, computed once per (content, search mode): frames, access units, me_cost per picture, and for the first
    GOP the class counts and whatever contradicts the restated checks.  The reconstruction-based contents are built while the
    oracle runs (the GOPs are closed and start from the same picture, so the pictures of the first serve all four)."""
    qp = QP[kind]
    base = synth.sequence(SYNTH.get(kind, "s1"), W, H, GOP)
    orc = OracleEncoder(W, H, qp=qp, gop=GOP, search=search)
    frames, aus, costs, tally, bad = [], [], [], dict.fromkeys(CLASSES, 0), []
    for i in range(G * GOP):
        k = i % GOP
        ref = [orc.recon(p) for p in range(3)] if k else None
        prev_mb = orc.mbinfo().reshape(-1) if k else None
        if i >= GOP:
            f = frames[k]
        elif kind in SYNTH or k == 0:
            f = np.asarray(base[k], np.uint8)
        else:
            f = np.concatenate([np.clip(r.astype(np.int32) + a, 0, 255).astype(np.uint8).ravel() for r, a in zip(ref, _pattern(kind, qp))])
        au, idr = orc.encode(f)
        assert idr == (k == 0)
        frames.append(f)
        aus.append(au)
        costs.append(orc.me_cost())
        if k and i < GOP:
            bad += ["picture %d: %s" % (i, b) for b in _classify(_planes(f), ref, prev_mb, orc.mbinfo().reshape(-1), orc.p_decision(), qp, tally)]
    orc.close()
    return frames, aus, costs, tally, bad


# what every content is there for: classes that must not be empty
WANTED = {"static": ("t1_hit",), "pan": ("t1_sums", "t2_hit", "t2_sums", "t2_cdc"), "scroll": ("t2_hit",), "luma_ac": ("t1_transform",),
          "luma_edge": ("t1_hit", "t1_sums"), "chroma_dc": ("t1_hit", "t1_cdc"), "chroma_ac": ("t1_transform",),
          "pan10": ("t1_sums", "t2_tried"), "pan51": ("t1_hit",)}


@SEARCH
@pytest.mark.parametrize("kind", KINDS)
def test_content_reaches_its_class(kind, search):
    """no GPU: the restated block sums and chroma DC beside the oracle's own decision"""
    _, _, _, tally, bad = reference(kind, search)
    print("%s: %s" % (kind, tally))
    assert not bad, bad[:5]
    for c in WANTED[kind]:
        assert tally[c] > 0, (kind, c, tally)
    assert tally["sad_only"] == 0, tally   # the SAD shortcut decides nothing that the cheaper checks in front of it do not
    if kind in ("luma_edge", "chroma_dc"):   # the two kinds sit in different macroblocks: every picture has half and half
        assert tally["t1_hit"] == tally["t1_sums" if kind == "luma_edge" else "t1_cdc"] == (GOP - 1) * MBW * MBH // 2, tally
    if kind == "scroll":
        assert 2 * tally["t2_hit"] > tally["t2_tried"], tally


def _compare_picture(enc, orc, cost, want_cost, tag):
    from media_amd import capi
    from test_gpu_parity import _compare_all
    _compare_all(enc, orc, tag)
    assert int(cost) == int(want_cost), "%s: me_cost %d, the oracle's %d" % (tag, int(cost), int(want_cost))
    for p in range(3):
        assert np.array_equal(enc.debug_read(capi.DBG_RECON_Y + p), orc.recon(p)), "%s: final plane %d" % (tag, p)


@pytest.mark.gpu
@SEARCH
@pytest.mark.parametrize("kind", KINDS)
def test_frame_by_frame_every_stage(kind, search):
    from media_amd import capi
    frames, aus, costs, _, _ = reference(kind, search)
    enc = capi.Encoder(W, H, qp=QP[kind], gop=GOP, search=search)
    enc.keep_pre(True)
    orc = OracleEncoder(W, H, qp=QP[kind], gop=GOP, search=search)
    for i in range(GOP + 1):          # one GOP and the IDR picture after it
        au, _ = enc.encode(frames[i])
        want, idr = orc.encode(frames[i])
        assert want == aus[i]
        assert au == want, "%s picture %d: access unit" % (kind, i)
        _compare_picture(enc, orc, 0 if idr else enc.me_cost()[0], 0 if idr else costs[i], "%s picture %d" % (kind, i))
    enc.close()
    orc.close()


@pytest.mark.gpu
@SEARCH
@pytest.mark.parametrize("kind", KINDS)
def test_lockstep_batch_of_four(kind, search):
    import torch
    from media_amd import capi
    frames, aus, costs, _, _ = reference(kind, search)
    fbytes = W * H * 3 // 2
    dev = torch.from_numpy(np.stack(frames)).cuda()
    enc = capi.Encoder(W, H, qp=QP[kind], gop=GOP, batch=G, search=search)
    cap = 2 * GOP * fbytes
    out, sizes, gb = np.zeros(G * cap, np.uint8), np.zeros(G * GOP, np.uint32), np.zeros(G, np.uint64)
    enc.encode_gops_device(dev.data_ptr(), fbytes, GOP * fbytes, GOP, out, cap, sizes, gb)
    for g in range(G):
        assert out[g * cap: g * cap + int(gb[g])].tobytes() == b"".join(aus[g * GOP:(g + 1) * GOP]), "%s GOP %d" % (kind, g)
        assert [int(x) for x in sizes[g * GOP:(g + 1) * GOP]] == [len(a) for a in aus[g * GOP:(g + 1) * GOP]]
    assert [int(c) for c in enc.me_cost()] == [costs[g * GOP + GOP - 1] for g in range(G)], "%s: me_cost of the last step" % kind
    enc.close()


@pytest.mark.gpu
@SEARCH
@pytest.mark.parametrize("kind", KINDS)
def test_one_stream_of_the_hub(kind, search):
    """the IND = true instantiation: one stream of the hub, every stage"""
    from media_amd import capi
    s = sm.spec("s1", W, H, 66, GOP, (QP[kind],) * GOP, search=search)
    frames, aus, costs, _, _ = reference(kind, search)
    stream = capi.Stream(s.w, s.h, qp=s.qps[0], gop=s.gop, profile_idc=s.prof, search=s.search)
    stream.keep_pre(True)
    orc = sm.oracle_for(s)
    for i in range(GOP):
        au = stream.encode(frames[i])[0]
        assert orc.encode(frames[i])[0] == aus[i]
        assert au == aus[i], "%s picture %d: access unit" % (kind, i)
        _compare_picture(stream, orc, stream.me_cost() if i else 0, costs[i] if i else 0, "%s hub picture %d" % (kind, i))
    stream.close()
    orc.close()
