"""The multi-reference motion search (config.refs = 2 / 3) where the OLDER pictures win: content, cases and per-picture
facts that tests/test_ref_mix_oracle.py (CPU: what the list holds) and tests/test_gpu_ref_mix.py (GPU) share.

Panning content takes ref_idx_l0 = 0 almost everywhere: the newest picture is the nearest.  frame_ref_mix gives every macroblock
position a PERIOD p in 1 .. periods.  A region of period p shows variant(base picture t // p, t % p), and the variants are
mutually unlike pictures made from the base picture: what the region shows in picture t resembles what it showed in picture
t - p (ref_idx_l0 = p - 1), moved on by one step of the base content's motion, and nothing in between.  In the left half of the
picture the period is drawn per macroblock (neighbours differ: vector prediction, P_Skip inference and the loop filter's
strengths see neighbours of another reference index), in the right half per 2x2 macroblocks (some neighbourhoods agree).

Everything is deterministic; what is computed is computed once per process, shared and never changed."""
import functools
from collections import namedtuple
import numpy as np
from large_batch import StagesOf     # what test_gpu_parity._compare_all reads of an oracle, kept from the moment it had coded the picture
from media_amd import synth

BASES = ("s1", "split", "still", "fast", "scroll")
INTER = (1, 2, 5, 6, 7)                                  # P_L0_16x16, P_Skip, 16x8, 8x16, P_8x8 (MbInfo.type)
SHAPES = ("16x16", "skip", "16x8", "8x16", "8x8")        # the order of every count below


def base_frame(base, w, h, i):
    """picture i of the base content.  still: one noise-free picture (a region of period p repeats an older picture exactly: zero
    vector, nothing to code, the reference index is all that tells it from its neighbour); fast: seven luma rows per step"""
    if base == "s1":
        return synth.frame_s1(w, h, i)
    if base == "split":
        return synth.frame_split(w, h, i)
    if base == "still":
        return synth.frame_s1(w, h, 0, noise=0)
    if base == "fast":
        return synth.frame_s1(w, h, i, noise=2, motion=(2, 7))
    if base == "scroll":
        return synth.frame_scroll(w, h, i)
    raise KeyError(base)


def _planes(f, w, h):
    ysz, csz = w * h, w * h // 4
    return f[:ysz].reshape(h, w), f[ysz:ysz + csz].reshape(h // 2, w // 2), f[ysz + csz:].reshape(h // 2, w // 2)


def variant(f, w, h, v):
    """(Y, U, V) of variant v of the tight I420 picture f.  0: unchanged; 1: Y inverted and rotated by 180 degrees, U rotated, V
    inverted and rotated (synth.frame_cut's twin); 2: Y mirrored left-right, U and V mirrored and swapped"""
    y, u, c = _planes(f, w, h)
    if v == 0:
        return y, u, c
    if v == 1:
        return 255 - y[::-1, ::-1], u[::-1, ::-1], 255 - c[::-1, ::-1]
    if v == 2:
        return y[:, ::-1], c[:, ::-1], u[:, ::-1]
    raise ValueError(v)


@functools.lru_cache(maxsize=None)
def period_map(w, h, periods, seed):
    """the period of every macroblock position, (rows, columns) of 1 .. periods"""
    mbw, mbh = (w + 15) // 16, (h + 15) // 16
    r = synth._hash_u32(seed, mbw * mbh).reshape(mbh, mbw)
    my, mx = np.mgrid[0:mbh, 0:mbw]
    coarse = r[my & ~1, mx & ~1]                         # the draw of the 2x2 group's first macroblock
    out = (1 + np.where(mx < mbw // 2, r, coarse) % np.uint32(periods)).astype(np.int32)
    out.setflags(write=False)
    return out


def frame_ref_mix(base, w, h, t, periods, seed):
    """tight I420 picture t: luma masks of 16 samples, chroma masks of 8"""
    pm = period_map(w, h, periods, seed)
    masks = [np.kron(pm, np.ones((b, b), np.int32))[:hh, :ww] for b, hh, ww in ((16, h, w), (8, h // 2, w // 2), (8, h // 2, w // 2))]
    out = [np.zeros((h, w), np.uint8), np.zeros((h // 2, w // 2), np.uint8), np.zeros((h // 2, w // 2), np.uint8)]
    for p in range(1, periods + 1):
        planes = variant(base_frame(base, w, h, t // p), w, h, t % p)
        for k in range(3):
            out[k] = np.where(masks[k] == p, planes[k], out[k])
    return np.concatenate([np.ascontiguousarray(a).ravel() for a in out])


# ---------------------------------------------------------------- the cases

Case = namedtuple("Case", "name base w h prof refs slices qp gop pictures seed start nv12")


def case(name, base, w, h, prof, refs, slices, qp, gop, pictures, seed=1, start=0, nv12=False):
    return Case(name, base, w, h, prof, refs, slices, qp, gop, pictures, seed, start, nv12)


CASES = (
    case("s1_208x160", "s1", 208, 160, 66, 3, 0, 27, 8, 11),                 # every reference index under 16x16; intra macroblocks in P pictures
    case("split_208x160", "split", 208, 160, 77, 3, 0, 24, 8, 11),           # every partition shape under every reference index
    case("split_96x80_high", "split", 96, 80, 100, 3, 2, 26, 7, 9),          # the same with the 8x8 transform and two slices
    case("split_48x48", "split", 48, 48, 66, 3, 0, 26, 8, 10),               # 3 x 3 macroblocks: every macroblock lies at an edge
    case("still_96x80", "still", 96, 80, 66, 3, 0, 30, 8, 10),               # P_Skip beside older references; strength 1 from the reference alone
    case("still_96x80_high", "still", 96, 80, 100, 3, 2, 30, 8, 10),
    case("fast_96x128", "fast", 96, 128, 77, 3, 4, 26, 8, 10),               # vectors of the older references cross band boundaries
    case("two_refs_s1_96x80", "s1", 96, 80, 100, 2, 0, 30, 6, 8),            # te(v) of one bit
    case("scroll_112x96", "scroll", 112, 96, 66, 3, 3, 22, 9, 11),
    case("long_ring", "split", 48, 48, 66, 3, 0, 26, 40, 42),                # the ring goes round a dozen times, frame_num runs on
    case("two_refs_split", "split", 96, 80, 100, 2, 0, 26, 7, 9),            # te(v) of one bit together with partitions
    case("nv12", "split", 96, 80, 100, 3, 2, 26, 7, 9, nv12=True),           # split_96x80_high handed over as NV12
)
BY_NAME = {c.name: c for c in CASES}
SEARCHES = (0, 1)     # exhaustive, seeded by the previous picture's vector
STILL = ("still_96x80", "still_96x80_high")
THREE = tuple(c for c in CASES if c.refs == 3)
TWO = tuple(c for c in CASES if c.refs == 2)
# the window restart of s1_208x160: (picture, "idr": force an IDR picture | a QP to set) before that picture is coded
WINDOW_EVENTS = ((4, "idr"), (6, 20), (8, 40))


@functools.lru_cache(maxsize=None)
def frames(c):
    out = tuple(frame_ref_mix(c.base, c.w, c.h, c.start + i, c.refs, c.seed) for i in range(c.pictures))
    for f in out:
        f.setflags(write=False)
    return out


def to_nv12(f, w, h):
    y, u, v = f[: w * h], f[w * h: w * h * 5 // 4], f[w * h * 5 // 4:]
    return np.concatenate([y, np.stack([u, v], axis=1).ravel()])


def slice_rows(c):
    """macroblock rows per slice band (the rule of include/mi355x_h264.h, `slices`); 0: one slice"""
    mbh = (c.h + 15) // 16
    if c.slices < 2:
        return 0
    nb = min(c.slices, max(1, mbh // 2))
    return -(-mbh // nb)


def oracle_for(c, search):
    from oracle_lib import OracleEncoder
    return OracleEncoder(c.w, c.h, qp=c.qp, gop=c.gop, profile_idc=c.prof, slices=c.slices, refs=c.refs, search=search)


Pic = namedtuple("Pic", "au idr stages facts")


def picture_facts(c, idr, since_idr, mb, mvq, dec):
    """what one picture holds, from the writer's side information (mbinfo(): type, ref_idx_l0 in chroma_mode, cbp; mvq()) and from
    the independent decoder (macroblock kinds, RefPicList0).  shapes[s][r]: macroblocks of SHAPES[s] with ref_idx_l0 = r"""
    from oracle_lib import OracleDecoder
    mbw, mbh = (c.w + 15) // 16, (c.h + 15) // 16
    t, ref, cbp = (mb[k].astype(np.int32).reshape(mbh, mbw) for k in ("type", "chroma_mode", "cbp"))
    inter = np.isin(t, INTER)
    f = {"idr": bool(idr), "since_idr": since_idr, "shapes": np.zeros((5, 3), np.int64), "diff_left": 0, "diff_top": 0, "diff_left_cbp0": 0,
         "diff_top_cbp0": 0, "skip_beside_older": 0, "intra_in_p": 0, "available": 0, "across_slice_edge": 0, "inter": inter, "ref": ref}
    if idr:
        return f
    for s, typ in enumerate(INTER):
        for r in range(3):
            f["shapes"][s, r] = int(((t == typ) & (ref == r)).sum())
    for name, a, b in (("left", (slice(None), slice(1, None)), (slice(None), slice(0, -1))), ("top", (slice(1, None), slice(None)), (slice(0, -1), slice(None)))):
        d = inter[a] & inter[b] & (ref[a] != ref[b])
        f["diff_" + name] = int(d.sum())
        f["diff_%s_cbp0" % name] = int((d & (cbp[a] == 0) & (cbp[b] == 0)).sum())
    older = inter & (ref > 0)
    beside = np.zeros_like(older)
    beside[:, 1:] |= older[:, :-1]
    beside[1:, :] |= older[:-1, :]
    f["skip_beside_older"] = int(((t == 2) & beside).sum())
    kinds = dec.mb_kinds()
    f["intra_in_p"] = int(np.isin(kinds, (OracleDecoder.KIND_I4, OracleDecoder.KIND_I16, OracleDecoder.KIND_IPCM)).sum())
    assert f["intra_in_p"] == int(np.isin(t, (0, 3, 4)).sum())
    ages = dec.ref_ages()
    f["available"] = sum(a >= 0 for a in ages)
    f["ref_ages"] = ages
    rows = slice_rows(c)
    if rows:
        v = mvq.reshape(mbh, mbw, 4, 2).astype(np.int32)
        for edge in range(rows, mbh, rows):     # the first macroblock row of the slice below
            # above the edge: a quadrant whose lower end, moved by its vector, lies below the edge; below it: the upper end above
            down = ((v[edge - 1, :, :, 1] + 32 * (np.arange(4) >> 1)[None, :] + 32) > 64).any(axis=1)
            up = ((v[edge, :, :, 1] + 32 * (np.arange(4) >> 1)[None, :]) < 0).any(axis=1)
            f["across_slice_edge"] += int((down & older[edge - 1] & (t[edge - 1] != 2)).sum() + (up & older[edge] & (t[edge] != 2)).sum())
    return f


def check_decoded(c, tag, orc_mb, orc_mvq, recon, dec):
    """the independent decoder against the writer's side information: planes, the reference index of every 4x4 block of every
    inter macroblock (the writer's chroma_mode), the vectors (mvq(); P_Skip's is inferred and not recorded)"""
    for p in range(3):
        assert np.array_equal(dec.plane(p), recon[p]), "%s: the decoder's plane %d is not the encoder's reconstruction" % (tag, p)
    for m in np.nonzero(np.isin(orc_mb["type"], INTER))[0]:
        for b in range(16):
            x, y, r = dec.mb_mv(int(m), b)
            assert r == int(orc_mb["chroma_mode"][m]), "%s macroblock %d block %d: decoded ref_idx_l0 %d, written %d" % (tag, m, b, r, int(orc_mb["chroma_mode"][m]))
            if orc_mb["type"][m] != 2:
                q = (b >> 3) * 2 + ((b >> 1) & 1)
                assert (x, y) == (int(orc_mvq[m, 2 * q]), int(orc_mvq[m, 2 * q + 1])), "%s macroblock %d block %d: vector" % (tag, m, b)


@functools.lru_cache(maxsize=None)
def expected(c, search, events=()):
    """the oracle's stream of the case: a tuple of Pic, every access unit decoded by the independent decoder and held against the
    writer's side information.  events: ((picture, "idr" | qp), ..) - force an IDR picture / set the QP before that picture"""
    from oracle_lib import OracleDecoder
    orc, dec = oracle_for(c, search), OracleDecoder()
    out, since = [], 0
    for i, f in enumerate(frames(c)):
        force = False
        for at, what in events:
            if at == i and what == "idr":
                force = True
            elif at == i:
                orc.set_qp(what)
        au, idr = orc.encode(f, force_idr=force)
        since = 0 if idr else since + 1
        tag = "%s search %d picture %d" % (c.name, search, i)
        assert dec.decode(au) == 1, tag
        st = StagesOf(orc)
        check_decoded(c, tag, st.mbinfo(), st.mvq(), st.s.recon, dec)
        out.append(Pic(au, idr, st, picture_facts(c, idr, since, st.mbinfo(), st.mvq(), dec)))
    orc.close()
    dec.close()
    return tuple(out)


def totals(pics):
    """the facts of a run summed over its P pictures"""
    keys = ("diff_left", "diff_top", "diff_left_cbp0", "diff_top_cbp0", "skip_beside_older", "intra_in_p", "across_slice_edge")
    out = {k: sum(p.facts[k] for p in pics) for k in keys}
    out["shapes"] = sum(p.facts["shapes"] for p in pics)
    return out


def me_launches(refs, idrs):
    """K_ME launches of a run whose pictures are IDR where idrs[i]: one per reference picture a P picture may use, min(refs,
    pictures since the IDR) (tests/large_batch.py, expected_stats)"""
    n = since = 0
    for idr in idrs:
        since = 0 if idr else since + 1
        n += min(max(refs, 1), since)
    return n


# ---------------------------------------------------------------- lockstep batches (capi.Encoder(batch = G), encode_gops_device)

Batch = namedtuple("Batch", "name case G")
# items are the case's content at a seed and a start of their own: in one launch the items' macroblocks take different references
BATCHES = (Batch("eight_48x48", BY_NAME["split_48x48"], 8), Batch("three_96x80", BY_NAME["split_96x80_high"], 3))


def batch_item(b, g):
    """item g of the batch: one closed GOP"""
    return b.case._replace(name="%s_item%d" % (b.name, g), seed=b.case.seed + 7 * g, start=b.case.start + 3 * g + (g & 1), pictures=b.case.gop)


@functools.lru_cache(maxsize=None)
def batch_expected(b, search):
    """the oracle's serial stream of the batch: one encoder codes the closed GOP of item 0, item 1, .. (idr_pic_id runs on, as the
    engine's does).  Returns ([per item: tuple of Pic], the stages of item 0's last picture); every access unit decoded and checked"""
    from oracle_lib import OracleDecoder
    orc, dec = oracle_for(b.case, search), OracleDecoder()
    items, stages0 = [], None
    for g in range(b.G):
        c, gop = batch_item(b, g), []
        for i, f in enumerate(frames(c)):
            au, idr = orc.encode(f)
            assert idr == (i == 0), "closed GOPs"
            tag = "%s search %d picture %d" % (c.name, search, i)
            assert dec.decode(au) == 1, tag
            st = StagesOf(orc)
            check_decoded(c, tag, st.mbinfo(), st.mvq(), st.s.recon, dec)
            gop.append(Pic(au, idr, st, picture_facts(c, idr, i, st.mbinfo(), st.mvq(), dec)))
        if g == 0:
            stages0 = gop[-1].stages
        items.append(tuple(gop))
    orc.close()
    dec.close()
    return tuple(items), stages0
