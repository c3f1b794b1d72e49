"""The decoder's loop filter on every threshold index, strength and branch: the streams, the cells a stream list has to reach, and
the floors.  Shared by tests/test_deblock_cells_oracle.py (CPU: the list holds what it claims, from the oracle decoder's own
account h264o_dec_dbf) and tests/test_gpu_deblock_cells.py (GPU).  Nothing of the decoder under test is used here.

Two kinds of stream.

"enc": access units of the oracle ENCODER on smooth content, their slice headers rewritten (slice_header.rehead) to another
SliceQP_Y, other filter offsets and another idc.  Still a conforming stream; prediction plus a small residual stays smooth, so the
filter fires - at the indexA / indexB the new header asks for.  Random residual never does that: a noisy line fails
|p0 - q0| < alpha.  Every picture is coded at or ABOVE the QP it is re-headed to: re-headed upward, the residual grows past the
16-bit range of 8.5 and the picture is too noisy to filter.  coded = target + 4 or + 8, with two exceptions of + 0: a target
above 47 is clamped to a coded QP of 51 (so the four pictures aimed at indexA 51 with oa = ob = 0 carry the encoder's own header,
not a rewritten one), and the IDR pictures of the `kinks` cases, whose samples have to stay at 0 and 255 (a lower QP under the
same levels scales the whole residual, DC included, and pulls every sample towards the prediction).  A picture with an I_PCM
macroblock keeps its header (pcm_alignment_zero_bit depends on the header's length).

"rand": h264o_enc_random_picture, for what the encoder never writes: mb_qp_delta across left edges, I_PCM neighbours, both
chroma offsets, slices cut anywhere, idc 0 / 1 / 2.

Everything is deterministic and computed once per process."""
import functools
from collections import namedtuple

import numpy as np

import adversarial
import range_ends
from media_amd import synth
from oracle_lib import OracleEncoder, OracleDecoder, Dbf
from slice_header import rehead
from temporal import nal_units, annexb

FLOOR = 8            # lines with a changed sample per (kind, bS, indexA >= 16), over the whole list
PICTURES = 12

# ---------------------------------------------------------------- the schedule
# One row per picture: SliceQP_Y the header is rewritten to, the QP the picture is coded at, slice_alpha_c0_offset_div2,
# slice_beta_offset_div2, idc, whether the picture is an IDR picture, and `step`: slice k of the picture gets SliceQP_Y qp - k * step
# (idc 0: the top edges between slices then have qPp != qPq, odd sums for an odd step).
Row = namedtuple("Row", "qp coded oa ob idc idr step")
QPC = list(range(30)) + [29, 30, 31, 32, 32, 33, 34, 34, 35, 35, 36, 36, 37, 37, 37, 38, 38, 38, 39, 39, 39, 39]   # Table 8-15


def _row(qp, oa, ob, idr, bump, idc=0, step=0):
    return Row(qp, min(51, max(10, qp + bump)), oa, ob, idc, idr, step)


def _main_rows():
    """luma indexA t = qp + 2 * oa for every t of 16 .. 51 under three offsets, two pictures each: IDR P, P P, P P"""
    rows = []
    for t in range(16, 52):
        k = 1 + t % 6
        for j, oa in enumerate((0, k if t - 2 * k >= 4 else -k, -k if t + 2 * k <= 51 else k - 7 if t - 2 * (k - 7) <= 51 else 0)):
            qp = t - 2 * oa
            assert 0 <= qp <= 51 and -6 <= oa <= 6, (t, oa)
            ob = max(-6, min(6, (0, (t * 5 + 1) % 7 - 3, -oa)[j]))
            bump = (4, 8)[(t + j) % 2]   # (never 0: a picture whose header changes offsets alone may decode to the same samples)
            rows += [_row(qp, oa, ob, j == 0, bump, step=(0, 1, 3)[t % 3]), _row(qp, oa, ob, False, bump, idc=2 if t % 4 == 1 and j == 1 else 0)]
    return tuple(rows)


def _chroma_rows():
    """chroma indexA / indexB 40 .. 51 = QPc + 2 * o (QPc <= 39: only a positive offset reaches them), an IDR picture and three P
    pictures each.  P pictures at these QPs on still content are all P_Skip with bS 0: the cases that run these rows use content
    that keeps a residual and splits vectors at any QP"""
    rows = []
    for c in range(40, 52):
        done = 0
        for o in range(6, 0, -1):
            qs = [q for q in range(30, 52) if QPC[q] + 2 * o == c]
            if qs and done < 2:
                rows += [_row(qs[0], o, o, True, 4), _row(qs[0], o, (c % 5) - 2, False, 8), _row(min(qs[-1], 49), o, o, False, 8), _row(min(qs[-1], 49), o, 0, False, 4)]
                done += 1
    return tuple(rows)


# indexA >= 16 with indexB < 16 and the reverse; both below 16 (lines are evaluated, none is filtered)
LOW_ROWS = (_row(20, 0, -6, True, 4), _row(20, 0, -6, False, 4), _row(20, -6, 0, True, 4), _row(20, -6, 0, False, 8), _row(12, 0, 0, True, 4),
            _row(12, 1, -1, False, 8), _row(4, 2, 2, True, 8), _row(0, 3, 0, False, 8), _row(15, 0, 0, True, 4), _row(15, 0, 0, False, 8),
            _row(9, 3, 3, False, 4), _row(13, 1, 1, False, 4))
# indexB 16, 17, 21 and 26 under a second offset
EXTRA_ROWS = (_row(22, 0, -3, True, 4), _row(13, 2, 2, False, 8), _row(27, 0, -3, False, 4), _row(20, 1, 3, True, 8), _row(30, -2, 2, False, 4), _row(36, 2, -2, False, 8))
MAIN_ROWS, CHROMA_ROWS = _main_rows(), _chroma_rows()


def _kink_rows(idr_qps, p_qp, n_p):
    """IDR pictures at their coded QP under offsets + 6 / + 6, each with n_p P pictures behind it (no residual: their QP is free)"""
    rows = []
    for q in idr_qps:
        rows += [_row(q, 6, 6, True, 0)] + [_row(p_qp[len(rows) // (n_p + 1) % len(p_qp)] - 4, (6, 4, 5)[k % 3], 6, False, 4) for k in range(n_p)]
    return tuple(rows)


# Clip1 on p0 + delta and q0 - delta at 0 and at 255, per bS (content `kinks` / `kinks8`, frame_kinks below)
KINK_ROWS = {"a24": _kink_rows((16,), (24,), 11), "a30": _kink_rows((16,), (30,), 11),
             "b": _kink_rows((18, 28, 14), (26, 32, 22), 3), "c": _kink_rows((20, 24, 16), (26, 32, 22), 3)}
SCHEDULE = MAIN_ROWS + CHROMA_ROWS + LOW_ROWS + EXTRA_ROWS + tuple(r for k in sorted(KINK_ROWS) for r in KINK_ROWS[k])

# ---------------------------------------------------------------- the cases
# kind "enc": rows = the schedule rows of its pictures;  kind "rand": features, and `rows` is the seed offset
Case = namedtuple("Case", "name kind w h prof slices refs content rows features")
# Baseline; Main with two slices on `cut` content; High, three references
CONFIGS = ((66, 0, 1, "split", 64, 48), (77, 2, 1, "cut", 96, 80), (100, 0, 3, "s1", 64, 48))
HARD_FROM = 42                                # P pictures coded at this QP and above are all P_Skip on the synth content
HARD = ("glyphs", "contrast", "bars")         # content that keeps a residual and distinct vectors at QP 51 (tests/adversarial.py)


def _chunks(rows, n=PICTURES):
    """n rows per stream; a last stream that would be short takes the rows in front of it as well"""
    return [tuple(rows[max(0, min(i, len(rows) - n)):i + n]) for i in range(0, len(rows), n)]


def _enc_cases():
    out = []
    for s, rows in enumerate(_chunks(MAIN_ROWS)):
        prof, slices, refs, content, w, h = CONFIGS[s % 3]
        if max(r.coded for r in rows) >= HARD_FROM:
            content = HARD[s % 3]
        out.append(Case("main_%02d_%d_%s" % (s, prof, content), "enc", w, h, prof, slices, refs, content, rows, 0))
    for s, rows in enumerate(_chunks(CHROMA_ROWS)):
        for content in HARD:
            prof, slices, refs, _, w, h = CONFIGS[(s + len(content)) % 3]
            out.append(Case("chroma_%02d_%d_%s" % (s, prof, content), "enc", w, h, prof, slices, refs, content, rows, 0))
    out.append(Case("low_66_split", "enc", 64, 48, 66, 0, 1, "split", LOW_ROWS, 0))
    out.append(Case("extra_100_contrast", "enc", 64, 48, 100, 0, 3, "contrast", EXTRA_ROWS, 0))
    # the saturating generators at middle indices: Clip1 on p0 + delta and q0 - delta
    for s, content in enumerate(("gradient", "bars", "checker", "glyphs", "contrast")):
        prof, slices, refs, _, w, h = CONFIGS[s % 3]
        out.append(Case("clip_%d_%s" % (prof, content), "enc", w, h, prof, slices, refs, content, tuple(MAIN_ROWS[(36 * s + 7 * i) % len(MAIN_ROWS)] for i in range(PICTURES)), 0))
    for name, prof, refs, content, rows in (("a30", 66, 1, "kinks", "a30"), ("a24", 100, 3, "kinks", "a24"), ("a30", 100, 3, "kinks", "a30"),
                                            ("b", 66, 1, "kinks8", "b"), ("b", 100, 3, "kinks8", "b"), ("c", 77, 1, "kinks8", "c"), ("c", 100, 3, "kinks8", "c")):
        out.append(Case("kinks_%s_%d" % (name, prof), "enc", 64, 48, prof, 0, refs, content, KINK_ROWS[rows], 0))
    # the smallest sizes: no macroblock edge at all, one row, one column
    for s, (w, h) in enumerate(((16, 16), (32, 16), (16, 48))):
        prof, _, refs, _, _, _ = CONFIGS[(2 * s) % 3]
        content = "contrast"
        out.append(Case("small_%dx%d_%d" % (w, h, prof), "enc", w, h, prof, 0, refs, content, tuple(MAIN_ROWS[(50 * s + 17 * i) % len(MAIN_ROWS)] for i in range(PICTURES)), 0))
    return out


BASE, RE = range_ends.BASE, range_ends.RE


def _rand_cases():
    out = []
    for s, (w, h, prof, slices, refs, feat) in enumerate((
            (16, 16, 66, 0, 1, BASE), (32, 16, 77, 0, 2, BASE | RE), (16, 48, 100, 0, 3, BASE), (64, 48, 66, 0, 2, BASE | RE),
            (64, 48, 100, 0, 3, BASE), (96, 80, 77, 2, 2, BASE | RE), (96, 80, 100, 3, 3, BASE))):
        out.append(Case("rand_%dx%d_%d%s" % (w, h, prof, "_ends" if feat & RE else ""), "rand", w, h, prof, slices, refs, None, s, feat))
    return out


CASES = _enc_cases() + _rand_cases()
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)

Picture = namedtuple("Picture", "au orig idr row reheaded pcm planes dbf stats kinds")


def frame_kinks(w, h, i, inner):
    """Content for the Clip1 cells.  p0 + delta < 0 needs p0 = q0 = 0 and delta < 0: with p1 = 0 that is q1 >= 5 (8-475), a kink ONE
    sample behind the edge; q0 - delta < 0 is the mirror image, the kink one sample in front.  So: rows of 0 with a bump of height
    s = 8, 11 or 14 that starts one sample behind every macroblock edge (left half of the picture) or ends one sample in front of
    it (right half); the first macroblock row as it is, the others as 255 - v; V inverted.  Macroblock columns belong in turn to
    two layers that move up / down by two luma samples per picture: whole-sample motion, so P pictures carry no residual and the
    macroblock edges between the layers get bS 1 (bS 2 where the encoder codes a residual all the same).  `inner`: the bumps of
    every second band of eight rows sit half a macroblock further on, at the inner edge 2 (bS 3 in intra macroblocks)."""
    def plane(w, h, mb, step, inv):
        x, y = np.arange(w)[None, :], np.arange(h)[:, None]
        yl = y + np.where((x // mb) % 2 == 0, step * i, -step * i)
        xm = (x + (mb // 2) * ((yl // 8) % 2)) % mb if inner else x % mb
        xm = np.where(x < w // 2, xm, mb - 1 - xm)
        s = 8 + 3 * ((yl // (16 if inner else 8)) % 3)
        v = np.where(yl % 8 < 5, np.select([xm == 0, xm == 1, xm == 2, xm == 3, xm == 4, xm == 5], [0, s, s + 2, s + 2, s, 4], 0), 0)
        return np.where((y < mb) ^ inv, v, 255 - v).astype(np.uint8).ravel()
    return np.concatenate([plane(w, h, 16, 2, False), plane(w // 2, h // 2, 8, 1, False), plane(w // 2, h // 2, 8, 1, True)])


def frame(content, w, h, i):
    if content in ("kinks", "kinks8"):
        return frame_kinks(w, h, i, content == "kinks8")
    if content == "cut":                         # two pictures of one content, two of the other, and back: a cut every second picture
        return synth.frame_cut(w, h, i % 4)
    if content in adversarial.GENERATORS:
        return adversarial.GENERATORS[content](w, h, i)
    return synth.sequence(content, w, h, 1, start=i)[0]


def reheaded_au(au, row):
    out = []
    k = 0
    for n in nal_units(au):
        if (n[0] & 31) in (1, 5):
            n = rehead(n, row.qp - k * row.step, row.idc, row.oa, row.ob)
            k += 1
        out.append(n)
    return annexb(out)


@functools.lru_cache(maxsize=None)
def stream(case):
    """the case's pictures: the access unit, the encoder's own one (enc cases), is_idr, the schedule row, whether the header was
    rewritten, whether it was left alone for an I_PCM macroblock, the oracle decoder's three coded planes, its filter account (Dbf), its statistics, its macroblock kinds"""
    enc = OracleEncoder(case.w, case.h, qp=30, gop=1000 if case.kind == "enc" else 5, profile_idc=case.prof, slices=case.slices, refs=case.refs)
    dec, plain = OracleDecoder(), OracleDecoder()
    out = []
    rows = case.rows if case.kind == "enc" else (None,) * PICTURES
    assert 6 <= len(rows) <= PICTURES
    for i, row in enumerate(rows):
        if case.kind == "enc":
            enc.set_qp(row.coded)
            orig, idr = enc.encode(frame(case.content, case.w, case.h, i), force_idr=row.idr or i == 0)
            assert plain.decode(orig) == 1
            pcm = bool((plain.mb_kinds() == OracleDecoder.KIND_IPCM).any())
            au = orig if pcm else reheaded_au(orig, row)
            reheaded = au != orig
        else:
            au, idr, _ = enc.random_picture(range_ends.seed(case, i) + 7919 * case.rows, features=case.features)
            orig, reheaded, pcm = au, False, False
        assert dec.decode(au) == 1, "%s picture %d: the independent decoder decodes every picture" % (case.name, i)
        planes = tuple(dec.plane(p) for p in range(3))
        for a in planes:
            a.setflags(write=False)
        out.append(Picture(au, orig, idr, row, reheaded, pcm, planes, dec.dbf(), dec.stats(), dec.mb_kinds()))
    enc.close(); dec.close(); plain.close()
    return tuple(out)


def account(cases):
    """the sum of the filter accounts of every picture of the cases"""
    total = Dbf()
    for c in cases:
        for p in stream(c):
            total = total + p.dbf
    return total


def account_of(aus):
    """the filter account of a list of access units, decoded by a decoder of their own"""
    dec, total = OracleDecoder(), Dbf()
    for au in aus:
        if dec.decode(au) == 1:
            total = total + dec.dbf()
    dec.close()
    return total


# ---------------------------------------------------------------- the cells a list has to reach
LUMA, CHROMA = 0, 1
DELTA = ("delta_clip_neg", "delta_clip_pos", "delta_unclipped", "delta_zero")
CLIP1 = ("clip1_p0_at_0", "clip1_p0_at_255", "clip1_q0_at_0", "clip1_q0_at_255")


def _branch_cells():
    """(cell, kind, the bS values it is counted over - one each): every one needs one line"""
    out = []
    for kind in (LUMA, CHROMA):
        out += [(c, kind, (bs,)) for c in ("rej_alpha", "rej_p", "rej_q") for bs in (1, 2, 3, 4)]
        out += [(c, kind, (bs,)) for c in DELTA for bs in (1, 2, 3)]
        out += [(c, kind, (bs,)) for c in CLIP1 for bs in (1, 2, 3)]
    out += [(c, LUMA, (bs,)) for c in ("apaq_00", "apaq_01", "apaq_10", "apaq_11", "p1_clip_neg", "p1_clip_pos", "p1_unclipped",
                                       "q1_clip_neg", "q1_clip_pos", "q1_unclipped") for bs in (1, 2, 3)]
    out += [(c, LUMA, (4,)) for c in ("strong_00", "strong_01", "strong_10", "strong_11", "strong_false")]
    return tuple(out)


BRANCH_CELLS = _branch_cells()
CONTEXT_CELLS = Dbf.CTX
# cells no stream can reach, each with the argument from the formulas of 8.7 (at most three; failing to find content is no argument)
UNREACHABLE = {}


def branch_count(dbf, cell):
    name, kind, bss = cell
    return int(sum(dbf.cells[name][kind, bs - 1] for bs in bss))


def coverage(dbf):
    """the summary of an account that DESIGN.md tabulates: of the 288 (kind, bS, indexA 16 .. 51) cells, how many have no filtered
    line, fewer than FLOOR filtered lines, fewer than FLOOR lines with a changed sample; indexB 16 .. 51 (of 72: kind, index) never
    filtered; luma indexB at which ap < beta is not met both true and false; branch and context cells never met"""
    filt, chg = dbf.tables["a_filt"][:, :, 16:], dbf.tables["a_changed"][:, :, 16:]
    bf = dbf.tables["b_filt"].sum(axis=1)[:, 16:]
    bl, ap = dbf.tables["b_filt"][LUMA].sum(axis=0)[16:], dbf.tables["b_ap"][LUMA].sum(axis=0)[16:]
    return {"lines": int(dbf.tables["a_eval"].sum()), "filtered": int(dbf.tables["a_filt"].sum()),
            "never": int((filt == 0).sum()), "filtered<%d" % FLOOR: int((filt < FLOOR).sum()), "changed<%d" % FLOOR: int((chg < FLOOR).sum()),
            "indexB never": int((bf == 0).sum()), "ap one-sided": int(((ap == 0) | (ap == bl)).sum()),
            "branch unmet": sum(branch_count(dbf, c) == 0 for c in BRANCH_CELLS), "context unmet": sum(dbf.ctx[c] == 0 for c in CONTEXT_CELLS),
            "filtered below 16": int(dbf.tables["a_filt"][:, :, :16].sum())}
