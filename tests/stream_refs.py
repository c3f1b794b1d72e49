"""Streams that search two and three reference pictures (mi355x_h264_stream_open_ex, MI355X_H264_STREAM_MULTIREF): the cases that
tests/test_stream_refs_oracle.py (CPU: what the list holds) and tests/test_gpu_stream_refs.py (GPU) share.

One stream per case: cases of tests/ref_mix.py, whose older pictures win.  The MIXED group: six streams of the split_48x48 content
at seeds and starts of their own, refs = 3, stream k handing in its first picture at tick k, every stream with a GOP length of its
own, one forced IDR picture and a QP walk in mid-run.  In a shared step every position then has its own number of usable reference
pictures, min(3, pictures since ITS stream's IDR): ticks in which pictures with one, two and three occur together are what the
indirect kernels' per-position count is for.

Everything is deterministic; what is computed is computed once per process, shared and never changed."""
import functools
from collections import namedtuple
import ref_mix as rm

# one stream per case (tests/ref_mix.py says what each is for)
ONE = tuple(rm.BY_NAME[n] for n in ("split_48x48", "s1_208x160", "split_96x80_high", "still_96x80", "fast_96x128", "two_refs_split", "nv12",
                                    "long_ring"))

# ---------------------------------------------------------------- the mixed group
REFS = 3
TICKS = 13
GOPS = (6, 5, 7, 4, 9, 6)
SEEDS = (1, 8, 19, 4, 36, 50)     # of ref_mix.period_map: every one gives the nine macroblocks all three periods
# (picture of the stream, "idr": force an IDR picture | a QP to set) before that picture is coded
EVENTS = {1: ((7, "idr"),), 2: ((3, 22), (5, 31), (7, 38), (9, 26))}
IDLE = 6      # streams opened beside the six and never used: with ONE P context the P share, (open + 1) // 2, is then all six

Member = namedtuple("Member", "k case join events")


def member(k):
    """stream k of the mixed group: joins at tick k, codes TICKS - k pictures"""
    b = rm.BY_NAME["split_48x48"]
    c = b._replace(name="mixed_%d" % k, seed=SEEDS[k], start=b.start + 3 * k + (k & 1), gop=GOPS[k], pictures=TICKS - k)
    return Member(k, c, k, EVENTS.get(k, ()))


MIXED = tuple(member(k) for k in range(len(GOPS)))


def ref_counts(refs, gop, pictures, forced=()):
    """usable reference pictures of every picture of a stream: 0 = an IDR picture (the first, every gop-th after an IDR, a forced
    one), else min(refs, pictures since the IDR) - include/mi355x_h264.h, "streams", restated"""
    out, since = [], 0
    for i in range(pictures):
        idr = i == 0 or since >= gop or i in forced
        since = 0 if idr else since
        out.append(0 if idr else min(max(refs, 1), since))
        since += 1
    return out


def member_counts(m):
    return ref_counts(m.case.refs, m.case.gop, m.case.pictures, [at for at, what in m.events if what == "idr"])


@functools.lru_cache(maxsize=None)
def schedule():
    """per tick: ((stream, picture of the stream, reference count), ..) of the streams that hand a picture in"""
    counts = [member_counts(m) for m in MIXED]
    return tuple(tuple((m.k, t - m.join, counts[m.k][t - m.join]) for m in MIXED if t >= m.join) for t in range(TICKS))


def mixed_ticks():
    """the ticks whose P pictures have one, two and three reference pictures between them"""
    return tuple(t for t, tick in enumerate(schedule()) if {1, 2, 3} <= {n for _, _, n in tick})


def expected(m, search=1):
    """the oracle's stream of a member, driven as the member is (ref_mix.expected: decoded and checked)"""
    return rm.expected(m.case, search, m.events)


@functools.lru_cache(maxsize=None)
def expected_with_refs(c, refs, search=1):
    """the oracle's stream of the case's OWN pictures coded with another number of reference pictures (ref_mix.expected of a case
    with other refs would draw other pictures): a tuple of ref_mix.Pic without facts"""
    from large_batch import StagesOf
    orc = rm.oracle_for(c._replace(refs=refs), search)
    out = []
    for f in rm.frames(c):
        au, idr = orc.encode(f)
        out.append(rm.Pic(au, idr, StagesOf(orc), None))
    orc.close()
    return tuple(out)
