"""The decoder peer is a decoder group of one stream (media_amd/csrc/decoder.h): what a Decoder does that a DecoderGroup does not - a
new coded size at an IDR picture, in both directions - and what it must keep doing as a wrapper: S objects on S threads, the running
sums of timing().  Every picture is compared with the oracle's independent decoder, sample for sample: integer kernels, no tolerance."""
import threading

import numpy as np
import pytest

import annexb
import dec_output as do
from media_amd import synth, h264dec
from oracle_lib import OracleEncoder, OracleDecoder

pytestmark = pytest.mark.gpu
E_STREAM = h264dec.E_STREAM


def segment(kind, w, h, n=3, **kw):
    """n pictures (IDR, P, ...) of an oracle-encoder stream: [(access unit, coded planes, cropped I420, display size)] as the
    oracle decoder sees them"""
    enc, ref = OracleEncoder(w, h, qp=28, gop=30, **kw), OracleDecoder()
    out = []
    for f in synth.sequence(kind, w, h, n):
        au = enc.encode(f)[0]
        assert ref.decode(au) == 1
        out.append((au, [ref.plane(p) for p in range(3)], np.concatenate([ref.cropped(p).ravel() for p in range(3)]), ref.size))
    assert out[0][3] == (w, h)
    enc.close()
    ref.close()
    return out


def parameter_sets(au):
    return b"".join(b"\x00\x00\x00\x01" + bytes([(ref << 5) | typ]) + payload for ref, typ, payload in annexb.split_nal_units(au) if typ in (7, 8))


def check_picture(dec, want, tag):
    _, planes, i420, size = want
    for p in range(3):
        assert np.array_equal(dec.plane(p), planes[p]), "%s plane %d" % (tag, p)
    assert dec.info()[:2] == size, (tag, dec.info())
    assert np.array_equal(dec.i420(), i420), "%s: i420()" % tag


def test_decoder_follows_the_coded_size_up_and_down():
    """64x48, 176x144 (growth: every array, the ring and the output staging of the smaller size are too small), 64x48 again, then
    46x30 (coded 48x32, cropped): three pictures each.  Every picture's planes, i420() and read(NV12, row_align 64) - against the
    restatement of tests/dec_output.py - are compared, so the buffers of the size before cannot have survived a change.  Ahead
    of every change, a P picture of the NEW size (with its parameter sets, without an IDR picture) is refused and leaves the last
    picture of the old size readable."""
    dec = h264dec.Decoder()
    decoded, last = 0, None
    for kind, w, h in (("s1", 64, 48), ("cut", 176, 144), ("split", 64, 48), ("s3", 46, 30)):
        seg = segment(kind, w, h, n=4)
        if last is not None:   # (the fourth picture: its frame_num follows the old stream's third, so the host parser has no say)
            with pytest.raises(h264dec.StreamError):
                dec.decode(parameter_sets(seg[0][0]) + seg[3][0])
            check_picture(dec, last, "after the refused %dx%d P picture" % (w, h))
        seg = seg[:3]
        for i, want in enumerate(seg):
            tag = "%dx%d picture %d" % (w, h, i)
            assert dec.decode(want[0]), tag
            decoded += 1
            check_picture(dec, want, tag)
            exp, written, desc, total = do.pack([(want[2], want[3])], do.NV12, 64)
            buf, pic = dec.read(h264dec.PIX_NV12, row_align=64)
            assert pic["bytes"] == total and all(pic[k] == desc[0][k] for k in desc[0]), (tag, pic, desc[0])
            assert np.array_equal(buf[written], exp[written]), tag
            assert pic["fresh"] == 1 and pic["serial"] == decoded, (tag, pic)
        last = seg[-1]
    assert dec.timing()[0] == decoded == 12
    dec.close()


def test_a_public_group_of_one_stream_keeps_its_coded_size():
    """DecoderGroup(1) is the same code without the decoder's option: the stream of another size fails alone, by name of both sizes,
    the last picture stays readable, the P picture that follows is refused for want of a reference, and the next IDR picture of
    the group's size decodes"""
    small, big, again = segment("s1", 64, 48), segment("cut", 176, 144, n=1), segment("split", 64, 48, n=2)
    grp = h264dec.DecoderGroup(1)

    def same(want, tag):
        got = grp.debug_planes(0)
        for p in range(3):
            assert np.array_equal(got[p], want[1][p]), "%s plane %d" % (tag, p)
        assert grp.info(0)[:2] == want[3] and np.array_equal(grp.read_i420(0), want[2]), tag

    for i in range(2):
        assert grp.decode([small[i][0]]) == [(0, 1)]
        same(small[i], "picture %d" % i)
    assert grp.decode([big[0][0]]) == [(E_STREAM, 0)]
    assert "differs" in grp.error(0) and "176x144" in grp.error(0) and "64x48" in grp.error(0), grp.error(0)
    same(small[1], "after the refusal")
    assert grp.decode([small[2][0]]) == [(E_STREAM, 0)] and "reference" in grp.error(0), grp.error(0)
    for i in range(2):
        assert grp.decode([again[i][0]]) == [(0, 1)], grp.error(0)
        same(again[i], "second stream, picture %d" % i)
    assert grp.last_step()["parse_threads"] == 1
    grp.close()


def test_four_decoders_on_four_threads():
    """bench.py drives S Decoder objects on S threads; each object is a group with a scheduler and two pinned sets of its own.
    Four different streams (176x144, six pictures, two reference pictures), every picture compared inside its thread."""
    streams = [segment(kind, 176, 144, n=6, refs=2) for kind in ("s1", "cut", "split", "scroll")]
    bad = []
    start = threading.Barrier(len(streams))

    def run(k):
        try:
            dec = h264dec.Decoder()
            start.wait()
            for i, want in enumerate(streams[k]):
                assert dec.decode(want[0]), "stream %d picture %d" % (k, i)
                check_picture(dec, want, "stream %d picture %d" % (k, i))
            assert dec.timing()[0] == len(streams[k])
            dec.close()
        except BaseException as ex:   # (an assertion in a thread is lost otherwise)
            start.abort()
            bad.append("stream %d: %r" % (k, ex))

    threads = [threading.Thread(target=run, args=(k,)) for k in range(len(streams))]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not bad, bad


def test_timing_sums_the_steps():
    """pictures counts the successful decode() calls; parse_ms and gpu_ms are sums: positive, never decreasing; a refused unit (the
    host parser refuses a truncated one) adds no picture"""
    seg = segment("s1", 64, 48, n=4)
    dec = h264dec.Decoder()
    assert dec.timing() == (0, 0.0, 0.0)
    before = (0, 0.0, 0.0)
    for i in range(3):
        assert dec.decode(seg[i][0])
        now = dec.timing()
        assert now[0] == i + 1 and now[1] > 0 and now[2] > 0 and now[1] >= before[1] and now[2] >= before[2], (i, before, now)
        before = now
    with pytest.raises(h264dec.StreamError):
        dec.decode(seg[3][0][: len(seg[3][0]) * 3 // 5])
    now = dec.timing()
    assert now[0] == 3 and now[1] >= before[1] and now[2] >= before[2], (before, now)
    check_picture(dec, seg[2], "after the refused unit")
    dec.close()
