"""The caller's output buffer is too small: mi355x_h264_encode_batch_device / _encode_gops_device return
MI355X_H264_E_OVERFLOW, write nothing behind the stated capacity, and the handle goes on with an IDR picture (the contract of
E_OVERFLOW in include/mi355x_h264.h: the picture that did not fit is missing from the caller's stream)."""
import numpy as np
import pytest

from media_amd import capi, synth
from oracle_lib import OracleEncoder

pytestmark = pytest.mark.gpu
W, H, GUARD = 176, 144, 4096


def test_batch_output_too_small_is_refused_and_the_next_picture_is_an_idr():
    frames = list(synth.sequence("s1", W, H, 6))
    fbytes = W * H * 3 // 2
    import torch
    dev = torch.from_numpy(np.stack(frames)).cuda()
    enc, orc = capi.Encoder(W, H, qp=24, gop=100), OracleEncoder(W, H, qp=24, gop=100)
    want = [orc.encode(f)[0] for f in frames[:4]]
    cap = len(want[0]) + len(want[1]) + len(want[2]) // 2   # the third picture does not fit
    buf = np.full(cap + GUARD, 0xA5, np.uint8)
    sizes = np.zeros(4, np.uint32)
    with pytest.raises(capi.EncoderError) as ei:
        enc.encode_batch_device(dev.data_ptr(), fbytes, 4, buf[:cap], sizes)
    assert ei.value.rc == capi.E_OVERFLOW
    assert (buf[cap:] == 0xA5).all()
    assert bytes(buf[: len(want[0]) + len(want[1])]) == want[0] + want[1]
    # the handle stays usable, and what it codes next does not refer to the pictures the caller never received
    got, ft = enc.encode(frames[4])
    ref, idr = orc.encode(frames[4], force_idr=True)
    assert ft == capi.FRAME_IDR and idr
    assert got == ref
    assert enc.encode(frames[5])[0] == orc.encode(frames[5])[0]
    enc.close()


def test_gops_output_too_small_is_refused_and_the_handle_stays_usable():
    G, gop = 2, 3
    frames = list(synth.sequence("s1", W, H, G * gop))
    fbytes = W * H * 3 // 2
    import torch
    dev = torch.from_numpy(np.stack(frames)).cuda()
    enc = capi.Encoder(W, H, qp=24, gop=gop, batch=G)
    want = []
    for g in range(G):
        orc = OracleEncoder(W, H, qp=24, gop=gop)
        orc.set_idr_id(g, G)
        want.append([orc.encode(f)[0] for f in frames[g * gop: (g + 1) * gop]])
    cap = len(want[0][0]) + len(want[0][1]) // 2   # the second picture of a GOP does not fit
    buf = np.full(G * cap + GUARD, 0xA5, np.uint8)
    sizes, gb = np.zeros(G * gop, np.uint32), np.zeros(G, np.uint64)
    with pytest.raises(capi.EncoderError) as ei:
        enc.encode_gops_device(dev.data_ptr(), fbytes, gop * fbytes, gop, buf[: G * cap], cap, sizes, gb)
    assert ei.value.rc == capi.E_OVERFLOW
    assert (buf[G * cap:] == 0xA5).all()
    assert bytes(buf[: len(want[0][0])]) == want[0][0]
    big = 1 << 20
    out = np.zeros(G * big, np.uint8)
    enc.set_idr_pic_id(0)
    enc.encode_gops_device(dev.data_ptr(), fbytes, gop * fbytes, gop, out, big, sizes, gb)
    for g in range(G):
        assert bytes(out[g * big: g * big + int(gb[g])]) == b"".join(want[g])
    enc.close()
