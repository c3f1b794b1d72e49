"""k_tq / k_tq8 store only the levels, samples and TotalCoeff bytes a later stage reads (media_amd/csrc/k_tq.h) - run with -m gpu
on an MI355X.  The sequence of tests/tq_sparse.py (dense pictures in front of sparse ones; tests/test_tq_sparse_oracle.py proves
what it holds) goes through every path that launches the two kernels, and EVERY picture is compared with the oracle: access unit,
MbInfo fields, quadrant vectors, the levels that are read, pre-filter and final planes.  A stage that reads what was last written
for an earlier picture produces other bytes or other samples than the oracle.

Mutation check (DESIGN.md section 11 holds the outcome): a build that gates the luma level stores by the NEIGHBOURING quadrant's
bit, and one that drops the sample store of a chroma block with TotalCoeff 0 and a non-zero DC term, must both fail here."""
import numpy as np
import pytest
import mem_guard as mg
import tq_sparse as ts
from media_amd import capi

pytestmark = pytest.mark.gpu


def _single(w, h, prof, make=capi.Encoder):
    """the sequence picture by picture through one encoder object (capi.Encoder: the direct kernels; capi.Stream: a hub stream,
    the IND = true kernels), the QP set per picture"""
    exp = ts.expected(w, h, prof)
    enc = make(w, h, qp=ts.QPS[0], gop=len(ts.QPS), profile_idc=prof)
    try:
        enc.keep_pre(True)
        for i, f in enumerate(ts.frames(w, h)):
            if i:
                enc.set_qp(ts.QPS[i])
            au, ft = enc.encode(f)
            tag = "%s %dx%d profile %d picture %d qp %d" % (make.__name__, w, h, prof, i, ts.QPS[i])
            assert (ft == capi.FRAME_IDR) == exp[i].idr, tag + ": picture type"
            assert au == exp[i].au, tag + ": access unit differs from the oracle's"
            ts.compare(enc, exp[i].stages, tag)
    finally:
        enc.close()


@pytest.mark.parametrize("w,h", [ts.SIZE, ts.SMALL], ids=lambda s: str(s))
def test_single_encoder(w, h):
    _single(w, h, 66)


@pytest.mark.parametrize("w,h", [ts.SIZE, ts.SMALL], ids=lambda s: str(s))
def test_hub_stream(w, h):
    _single(w, h, 66, make=capi.Stream)


@pytest.mark.parametrize("w,h", [ts.SIZE, ts.SMALL], ids=lambda s: str(s))
def test_high_profile(w, h):
    _single(w, h, 100)


def test_high_profile_hub_stream():
    _single(*ts.SIZE, 100, make=capi.Stream)


def test_single_encoder_guarded_and_poisoned():
    """the same with guards around and poison in every allocation of the library: what the kernels no longer store is poison until
    some picture codes it, and no store lands outside its array"""
    with mg.guarded() as seen:
        _single(*ts.SIZE, 66)
    mg.clean(seen, kinds=["encoder"])


def test_lockstep_batch_of_eight():
    """encode_gops_device with eight closed GOPs per call, every call at another QP (dense, sparse, dense, sparse), the items at
    different pictures of the sequence: every access unit of every item against the oracle's serial stream, the stages of item 0's
    last picture after every call"""
    import torch
    w, h = ts.SIZE
    exp = ts.expected_batch(w, h)
    G, gop = ts.BATCH_G, ts.BATCH_GOP
    enc = capi.Encoder(w, h, qp=ts.BATCH_QPS[0], gop=gop, batch=G)
    try:
        enc.keep_pre(True)
        fbytes = w * h * 3 // 2
        cap = 2 * gop * fbytes + 4096
        out, sizes, gb = np.zeros(G * cap, np.uint8), np.zeros(G * gop, np.uint32), np.zeros(G, np.uint64)
        for call, qp in enumerate(ts.BATCH_QPS):
            enc.set_qp(qp)
            dev = torch.from_numpy(np.stack([f for g in range(G) for f in ts.batch_frames(w, h, call, g)])).cuda()
            enc.encode_gops_device(dev.data_ptr(), fbytes, gop * fbytes, gop, out, cap, sizes, gb)
            for g in range(G):
                aus = exp[call][g][0]
                o = g * cap
                for i, au in enumerate(aus):
                    n = int(sizes[g * gop + i])
                    assert out[o:o + n].tobytes() == au, "call %d (qp %d) item %d picture %d: access unit differs from the oracle's" % (call, qp, g, i)
                    o += n
                assert int(gb[g]) == o - g * cap
            ts.compare(enc, exp[call][0][1], "call %d (qp %d) item 0, last picture" % (call, qp))
            del dev
    finally:
        enc.close()
