"""The launch order of submit_step (media_amd/csrc/engine.h) as the profiler sees it, for comparing two builds of the library.
   rocprofv3 --kernel-trace --output-format csv -d DIR -- python tools/step_trace.py run      (MI355X_H264_LIB names the build)
   python tools/step_trace.py list DIR > profiles/NAME.txt
run: 2 closed GOPs of 4 pictures in lockstep (direct, batch 2), then three streams of one hub (two reference pictures, QP 22 / 30 /
38, the last with two temporal layers, an IDR picture forced on the second at picture 3; three idle streams beside them and one P
context, so that a P step's share is all three), 6 pictures each, all at 96x80.  Every tick's pictures leave a gate together on
native threads (tools/stream_tick.cpp) and the gather window is half a second; which pictures share a step is still a matter of
timing, so `run` prints the steps as the hub reports them.
list: per hardware queue, in dispatch order, one line per launch: kernel name, grid, workgroup size."""
import csv
import ctypes as C
import glob
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H = 96, 80


def run():
    os.environ["MI355X_H264_HUB_WINDOW_US"] = "500000"
    os.environ["MI355X_H264_HUB_CTX"] = "1"
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch
    from media_amd import capi, synth
    frames = [np.ascontiguousarray(f) for f in synth.sequence("s1", W, H, 8)]
    fbytes = W * H * 3 // 2
    # direct: item g codes pictures 4 g .. 4 g + 3
    dev = torch.from_numpy(np.stack(frames)).cuda()
    enc = capi.Encoder(W, H, qp=26, gop=4, batch=2)
    cap = 8 * fbytes
    out, sizes, gb = np.zeros(2 * cap, np.uint8), np.zeros(8, np.uint32), np.zeros(2, np.uint64)
    enc.encode_gops_device(dev.data_ptr(), fbytes, 4 * fbytes, 4, out, cap, sizes, gb)
    enc.close()
    print("direct: sizes %s" % sizes.tolist())

    class Job(C.Structure):   # StreamTickJob of tools/stream_tick.cpp
        _fields_ = [("stream", C.c_void_p), ("pic", C.c_void_p), ("w", C.c_int32), ("h", C.c_int32), ("device", C.c_int32), ("rc", C.c_int32),
                    ("out", C.c_void_p), ("len", C.c_uint32), ("frame_type", C.c_int32)]
    with tempfile.TemporaryDirectory() as d:
        so = os.path.join(d, "libstream_tick.so")
        subprocess.check_call(["g++", "-O1", "-std=c++17", "-shared", "-fPIC", "-pthread", os.path.join(ROOT, "tools", "stream_tick.cpp"), "-o", so])
        T = C.CDLL(so)
    T.stream_tick.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(Job), C.c_int]
    host = C.cast(capi.lib().mi355x_h264_stream_encode, C.c_void_p)
    devfn = C.cast(capi.lib().mi355x_h264_stream_encode_device, C.c_void_p)
    streams = [capi.Stream(W, H, qp=qp, gop=30, refs=2, temporal_layers=layers) for qp, layers in ((22, 1), (30, 1), (38, 2))]
    idle = [capi.Stream(W, H, qp=26, gop=30, refs=2) for _ in range(3)]
    for i in range(6):
        if i == 3:
            streams[1].force_idr()
        jobs = (Job * 3)(*[Job(s.h.value, frames[(i + k) % 8].ctypes.data, W, H, 0, 0, None, 0, 0) for k, s in enumerate(streams)])
        assert T.stream_tick(host, devfn, jobs, 3) == 0
        for s, j in zip(streams, jobs):
            s._check(j.rc)
        steps = [s.last_step() for s in streams]
        print("hub picture %d: %s" % (i, ["step %d position %d of %d%s" % (t["serial"], t["position"], t["pictures"], " (IDR)" if t["idr"] else "") for t in steps]))
    for s in streams + idle:
        s.close()


def listing(directory):
    files = sorted(glob.glob(os.path.join(directory, "**", "*kernel_trace.csv"), recursive=True))
    assert len(files) == 1, files
    rows = list(csv.DictReader(open(files[0])))
    rows.sort(key=lambda r: int(r["Dispatch_Id"]))
    queues = {}
    for r in rows:
        queues.setdefault(r["Queue_Id"], []).append(r)
    for n, (q, rs) in enumerate(queues.items()):     # (queue ids differ from run to run: numbered in the order of their first launch)
        print("queue %d: %d launches" % (n, len(rs)))
        for r in rs:
            print("  %s grid (%s, %s, %s) workgroup (%s, %s, %s)" % (r["Kernel_Name"], r["Grid_Size_X"], r["Grid_Size_Y"], r["Grid_Size_Z"],
                                                                    r["Workgroup_Size_X"], r["Workgroup_Size_Y"], r["Workgroup_Size_Z"]))


if __name__ == "__main__":
    if len(sys.argv) == 2 and sys.argv[1] == "run":
        run()
    elif len(sys.argv) == 3 and sys.argv[1] == "list":
        listing(sys.argv[2])
    else:
        sys.exit(__doc__)
