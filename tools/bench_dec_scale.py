"""What the decoder's resampling output costs per 1080p picture (media_amd/csrc/k_dec_out_scale.h): one decoded picture (S1, QP 26,
written by the HIP encoder) read into device memory as I420, alternating in one run between
    native      k_dec_out<I420>, 1920x1080
    1280x720    k_dec_out_scaled<I420>
    480x270     k_dec_out_scaled<I420>
    d2d         a device-to-device copy of the picture's 3 110 400 source bytes (torch)
Prints one JSON line per form: the median, minimum and maximum over --repeat windows of --calls calls each of the host's time per
call (every read call ends in a synchronise; the copies are synchronised once per window, so their figure has no per-call wait in
it).  Kernel times proper: run it under `rocprofv3 --kernel-trace --stats -- python tools/bench_dec_scale.py --repeat 1`.

    python tools/bench_dec_scale.py [--calls 200] [--repeat 5] [--layout i420]"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
WIDTH, HEIGHT, QP = 1920, 1080, 26
LAYOUTS = {"i420": 0, "nv12": 1, "nv21": 2, "rgba": 3}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--layout", default="i420", choices=sorted(LAYOUTS))
    a = ap.parse_args()
    import torch
    from media_amd import capi, synth, h264dec
    lay = LAYOUTS[a.layout]
    enc = capi.Encoder(WIDTH, HEIGHT, qp=QP, gop=30)
    au = enc.encode(synth.sequence("s1", WIDTH, HEIGHT, 1)[0])[0]
    enc.close()
    dec = h264dec.Decoder()
    assert dec.decode(au)
    dst = torch.empty(WIDTH * HEIGHT * 4, dtype=torch.uint8, device="cuda")
    src = torch.empty(WIDTH * HEIGHT * 3 // 2, dtype=torch.uint8, device="cuda")
    forms = [("native", (0, 0)), ("1280x720", (1280, 720)), ("480x270", (480, 270)), ("d2d", None)]

    def window(size):
        if size is None:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.calls):
                dst[:src.numel()].copy_(src)
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) / a.calls
        dec.set_output_size(*size)
        t0 = time.perf_counter()
        for _ in range(a.calls):
            dec.read(lay, 1, device_tensor=dst)
        return (time.perf_counter() - t0) / a.calls

    for _, size in forms:   # warm every shape
        window(size)
    runs = {name: [] for name, _ in forms}
    for _ in range(a.repeat):
        for name, size in forms:
            runs[name].append(window(size) * 1e6)
    for name, _ in forms:
        v = runs[name]
        print(json.dumps({"form": name, "layout": a.layout, "calls": a.calls, "us_per_call_median": round(statistics.median(v), 2),
                          "us_per_call_min": round(min(v), 2), "us_per_call_max": round(max(v), 2), "runs": [round(x, 2) for x in v]}), flush=True)
    dec.close()


if __name__ == "__main__":
    main()
