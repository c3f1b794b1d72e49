"""Aggregate decode throughput of S 1080p streams: one DecoderGroup against S Decoder objects on S host threads.
The content is what `bench.py --mode decode` decodes (S1, QP 26, GOP 30, written by the HIP encoder); every stream gets the same
access units.  Both forms run interleaved, --repeat times each, in one process, once per read mode of --read:
    none   nothing is read back
    each   every stream's picture with read_i420(k), one after the other (the objects: i420() on each stream's thread)
    all    all pictures of a step with one read_all() (--layout, to the host)
    armed  set_output() once; per step decode(t + 1), then output(back=1): the pictures of step t, copied while t + 1 was parsed
--out-size WxH (with all / armed) adds a third form, group_scaled: the same group with every stream's output size set
(mi355x_h264_dec_group_set_output_size), interleaved with the other forms in the same run; --no-objects leaves the objects out.
The objects know `none` and read every picture back in all other modes.  Prints one JSON line per (S, form, read) with median and
min / max fps, and for the group the host's parse / launch time per picture (mi355x_h264_dec_group_last_step).  Kernel times: run it
once under `rocprofv3 --kernel-trace --stats -- python tools/bench_dec_group.py --streams 16 --repeat 1 --read armed`.

    python tools/bench_dec_group.py [--streams 1,4,16,32] [--pictures 60] [--repeat 3] [--read none,each] [--layout i420]
                                    [--out-size 480x270] [--no-objects]"""
import argparse
import json
import os
import statistics
import sys
import threading
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
WIDTH, HEIGHT, QP, GOP = 1920, 1080, 26, 30


def make_stream(n):
    from media_amd import capi, synth
    enc = capi.Encoder(WIDTH, HEIGHT, qp=QP, gop=GOP)
    aus = [enc.encode(f)[0] for f in synth.sequence("s1", WIDTH, HEIGHT, n)]
    enc.close()
    return aus


LAYOUTS = {"i420": 0, "nv12": 1, "nv21": 2, "rgba": 3}


def run_group(aus, S, read, layout=0, out_size=None):
    from media_amd import h264dec
    g = h264dec.DecoderGroup(S)
    if out_size:
        g.set_output_size(-1, *out_size)
    parse_us = launch_us = 0
    dst = None  # read_all's destination
    taken = 0   # bytes looked at, so that no mode gets away with not touching its pictures
    t0 = time.perf_counter()
    if read == "armed":
        g.set_output(layout)
    for t, au in enumerate(aus):
        res = g.decode([au] * S)
        assert all(r == (0, 1) for r in res), res
        st = g.last_step()
        parse_us += st["parse_us"]; launch_us += st["launch_us"]
        if read == "each":
            for k in range(S):
                taken += g.read_i420(k).size
        elif read == "all":
            buf, _ = g.read_all(layout, out=dst)
            dst = buf.base if buf.base is not None else buf   # (the first call's array serves the others)
            taken += buf.size
        elif read == "armed" and t > 0:
            taken += g.output(1)[0].size
    if read == "armed":
        taken += g.output(0)[0].size
    g.sync()
    dt = time.perf_counter() - t0
    g.close()
    n = len(aus) * S
    return n / dt, {"parse_ms_per_picture": parse_us / 1e3 / n, "launch_ms_per_picture": launch_us / 1e3 / n}


def run_objects(aus, S, read):
    from media_amd import h264dec
    decs = [h264dec.Decoder() for _ in range(S)]
    start = threading.Barrier(S + 1)

    def work(d):
        start.wait()
        for au in aus:
            assert d.decode(au)
            if read != "none":
                d.i420()
        d.sync()

    th = [threading.Thread(target=work, args=(d,)) for d in decs]
    for t in th:
        t.start()
    start.wait()
    t0 = time.perf_counter()
    for t in th:
        t.join()
    dt = time.perf_counter() - t0
    out = {}
    n, p, g = zip(*[d.timing() for d in decs])
    out["parse_ms_per_picture"] = sum(p) / sum(n)
    out["gpu_ms_per_picture"] = sum(g) / sum(n)
    for d in decs:
        d.close()
    return len(aus) * S / dt, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", default="1,4,16,32")
    ap.add_argument("--pictures", type=int, default=60)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--read", default="none,each", help="read modes, comma-separated: none, each, all, armed")
    ap.add_argument("--layout", default="i420", choices=sorted(LAYOUTS), help="of the modes all and armed")
    ap.add_argument("--out-size", default="", help="WxH: also run the group with this output size for every stream (modes all and armed)")
    ap.add_argument("--no-objects", action="store_true", help="leave out the S Decoder objects")
    a = ap.parse_args()
    modes = a.read.split(",")
    assert all(m in ("none", "each", "all", "armed") for m in modes), modes
    out_size = tuple(int(x) for x in a.out_size.split("x")) if a.out_size else None
    assert out_size is None or (len(out_size) == 2 and all(m in ("all", "armed") for m in modes)), "--out-size WxH goes with --read all|armed"
    aus = make_stream(a.pictures)
    for S in [int(x) for x in a.streams.split(",")]:
        for read in modes:
            forms = ["group"] + (["group_scaled"] if out_size else []) + ([] if a.no_objects else ["objects"])
            runs = {form: [] for form in forms}
            extra = {}
            for _ in range(a.repeat):
                for form in forms:
                    if form == "objects":
                        fps, extra[form] = run_objects(aus, S, read)
                    else:
                        fps, extra[form] = run_group(aus, S, read, LAYOUTS[a.layout], out_size if form == "group_scaled" else None)
                    runs[form].append(fps)
            for form in forms:
                v = runs[form]
                if form == "group_scaled":
                    extra[form]["out_size"] = a.out_size
                print(json.dumps(dict({"streams": S, "form": form, "read_back": read != "none", "read": read, "layout": a.layout if read in ("all", "armed") else "i420", "pictures_per_stream": a.pictures, "fps_median": round(statistics.median(v), 1),
                                       "fps_min": round(min(v), 1), "fps_max": round(max(v), 1), "runs": [round(x, 1) for x in v]}, **extra[form])), flush=True)


if __name__ == "__main__":
    main()
