"""Intra refresh at 1080p: what it costs and what it buys (profiles/intra_refresh_1080p.json).
   python tools/bench_intra_refresh.py [--out FILE] [--streams 16] [--pictures 120] [--repeat 3]
benefit: largest and mean access-unit bytes over PICTURES pictures of the S1 content at QP 26 - gop = 30 without refresh against
         gop = PICTURES with refresh over 8 bands (one encoder each, host I420);
cost:    fps of STREAMS plugin objects with 8 slices through media_amd/lib/plugin_bench (bitrate mode, scene detection on), without
         and with --intra-refresh 8, alternated REPEAT times in one process chain.
Reported only: no threshold."""
import argparse
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
from media_amd import capi, synth  # noqa: E402

W, H, QP, N = 1920, 1080, 26, 8


def sizes(frames, **kw):
    enc = capi.Encoder(W, H, qp=QP, **kw)
    try:
        out = [(len(au), ft == capi.FRAME_IDR, enc.last_refresh_band) for au, ft in (enc.encode(f) for f in frames)]
    finally:
        enc.close()
    b = [s for s, _, _ in out]
    return {"pictures": len(b), "idr_pictures": sum(i for _, i, _ in out), "largest": max(b), "mean": round(sum(b) / len(b), 1), "total": sum(b),
            "largest_p": max(s for s, i, _ in out if not i), "bytes": b}


def plugin(path, nsrc, frames, streams, refresh):
    exe = os.path.join(ROOT, "media_amd", "lib", "plugin_bench")
    env = dict(os.environ)
    env.update({"RO_VMI_DEMO_VIDEO_ENCODE_FORMAT": "3", "RO_SYS_VMI_CLOUDPHONE": "video", "RO_HARDWARE_WIDTH": str(W), "RO_HARDWARE_HEIGHT": str(H),
                "RO_HARDWARE_FPS": "30", "PERSIST_VMI_VIDEO_ENCODE_BITRATE": "5000000", "PERSIST_VMI_VIDEO_ENCODE_GOPSIZE": "120",
                "PERSIST_VMI_VIDEO_ENCODE_PROFILE": "baseline", "PERSIST_VMI_VIDEO_ENCODE_PARAM_ADJUSTING": "0", "PERSIST_VMI_VIDEO_ENCODE_KEYFRAME": "0",
                "PERSIST_VMI_VIDEO_ENCODE_SCENEDETECT": "1", "PERSIST_VMI_VIDEO_ENCODE_SLICES": str(N), "MEDIA_LOG_QUIET": "1"})
    env.pop("PERSIST_VMI_VIDEO_ENCODE_QP", None)
    env.pop("PERSIST_VMI_VIDEO_ENCODE_INTRAREFRESH", None)
    args = [exe] + (["--intra-refresh", str(N)] if refresh else []) + [path, str(W), str(H), str(nsrc), str(frames), str(streams)]
    r = subprocess.run(args, env=env, capture_output=True, text=True, timeout=400)
    rows = [json.loads(ln) for ln in r.stdout.splitlines() if ln.startswith("{")]
    if r.returncode != 0 or not rows:
        raise SystemExit("plugin_bench exited %d: %s" % (r.returncode, r.stderr[-400:]))
    return rows[0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "intra_refresh_1080p.json"))
    ap.add_argument("--streams", type=int, default=16)
    ap.add_argument("--pictures", type=int, default=120)
    ap.add_argument("--repeat", type=int, default=3)
    a = ap.parse_args()
    frames = synth.sequence("s1", W, H, a.pictures + a.streams + 1)
    res = {"content": "S1 %dx%d" % (W, H), "qp": QP, "bands": N,
           "benefit": {"gop30_one_slice": sizes(frames[:a.pictures], gop=30),
                       "gop30_slices8": sizes(frames[:a.pictures], gop=30, slices=N),
                       "gop%d_refresh8" % a.pictures: sizes(frames[:a.pictures], gop=a.pictures, slices=N, intra_refresh=True)},
           "cost": {"streams": a.streams, "pictures_per_stream": a.pictures, "slices8": [], "slices8_refresh": []}}
    with tempfile.NamedTemporaryFile(suffix=".i420") as f:
        for fr in frames:
            f.write(np.ascontiguousarray(fr).tobytes())
        f.flush()
        for _ in range(a.repeat):
            res["cost"]["slices8"].append(plugin(f.name, len(frames), a.pictures, a.streams, False))
            res["cost"]["slices8_refresh"].append(plugin(f.name, len(frames), a.pictures, a.streams, True))
    with open(a.out, "w") as o:
        json.dump(res, o, indent=1)
        o.write("\n")
    for k, v in res["benefit"].items():
        print(k, {x: v[x] for x in ("idr_pictures", "largest", "largest_p", "mean", "total")})
    for k in ("slices8", "slices8_refresh"):
        print(k, [{x: r.get(x) for x in ("fps", "p50_ms", "bytes")} for r in res["cost"][k]])


if __name__ == "__main__":
    main()
