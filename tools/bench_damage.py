"""Damage tiles measured through the plugin surface (tools/plugin_bench.cpp, media_amd/lib/plugin_bench): host-fed 1080p streams,
bitrate mode, S threads of one object each.

  python tools/bench_damage.py [--streams 1,16,64] [--shares 0,50,90,99] [--frames 240] [--pool 96] [--repeat 3]
                               [--parent-dir DIR] [--out profiles/damage_bench.log]

Two comparisons, each alternating its two sides --repeat times in this one process on one machine:
  ordinary   plain content (the `s1` sequence), the key off, this build against the parent's build when --parent-dir names a directory
             that holds the parent's plugin_bench beside its libraries; without it this build against itself (its own spread).
  damage     --static-share P content for every P of --shares, the key off against detect, both on this build.
Every run prints plugin_bench's JSON lines; the summary gives per configuration and stream count the median and the range of the
aggregate fps, the medians of the p50 / p99 call latency, the bytes put on the link per picture, the link rate and the damaged tiles
per picture (mi355x_h264_stream_last_upload; the parent's build does not report them).  Needs a GPU: plugin_bench fails without one."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
W, H = 1920, 1080


def run(exe, path, pool, frames, streams, extra, env, log):
    cmd = [exe] + extra + [path, str(W), str(H), str(pool), str(frames), streams]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=900)
    rows = [json.loads(l) for l in r.stdout.splitlines() if l.startswith("{")]
    if r.returncode != 0 or not rows or any("error" in row for row in rows):
        raise SystemExit("%s exited %d: %s %s" % (" ".join(cmd), r.returncode, r.stdout[-300:], r.stderr[-300:]))
    for row in rows:
        log(json.dumps(row))
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", default="1,16,64")
    ap.add_argument("--shares", default="0,50,90,99")
    ap.add_argument("--frames", type=int, default=240)
    ap.add_argument("--pool", type=int, default=96, help="pictures in the file; every stream cycles through them")
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--parent-dir", default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    from media_amd import synth
    out = open(args.out, "w") if args.out else None

    def log(line):
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()

    exe = os.path.join(ROOT, "media_amd", "lib", "plugin_bench")
    parent = os.path.join(args.parent_dir, "plugin_bench") if args.parent_dir else None
    env = dict(os.environ)
    env.update({"RO_VMI_DEMO_VIDEO_ENCODE_FORMAT": "3", "RO_SYS_VMI_CLOUDPHONE": "video", "RO_HARDWARE_WIDTH": str(W), "RO_HARDWARE_HEIGHT": str(H),
                "RO_HARDWARE_FPS": "30", "PERSIST_VMI_VIDEO_ENCODE_BITRATE": "5000000", "PERSIST_VMI_VIDEO_ENCODE_GOPSIZE": "30",
                "PERSIST_VMI_VIDEO_ENCODE_PROFILE": "baseline", "PERSIST_VMI_VIDEO_ENCODE_PARAM_ADJUSTING": "0", "PERSIST_VMI_VIDEO_ENCODE_KEYFRAME": "0",
                "PERSIST_VMI_VIDEO_ENCODE_SCENEDETECT": "1", "MEDIA_LOG_QUIET": "1"})
    for k in ("PERSIST_VMI_VIDEO_ENCODE_QP", "PERSIST_VMI_VIDEO_ENCODE_DAMAGE"):
        env.pop(k, None)
    results = {}   # (comparison, side, streams) -> [row, ...]

    def keep(comparison, side, rows):
        for row in rows:
            results.setdefault((comparison, side, row["streams"]), []).append(row)

    with tempfile.NamedTemporaryFile(suffix=".i420") as f:
        for fr in synth.sequence("s1", W, H, args.pool):
            f.write(np.ascontiguousarray(fr).tobytes())
        f.flush()
        log("# damage bench: %dx%d, %d frames per stream, pool of %d pictures, %d alternations; parent build: %s" %
            (W, H, args.frames, args.pool, args.repeat, "yes" if parent else "no (this build against itself)"))
        for rep in range(args.repeat):
            log("# ordinary calls, alternation %d: %s, then this build" % (rep, "the parent's build" if parent else "this build"))
            keep("ordinary", "parent" if parent else "self_a", run(parent or exe, f.name, args.pool, args.frames, args.streams, [], env, log))
            keep("ordinary", "this", run(exe, f.name, args.pool, args.frames, args.streams, [], env, log))
        for share in [int(s) for s in args.shares.split(",") if s.strip()]:
            for rep in range(args.repeat):
                log("# static share %d %%, alternation %d: off, then detect" % (share, rep))
                keep("share %d" % share, "off", run(exe, f.name, args.pool, args.frames, args.streams, ["--static-share", str(share)], env, log))
                keep("share %d" % share, "detect", run(exe, f.name, args.pool, args.frames, args.streams, ["--damage", "detect", "--static-share", str(share)], env, log))
    log("# summary: comparison | side | streams | fps median (min .. max) | p50 ms | p99 ms | upload bytes/picture | link GB/s | damaged tiles/picture of total")
    for (comparison, side, streams), rows in sorted(results.items(), key=lambda kv: (kv[0][0], kv[0][2], kv[0][1])):
        fps = [r["fps_aggregate"] for r in rows]
        med = lambda key: statistics.median(r[key] for r in rows) if all(key in r for r in rows) else None
        up, gbps, tiles = med("upload_bytes_per_picture"), med("link_gbps"), med("damaged_tiles_per_picture")
        log("%-10s | %-7s | %2d | %8.1f (%8.1f .. %8.1f) | %7.3f | %7.3f | %s | %s | %s" % (
            comparison, side, streams, statistics.median(fps), min(fps), max(fps), med("latency_ms_p50"), med("latency_ms_p99"),
            "not reported" if up is None else "%.0f" % up, "not reported" if gbps is None else "%.2f" % gbps,
            "not reported" if tiles is None else "%.1f of %d" % (tiles, rows[0]["tiles_total"])))


if __name__ == "__main__":
    main()
