"""Rate-distortion points from the GPU: bytes and PSNR per picture type for the six synthetic contents of media_amd/synth.py at
1080p, QP 22 / 26 / 32 / 38, both values of config.search - the table of DESIGN.md section 3 ("cost of the seeded form") at the
size the product runs at.  The distortion is the library's own quality report (include/mi355x_h264.h, mi355x_h264_quality_read:
integer SSE per plane from the device); PSNR is computed here, from the SSE summed over the pictures of a type.

   python tools/rd_points.py [--pictures N] [--width W --height H] [--out profiles/quality_rd_1080p.json]
   python tools/rd_points.py --ssim [...] [--out profiles/ssim_rd_1080p.json]
--ssim: the report runs with both metrics (mi355x_h264_quality_enable_ex) and every point carries the mean SSIM Y / U / V beside the
PSNR - sum / (65536 * windows) over the pictures of a type, computed here - and the seeded search's SSIM difference; the default
output file is then profiles/ssim_rd_1080p.json, and quality_rd_1080p.json stays as it is.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from media_amd import capi, synth   # noqa: E402

CONTENTS = ("s1", "scroll", "split", "cut", "s3", "ramp")
QPS = (22, 26, 32, 38)
SEARCHES = (("exhaustive", 0), ("seeded", 1))


def run(frames, w, h, qp, search, ssim=False):
    """one closed GOP (IDR + P pictures) -> {"idr": .., "p": ..}: pictures, mean bytes, PSNR Y / U / V of the summed SSE (ssim: and
    the mean SSIM Y / U / V of the summed window values)"""
    enc = capi.Encoder(w, h, qp=qp, gop=len(frames), search=search)
    acc = {"idr": [0, 0, [0, 0, 0], [0, 0, 0], [0, 0, 0], [0, 0, 0]], "p": [0, 0, [0, 0, 0], [0, 0, 0], [0, 0, 0], [0, 0, 0]]}
    try:
        enc.quality_enable(True, ssim=ssim)
        for f in frames:
            au, ft = enc.encode(f)
            rec = enc.quality()[0]
            assert rec["valid"] and rec["bytes"] == len(au)
            a = acc["idr" if ft == capi.FRAME_IDR else "p"]
            a[0] += 1
            a[1] += len(au)
            for p in range(3):
                a[2][p] += rec["sse"][p]
                a[3][p] += rec["samples"][p]
                if ssim:
                    a[4][p] += rec["ssim_sum"][p]
                    a[5][p] += rec["ssim_windows"][p]
    finally:
        enc.close()
    out = {}
    for k, (n, nbytes, sse, samples, qsum, windows) in acc.items():
        if n:
            db = [capi.psnr(s, m) for s, m in zip(sse, samples)]
            out[k] = {"pictures": n, "bytes_mean": round(nbytes / n, 1), "psnr_y": round(min(db[0], 999.0), 3), "psnr_u": round(min(db[1], 999.0), 3),
                      "psnr_v": round(min(db[2], 999.0), 3), "sse": sse}
            if ssim:
                out[k].update({"ssim_y": round(capi.ssim_mean(qsum[0], windows[0]), 5), "ssim_u": round(capi.ssim_mean(qsum[1], windows[1]), 5),
                               "ssim_v": round(capi.ssim_mean(qsum[2], windows[2]), 5), "ssim_sum": qsum, "ssim_windows": windows})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pictures", type=int, default=8)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--ssim", action="store_true", help="both metrics: the mean SSIM beside the PSNR")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.out is None:
        args.out = os.path.join(ROOT, "profiles", "ssim_rd_1080p.json" if args.ssim else "quality_rd_1080p.json")
    w, h = args.width, args.height
    res = {"what": "bytes and PSNR%s per picture type from the GPU (mi355x_h264_quality_read%s), one closed GOP of %d pictures, %dx%d, Baseline"
                   % (" and mean SSIM" if args.ssim else "", ", mi355x_h264_quality_ssim_read" if args.ssim else "", args.pictures, w, h),
           "points": []}
    for content in CONTENTS:
        frames = synth.sequence(content, w, h, args.pictures)
        for qp in QPS:
            row = {"content": content, "qp": qp}
            for name, search in SEARCHES:
                try:
                    row[name] = run(frames, w, h, qp, search, args.ssim)
                except capi.EncoderError as err:   # (a picture refused with E_OVERFLOW: noise at the lowest QPs)
                    row[name] = {"error": str(err)}
            e, s = row["exhaustive"].get("p"), row["seeded"].get("p")
            if e and s:   # the cost of the seeded form: bytes per P picture at equal QP, and what it does to the luma PSNR
                row["seeded_p_bytes_pct"] = round(100.0 * (s["bytes_mean"] / e["bytes_mean"] - 1.0), 3)
                row["seeded_p_psnr_y_db"] = round(s["psnr_y"] - e["psnr_y"], 3)
                if args.ssim:
                    row["seeded_p_ssim_y"] = round(s["ssim_y"] - e["ssim_y"], 5)
            res["points"].append(row)
            print(json.dumps(row), flush=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
