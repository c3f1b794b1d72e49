#!/usr/bin/env python3
"""usage: MI355X_H264_LIB=<a -DME_AB_COUNT build> me_counts.py [bench.py arguments]
Runs bench.py in this process and prints what mi355x_h264_me_counts() has counted over it (media_amd/csrc/k_me.h, MEC_*), one JSON line.
Default arguments: one closed GOP of the bench workload (the table in k_me.h section 1 and DESIGN.md section 11)."""
import ctypes, json, os, runpy, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("test1_hit", "test1_rejected_block_sums", "test1_rejected_later", "test2_tried", "test2_rejected_luma_block_sums",
         "test2_rejected_chroma_dc", "test2_rejected_transform", "test2_hit", "seeded_test_won", "exhaustive_pass_run")
sys.path.insert(0, ROOT)
sys.argv = [os.path.join(ROOT, "bench.py")] + (sys.argv[1:] or "--gops-in-flight 1 --instances 1 --steps 1 --warmup 0 --no-cpu-baseline".split())
runpy.run_path(sys.argv[0], run_name="__main__")
from media_amd import capi
out = (ctypes.c_uint * len(NAMES))()
rc = capi.lib().mi355x_h264_me_counts(out, 1)
print(json.dumps({"me_counts": dict(zip(NAMES, out)) if rc == 0 else None, "rc": rc}))
