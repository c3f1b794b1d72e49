#!/usr/bin/env python3
"""usage: MI355X_H264_LIB=<a -DTURN_AB_COUNT build> turn_timeouts.py [bench.py arguments]
Runs bench.py in this process and prints what mi355x_h264_turn_timeouts() has counted over it (media_amd/csrc/engine.h): acquires of
the GPU's motion-search lock that ended by the time-out instead of by getting the lock, one JSON line.  0 is what a lock that is
always given back (k_tq.h tq_turn_release) shows.  Default arguments: two instances of 32 GOPs, two steps."""
import ctypes, json, os, runpy, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.argv = [os.path.join(ROOT, "bench.py")] + (sys.argv[1:] or "--steps 2 --warmup 1 --no-cpu-baseline".split())
runpy.run_path(sys.argv[0], run_name="__main__")
from media_amd import capi
out = ctypes.c_uint(0)
rc = capi.lib().mi355x_h264_turn_timeouts(ctypes.byref(out), 1)
print(json.dumps({"turn_timeouts": out.value if rc == 0 else None, "rc": rc}))
