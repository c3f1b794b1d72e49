"""The stream hub's scheduling (media_amd/csrc/hub_sched.h: queues, step contexts, leader / followers) without HIP, under
ThreadSanitizer and under AddressSanitizer + UBSan: tools/hub_sched_harness.cpp."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "media_amd", "csrc")


def test_hub_scheduler_under_sanitizers(tmp_path):
    """64 threads open streams on one scheduler, hand in pictures, force IDR pictures (their own and each other's), change QPs
    and close, against a step that sleeps briefly and fails now and then.  The harness aborts unless every picture handed in is
    run exactly once and in its stream's order, a step holds pictures of one type and (P steps) at most the share, the picture
    after a failed one is an IDR picture, and the close of the last stream returns with no step context busy; the sanitizers
    must report nothing (a report makes the run fail: halt_on_error)."""
    if not shutil.which("g++"):
        pytest.skip("no g++")
    for name in ("host_framing.h", "hub_sched.h"):   # plain C++: a host compiler takes them with no ROCm include path
        r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-x", "c++", os.path.join(CSRC, name)],
                           capture_output=True, text=True)
        assert r.returncode == 0, (name, r.stderr[-1500:])
    ran = 0
    for san, rounds, env in (("thread", "30", {"TSAN_OPTIONS": "halt_on_error=1 second_deadlock_stack=1"}),
                             ("address,undefined", "30", {"ASAN_OPTIONS": "detect_leaks=1", "UBSAN_OPTIONS": "halt_on_error=1"})):
        exe = str(tmp_path / ("hub_sched_" + san.split(",")[0]))
        r = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-pthread", "-fsanitize=" + san, "-fno-sanitize-recover=undefined", "-I", CSRC,
                            os.path.join(ROOT, "tools", "hub_sched_harness.cpp"), "-o", exe], capture_output=True, text=True)
        if r.returncode != 0 and san == "address,undefined":
            continue   # (as for the parser: that runtime may be missing; ThreadSanitizer, the point of this test, may not)
        assert r.returncode == 0, "the %s build failed: %s" % (san, r.stderr[-1500:])
        for seed in ("1", "2"):
            r = subprocess.run([exe, rounds, seed], capture_output=True, text=True, timeout=300, env=dict(os.environ, **env))
            assert r.returncode == 0 and r.stdout.startswith("ok "), (san, seed, r.stdout[-300:], r.stderr[-3000:])
            assert "WARNING: ThreadSanitizer" not in r.stderr and "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
        ran += 1
    assert ran >= 1
