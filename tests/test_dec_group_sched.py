"""The part of a decoder group without HIP (media_amd/csrc/dec_group_sched.h: the pool's hand-out of parse jobs and the rotation of
the two sets of pinned buffers) under ThreadSanitizer: tools/dec_group_sched_harness.cpp."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "media_amd", "csrc")


def test_parse_pool_and_buffer_rotation_under_thread_sanitizer(tmp_path):
    """8 threads, 12 streams, 400 steps of random participation (every stream, one stream, a random subset; some steps launch
    nothing).  The harness aborts unless every job is parsed exactly once and by one thread at a time, and no buffer set is
    handed out or written while its uploads are marked in flight; ThreadSanitizer must report nothing."""
    assert shutil.which("g++"), "g++ is what this test is about"
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-x", "c++", os.path.join(CSRC, "dec_group_sched.h")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-1500:]   # plain C++: no ROCm include path
    exe = str(tmp_path / "dec_group_sched_tsan")
    r = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-pthread", "-fsanitize=thread", "-I", CSRC,
                        os.path.join(ROOT, "tools", "dec_group_sched_harness.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, "the ThreadSanitizer build failed: %s" % r.stderr[-1500:]
    for seed in ("1", "2"):
        r = subprocess.run([exe, "400", seed], capture_output=True, text=True, timeout=300,
                           env=dict(os.environ, TSAN_OPTIONS="halt_on_error=1 second_deadlock_stack=1"))
        assert r.returncode == 0 and r.stdout.startswith("ok "), (seed, r.stdout[-300:], r.stderr[-3000:])
        assert "WARNING: ThreadSanitizer" not in r.stderr, r.stderr[-3000:]
