"""The guard mode of the library's own memory (media_amd/csrc/dev_mem.h; include/mi355x_h264.h, mi355x_h264_debug_mem_guard) as far
as it needs no device: the checker itself, with its HIP calls bound to malloc / memcpy, under AddressSanitizer + UBSan as a program
of its own (tools/dev_mem_harness.cpp), the exports, what the process-wide switch refuses, and the refusal of every new call on a
null handle.  What the guards see on the GPU: tests/test_gpu_mem_guard.py."""
import ctypes as C
import os
import subprocess

from media_amd import capi, h264dec

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "media_amd", "csrc")
NAMES = ("mi355x_h264_debug_mem_guard", "mi355x_h264_debug_mem_guard_get", "mi355x_h264_debug_mem_tally", "mi355x_h264_debug_mem_check",
         "mi355x_h264_debug_mem_poke", "mi355x_h264_stream_debug_mem_check", "mi355x_h264_dec_debug_mem_check",
         "mi355x_h264_dec_group_debug_mem_check", "mi355x_h264_dec_group_debug_mem_poke")


def test_the_checker_under_address_and_ub_sanitizer(tmp_path):
    """blocks of 1, 4, 4095, 4096 and 1 MiB + 3 bytes, guards of 4096 and 262144 bytes, poisoned and not: the harness aborts unless
    pointers, fills, totals, the clean check, every reported offset, the refusals of the poke, the tally of drop / free_all and
    the allocation sizes with the switch off are what dev_mem.h states; the sanitizers must report nothing"""
    exe = str(tmp_path / "dev_mem_harness")
    r = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I", CSRC,
                        os.path.join(ROOT, "tools", "dev_mem_harness.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, "the build failed: %s" % r.stderr[-2000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1")
    for k in ("MI355X_H264_MEM_GUARD", "MI355X_H264_MEM_POISON", "MI355X_H264_MEM_GUARD_LOG"):
        env.pop(k, None)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0 and r.stdout.startswith("ok dev_mem"), (r.stdout[-300:], r.stderr[-3000:])
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]


def test_the_exports_exist_and_the_abi_version_stands():
    syms = subprocess.run(["nm", "-D", "--defined-only", capi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for n in NAMES:
        assert n in capi.EXPORTS and " T %s\n" % n in syms, n
    assert capi.lib().mi355x_h264_abi_version() == 3   # functions were added, nothing changed


def test_the_switch_refuses_bad_sizes_and_changes_nothing_then():
    L = capi.lib()
    was = capi.mem_guard_get()
    try:
        capi.mem_guard(8192, True)
        for bad in (1, 4095, 4097, 6000, -4096, (1 << 20) + 4096, 1 << 21, 1 << 40):
            assert L.mi355x_h264_debug_mem_guard(bad, 0) == capi.E_ARG, bad
            assert capi.mem_guard_get() == (8192, True), bad
        assert capi.mem_guard(1 << 20, False) == (8192, True) and capi.mem_guard_get() == (1 << 20, False)
        assert capi.mem_guard(4096, True) == (1 << 20, False)
        capi.mem_guard(0, True)
        assert capi.mem_guard_get() == (0, False)   # poison without guards is no mode
        assert L.mi355x_h264_debug_mem_guard_get(None, None) == 0
    finally:
        capi.mem_guard(*was)
    assert capi.mem_guard_get() == was


def test_the_tally_reads_and_resets_without_a_device():
    assert capi.mem_tally() == 0 and capi.mem_tally(reset=True) == 0 and capi.mem_tally() == 0


def test_null_handles_are_refused():
    L = capi.lib()
    h264dec._bind()
    regions, buf = C.c_int(7), C.create_string_buffer(64)
    for name in ("mi355x_h264_debug_mem_check", "mi355x_h264_stream_debug_mem_check", "mi355x_h264_dec_debug_mem_check",
                 "mi355x_h264_dec_group_debug_mem_check"):
        assert getattr(L, name)(None, C.byref(regions), buf, len(buf)) == capi.E_ARG, name
        assert getattr(L, name)(None, None, None, 0) == capi.E_ARG, name
    for name in ("mi355x_h264_debug_mem_poke", "mi355x_h264_dec_group_debug_mem_poke"):
        assert getattr(L, name)(None, b"d_mb", -1, 0) == capi.E_ARG, name
        assert getattr(L, name)(None, None, 0, 0) == capi.E_ARG, name
