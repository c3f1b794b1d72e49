"""Lockstep steps of 25 to 64 pictures against the oracle - run with -m gpu on an MI355X.

The case list is tests/large_batch.py (tests/test_large_batch_oracle.py proves its coverage on the oracle).  These are the
step sizes the published throughput comes from (two engines of 32 closed GOPs; MAX_BATCH = 64; stream hubs of up to 64 streams),
where k_intra_rows walks from picture y to pictures y + 24 and y + 48 and batch items and grid positions 16 .. 63 of every other
kernel are in use.

Direct steps (capi.Encoder(batch = G), encode_gops_device), two calls or three: every GOP of every item equals the oracle's
serial stream byte for byte, sizes[] and the per-item scene-change statistic agree, and mi355x_h264_stats holds what the case's
geometry and the oracle's decisions say (large_batch.expected_stats).  The direct API reads the stages of item 0 only; they are
compared after every call.  Of items 1 and up, every picture's bytes are checked, and with them the loop-filtered planes of all
but the last picture of each GOP (the next P picture is predicted from them).  NOT observable on this path: the loop filter's
output for the LAST picture of the GOPs of items 1 and up.  The hub tests below read the pre-filter and the final planes of
every item after every picture.

Other slot counts (MI355X_H264_INTRA_SLOTS, MI355X_H264_PINTRA_SLOTS: read once per process) run in a fresh child process each,
tests/large_batch_child.py, one at a time and under a time limit."""
import json
import os
import subprocess
import sys
import pytest
import large_batch as lb
from test_gpu_parity import _compare_all
from test_gpu_stream_matrix import run_group, steps_of, tick   # noqa: F401  (tick: the fixture)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD_TIMEOUT_S = 120


def _direct(c):
    def item0(enc, call, stages):
        _compare_all(enc, stages, "%s call %d item 0, last picture" % (c.name, call))

    bad = lb.run_direct(c, after_call=item0)
    assert not bad, "%s: %d differences, the first: %s" % (c.name, len(bad), bad[:8])


@pytest.mark.parametrize("c", [c for c in lb.DIRECT_CASES if c.name != "slices_32"], ids=lambda c: c.name)
def test_large_step_equals_the_oracle(c):
    """64 Baseline items (24 + 24 + 16), 40 High items (24 + 16), 25 Main items with two reference pictures (24 + 1); the sparse
    and the dense variant of the schedule switch (picture-walking k_i4_decide / k_pintra_rows / bS 4 filter launches, and all
    pictures resident from the second call on): bytes, sizes[], me_cost per item, the stages of item 0, the statistics"""
    _direct(c)


@pytest.mark.parametrize("setting", [None, "0"])
def test_large_step_with_slices_and_both_loop_filter_forms(monkeypatch, setting):
    """32 items of three slices at 176x144 (k_bit_scan / k_pack grids of 96 workgroups, access units put together from three
    payloads per item), under the default MI355X_H264_PAIR_FILTER and with the two-rows-per-wave form switched off"""
    if setting is not None:
        monkeypatch.setenv("MI355X_H264_PAIR_FILTER", setting)
    _direct(lb.by_name("slices_32"))


def _child(args, env):
    """one fresh child process with `env` set, under a time limit; returns its JSON lines.  A child that times out or dies
    fails the test there and then"""
    e = dict(os.environ)
    e.update(env)
    try:
        r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "large_batch_child.py")] + args, env=e, capture_output=True, text=True, timeout=CHILD_TIMEOUT_S)
    except subprocess.TimeoutExpired as ex:
        pytest.fail("the child process %s did not finish in %d s; its output: %s" % (args, CHILD_TIMEOUT_S, ex.stdout))
    lines = [json.loads(line) for line in r.stdout.splitlines() if line.startswith("{")]
    print(r.stdout)
    assert r.returncode == 0, "the child process %s ended with %d: %s\n%s" % (args, r.returncode, lines, r.stderr[-2000:])
    return lines


@pytest.mark.parametrize("variant", sorted(lb.CHILD_VARIANTS))
def test_other_slot_counts_in_a_fresh_process(variant):
    """MI355X_H264_INTRA_SLOTS = 3 with 8 (3 + 3 + 2) and 7 (3 + 3 + 1) items, Baseline and High; MI355X_H264_INTRA_SLOTS = 1 with
    4 items (every picture but the first is walked to) together with MI355X_H264_PINTRA_SLOTS = 3 on 8 items of the dense content (a
    grid between 1 and G, which the default rule never picks: k_i4_decide and k_pintra_rows must agree on which pictures a workgroup
    takes).  Every item's bytes, sizes and statistics against the oracle, as in the direct tests"""
    env, cases = lb.CHILD_VARIANTS[variant]
    lines = _child(["direct", variant], env)
    assert [ln["case"] for ln in lines] == [c.name for c in cases], "the child did not report every case"
    for ln in lines:
        assert not ln["differences"], "%s: %s" % (ln["case"], ln["differences"][:8])


def test_hub_idr_step_walks_in_a_fresh_process():
    """k_intra_rows<true> walking: twelve streams under MI355X_H264_INTRA_SLOTS = 2.  The first stream to arrive leads an IDR step
    alone, the next step takes what queued meanwhile; the run must hold an IDR step of more pictures than slots whose size is no
    multiple of the slot count (a run in which none occurred fails), every picture compared stage by stage"""
    (ln,) = _child(["hub"], {"MI355X_H264_INTRA_SLOTS": str(lb.HUB_WALK_SLOTS)})
    assert not ln["differences"], ln["differences"]
    print("IDR step sizes %s, P step sizes %s" % (ln["idr_steps"], ln["p_steps"]))
    assert any(n > lb.HUB_WALK_SLOTS and n % lb.HUB_WALK_SLOTS for n in ln["idr_steps"]), \
        "no IDR step of more than %d pictures and of a size that is no multiple of it: %s" % (lb.HUB_WALK_SLOTS, ln["idr_steps"])


@pytest.mark.parametrize("group", sorted(lb.HUB_GROUPS))
def test_hub_groups_of_48_and_64_streams(tick, monkeypatch, group):   # noqa: F811
    """one engine of 48 streams (High, NV12 read in place from device memory) and one of 64 (Baseline), a QP of its own per
    stream, six pictures of GOP 3: every stream after every picture against its oracle, stage by stage - the path that reads
    the pre-filter and final planes of EVERY batch item"""
    monkeypatch.setenv("MI355X_H264_HUB_ITEMS", str(lb.HUB_ITEMS))
    specs = lb.HUB_GROUPS[group]()
    seen = {}

    def check(r, i, au, idr, tag):
        if i == lb.HUB_PICTURES - 1:
            seen[r.k] = r.stream.hub_stats()

    log = run_group(tick, monkeypatch, specs, per_picture=check)
    steps = steps_of(log)
    sizes = {True: sorted(len(p) for p in steps.values() if p[0][2]), False: sorted(len(p) for p in steps.values() if not p[0][2])}
    print("%s: IDR step sizes %s (largest %d), P step sizes %s" % (group, sizes[True], sizes[True][-1], sizes[False]))
    assert len(log) == len(specs) * lb.HUB_PICTURES and {k for k, *_ in log} == set(range(len(specs))), "every picture of every stream was coded and compared"
    stats = seen[len(specs) - 1]
    assert stats["open_streams"] == len(specs) > 32, "batch items of 32 and more were open on ONE engine: %s" % stats
    assert stats["pictures"] == len(log) and stats["steps"] == len(steps), stats
    assert stats["max_batch"] == max(len(p) for p in steps.values()), "max_batch %d, the log's largest step %d" % (stats["max_batch"], max(len(p) for p in steps.values()))
    assert any(not pics[0][2] and max(p[0] for p in pics) >= 24 and len(pics) >= 2 for pics in steps.values()), "no P step carried pictures of items of 24 and more"
    assert any(pics[0][2] and max(p[0] for p in pics) >= 32 for pics in steps.values()), "no IDR step carried an item of 32 or more"
