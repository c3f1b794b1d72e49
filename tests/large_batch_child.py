"""The child process of tests/test_gpu_large_batch.py: MI355X_H264_INTRA_SLOTS and MI355X_H264_PINTRA_SLOTS are read once per
process, so the cases that need other values than the defaults run here, started fresh with the variables set.  Prints one
JSON line per case: {"case": name, "differences": [...]} (and, for the hub group, the sizes of its IDR steps); the parent asserts.

    python tests/large_batch_child.py direct <variant of large_batch.CHILD_VARIANTS>
    python tests/large_batch_child.py hub"""
import json
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


class Env:
    """what run_group needs of pytest's monkeypatch (this process ends with the case)"""

    def setenv(self, k, v):
        os.environ[k] = v


def main(argv):
    import torch
    torch.cuda.init()    # (torch's HIP runtime before the encoder library's, as tests/conftest.py does)
    import large_batch as lb
    if argv[0] == "direct":
        env, cases = lb.CHILD_VARIANTS[argv[1]]
        assert all(os.environ.get(k) == v for k, v in env.items()), "start this with %s set" % env
        for c in cases:
            try:
                bad = lb.run_direct(c)
            except Exception as ex:   # noqa: BLE001
                print(json.dumps({"case": c.name, "differences": ["%s: %s" % (type(ex).__name__, ex)]}), flush=True)
                return 1    # (nothing more is started on the GPU after an error)
            print(json.dumps({"case": c.name, "differences": bad}), flush=True)
        return 0
    assert argv[0] == "hub" and os.environ.get("MI355X_H264_INTRA_SLOTS") == str(lb.HUB_WALK_SLOTS)
    from test_gpu_stream_matrix import build_tick, run_group, steps_of
    with tempfile.TemporaryDirectory() as d:
        try:
            log = run_group(build_tick(d), Env(), lb.hub_group(lb.HUB_WALK_STREAMS))
            steps = steps_of(log)
        except Exception as ex:   # noqa: BLE001
            print(json.dumps({"case": "hub_walk", "differences": ["%s: %s" % (type(ex).__name__, ex)], "idr_steps": []}), flush=True)
            return 1
    print(json.dumps({"case": "hub_walk", "differences": [], "idr_steps": [len(p) for p in steps.values() if p[0][2]],
                      "p_steps": [len(p) for p in steps.values() if not p[0][2]]}), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
