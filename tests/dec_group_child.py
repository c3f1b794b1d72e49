"""The child process of tests/test_gpu_dec_group.py: MI355X_H264_DEC_SYNC and the group's slot variables are read once per
process or group, so the runs that need them set start fresh here.  Prints one JSON line {"case": name, "differences": [...]}.

    python tests/dec_group_child.py <case name of tests/dec_group.py>"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main(argv):
    import torch
    torch.cuda.init()    # (torch's HIP runtime before the decoder library's, as tests/conftest.py does)
    import dec_group as dg
    from test_gpu_dec_group import run_case
    try:
        bad = run_case(dg.BY_NAME[argv[0]], singles=False)
    except Exception as ex:   # noqa: BLE001
        print(json.dumps({"case": argv[0], "differences": ["%s: %s" % (type(ex).__name__, ex)]}), flush=True)
        return 1
    print(json.dumps({"case": argv[0], "differences": bad}), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
