"""Writes tests/golden/dec_loss_streams.json: the intra-refresh streams of tests/dec_loss.py, coded by the GPU encoder (the oracle
has no intra refresh).  Needs the device; run from the repository root:  python tests/golden/make_dec_loss_golden.py
The content is tests/intra_refresh.py's texture played BACKWARDS at 16 rows a picture: it moves DOWN by one macroblock row per
picture (the search range's limit), so that damage in a band reaches the bands below it before the refresh cycle has passed.
tests/test_dec_loss_oracle.py asserts what that buys: no case is exact again before the end of its cycle.  (At 3, 6 and 8 rows a
picture the n = 3 stream joined two pictures before a recovery point was exact one picture early; 12 and 16 rows hold for every
case.)  The loss pictures and flipped bits of tests/dec_loss.py were chosen for THIS content on the CPU; after regenerating, run
tests/test_dec_loss_oracle.py and tests/test_dec_loss_host.py."""
import base64
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import intra_refresh as ir          # noqa: E402
from media_amd import capi          # noqa: E402

STEP = 16
CASES = (ir.Case("ir3_64x96", 64, 96, 3, 66, 26, 14, 1, STEP, True), ir.Case("ir2_48x64", 48, 64, 2, 66, 26, 12, 1, STEP, True))


def main(path=os.path.join(HERE, "dec_loss_streams.json")):
    out = {}
    for c in CASES:
        enc = capi.Encoder(c.w, c.h, intra_refresh=True, qp=c.qp, gop=1000, profile_idc=c.prof, slices=c.n, search=c.search)
        aus, ks = [], []
        for f in ir.frames(c)[::-1]:
            bs, _ = enc.encode(f)
            aus.append(base64.b64encode(bytes(bs)).decode())
            ks.append(enc.last_refresh_band)
        enc.close()
        out[c.name] = {"case": list(c), "bands": ks, "aus": aus}
        print(c.name, ks, sum(len(a) for a in aus))
    with open(path, "w") as f:
        json.dump(out, f)


if __name__ == "__main__":
    main(*sys.argv[1:])
