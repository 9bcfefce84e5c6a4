"""tests/golden/state_messages.json: the return code and the exact
vp_last_error() text of every refused image and delta the suites build
(tests/statecases.py mutations, tests/deltacases.py mutations), read from the
library on a GPU. The texts are part of the interface: record them from the
commit whose messages are to be kept, then the GPU suites and
tests/test_state_reader.py compare against them.

  python3 tests/golden/make_state_messages.py [--out FILE]
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import deltacases as DC  # noqa: E402
import deltaref as DR  # noqa: E402
import statecases as SC  # noqa: E402
import stateref as SR  # noqa: E402
from gpuh import check_batches  # noqa: E402
from test_state_delta_gpu import MARK, standby  # noqa: E402
from test_state_gpu import make_pair  # noqa: E402


def refusal(nf, call, blob, img):
    buf = np.frombuffer(blob, np.uint8)
    rc = call(nf.h, C.c_void_p(buf.ctypes.data), buf.size)
    text = nf.L.vp_last_error().decode()
    assert rc != 0 and nf.save_state() == img, (rc, text)
    return [rc, text]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(HERE, "state_messages.json"))
    out = ap.parse_args().out
    rec = {"image": {}, "image_small": {}, "delta": {}}
    for kind in ("nat", "lb"):
        tr, cut = SC.trace(kind, "part")
        nf, o = make_pair(kind, **SC.pair_args(kind, "part"))
        check_batches(nf, o, tr[0][:cut * 64], tr[1][:cut], tr[2][:cut], tr[3][:cut], 64, [])
        img = nf.save_state()
        muts = SC.mutations(kind, img)
        rec["image"][kind] = {m: refusal(nf, nf.L.vp_state_load, muts[m], img)
                              for m in SC.names_for(kind)}
        small = SR.pack(SC.small_state(kind))
        muts = SC.mutations(kind, small)
        rec["image_small"][kind] = {m: refusal(nf, nf.L.vp_state_load, muts[m], img)
                                    for m in SC.HEADER_LEVEL if m in muts}
    for kind in ("fw", "lb"):
        s0, s1, touched = DC.victim(kind, cap=SC.CAP, bcap=SC.LB_BCAP)
        good = DR.diff(s0, s1, touched, base=MARK, mark=(MARK[0] + 40, MARK[1]))
        nf = standby(kind, SR.pack(s0), MARK, **SC.pair_args(kind))
        muts = DC.mutations(s0, good)
        rec["delta"][kind] = {m: refusal(nf, nf.L.vp_state_delta_apply, muts[m], SR.pack(s0))
                              for m in DC.names_for(kind)}
    with open(out, "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)
        f.write("\n")
    print("%s: %d texts" % (out, sum(len(k) for g in rec.values() for k in g.values())))


if __name__ == "__main__":
    main()
