"""Regenerate tests/golden/ref_libvig.npz: the answers of the reference's own
libVig (oracle/_ref, built by `make -C oracle ref` where the reference's
sources are present) to every seeded case of tests/oracle_cases.py. The
restatement is checked against them in tests/test_oracle.py.

    python tests/golden/make_ref_golden.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import oracle_cases as OC  # noqa: E402


def main():
    out = {}
    for name, (fn, plist) in OC.CASES.items():
        for params in plist:
            for i, a in enumerate(fn(True, *params)):
                out[OC.key(name, params, i)] = a
    np.savez_compressed(OC.FIXTURE, **out)
    print("%s: %d arrays, %d bytes" % (OC.FIXTURE, len(out), os.path.getsize(OC.FIXTURE)))


if __name__ == "__main__":
    main()
