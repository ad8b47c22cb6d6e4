"""Generates tests/golden/transfer_reference.npz: the float64 transfer-learning reference of every case of
transfer_reference.CASES, as transfer_reference.golden_record keeps it (the four metrics, their scales, per parameter
tensor ||g|| and g . u) -- scalars only, no gradients.  test_transfer_learn.test_reference_matches_golden holds
transfer_ref to it.  Re-run only when the case table changes on purpose:
python tests/golden/make_transfer_reference_golden.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
ROOT = os.path.dirname(TESTS)
for p in (TESTS, ROOT, os.path.join(ROOT, "reinforcement-learning_amd")):
    sys.path.insert(0, p)
import transfer_reference as tr  # noqa: E402


def main():
    out = {}
    for name in tr.CASES:
        for k, v in tr.golden_record(tr.build_transfer_case(name)).items():
            out[f"{name}:{k}"] = np.asarray(v, np.float64)
    np.savez(tr.GOLDEN, **out)
    print(f"{tr.GOLDEN}: {len(out)} arrays of {len(tr.CASES)} cases")


if __name__ == "__main__":
    main()
