"""Writes tests/golden/svm_tight.npz: scikit-learn's decision values at tol = 1e-6 for those problems of tests/_svm_ref.py whose
tight fit is too slow for a test (libsvm needs minutes at 1e-6 on the 1024-row linear problem: 24 features, an ill-conditioned Gram).
The tests compute every other tight fit themselves; `dd_ref` = |SVC(tol 1e-3) - SVC(tol 1e-6)| is formed in the test either way.
Run from the repository root: python tests/golden/make_golden_svm.py"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import _svm_ref as R  # noqa: E402

SLOW = 2.0  # seconds

if __name__ == "__main__":
    out = {}
    for ci, case in enumerate(R.CASES):
        x, y, train, val = R.make_case(*case)
        for swapped, (tr, va) in enumerate(((train, val), (val, train))):
            for name in sorted(R.PARAMS):
                t = time.time()
                _, dec, _ = R.sk_decision(x, y, tr, va, name, tol=1e-6)
                dt = time.time() - t
                if dt > SLOW:
                    out[R.tight_key(ci, name, swapped)] = dec
                    print(f"case {ci} {name} swapped {swapped}: {dt:.1f} s, recorded {dec.shape}", flush=True)
    np.savez_compressed(os.path.join(os.path.dirname(os.path.abspath(__file__)), "svm_tight.npz"), **out)
