#!/usr/bin/env python3
"""Generate the three short companions of lds_config1_d4k5_t200.npz by running the REFERENCE: the same shape (D = 4, K = 5),
noise kind, default priors and checkpoints, with T = 3, 19 and 60 and seeds of their own.  Together with the T = 200 fixture
they are the four chains of different lengths that tests/test_lengths_gpu.py puts on one handle; on their own they go
through the `golden`-parametrised tests like every other lds_*.npz.

Runs where make_golden.py runs (it needs the reference tree):

    python tests/golden/make_golden_lengths.py
"""
import os
import sys
import warnings

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_golden import load_reference, run_case

CASES = [
    # name, T, D, K, noise, checkpoints, seed, dense column covariances stored
    ("d4k5_t3", 3, 4, 5, "diagonal_gamma", (1, 2, 5), 20281, True),
    ("d4k5_t19", 19, 4, 5, "diagonal_gamma", (1, 2, 5), 20282, True),
    ("d4k5_t60", 60, 4, 5, "diagonal_gamma", (1, 2, 5), 20283, True),
]

if __name__ == "__main__":
    warnings.simplefilter("ignore", DeprecationWarning)
    ref = load_reference()
    for c in CASES:
        run_case(ref, *c)
