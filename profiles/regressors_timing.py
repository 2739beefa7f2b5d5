#!/usr/bin/env python3
"""What known regressors in the output equation cost on the fused LDS path (pyvb_lds_create_regressors, k_known.hip): time per
iteration at N = 1024 replicates of T = 10^4 steps for
    regressors  D = 32, K = 32, Pv = 8    the rows [y_t ; v_t] are 40 wide
    plain32     D = 32, K = 32            the same model without the regressors
    plain40     D = 32, K = 40            a plain handle that moves the bytes the handle with regressors moves
so plain40 -> regressors is what the new small kernels and the separate launches of C, E, R add.  The three handles are timed in turn,
three rounds each (alternating, so that a drift of the machine shows as spread, not as a difference), a host clock around `steps`
iterations that end in a synchronise, after a warm-up; then one more window per handle with the event timers on, for the time and the
launches per kernel (kernel_times; "regressors" is every kernel of k_known.hip together) and their share of the iteration.

    python profiles/regressors_timing.py [N] [T] [steps] > profiles/regressors_timing.txt
"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pyvb_amd import synth
from pyvb_amd.lds import LDSBatch

N = int(sys.argv[1]) if len(sys.argv) > 1 else 1024
T = int(sys.argv[2]) if len(sys.argv) > 2 else 10000
STEPS = int(sys.argv[3]) if len(sys.argv) > 3 else 20
DISTINCT = min(N, 32)          # distinct systems, tiled to N replicates (distinct data per system, as bench.py does)
ROUNDS, WARMUP = 3, 5


def tile(a):
    return np.ascontiguousarray(np.concatenate([a] * (N // DISTINCT))) if isinstance(a, np.ndarray) and a.ndim and a.shape[0] == DISTINCT else a


def make(kind):
    D, K, Pv = {"regressors": (32, 32, 8), "plain32": (32, 32, 0), "plain40": (32, 40, 0)}[kind]
    if Pv:
        Y, _, V, st0, pri = synth.make_regression_problem(T, D, K, 0, Pv, DISTINCT, seed=420)
        return LDSBatch.from_problem(tile(Y), {k: tile(v) for k, v in st0.items()}, pri, V=tile(V))
    Y, st0, pri = synth.make_problem(T, D, K, DISTINCT, seed=420)
    return LDSBatch.from_problem(tile(Y), {k: tile(v) for k, v in st0.items()}, pri)


def window(b, steps):
    b.sync()
    t0 = time.perf_counter()
    b.iterate(steps)
    b.sync()
    return (time.perf_counter() - t0) / steps * 1e3


def main():
    assert N % DISTINCT == 0
    kinds = ("regressors", "plain32", "plain40")
    handles = {k: make(k) for k in kinds}
    print("N = %d, T = %d, %d iterations per window, %d rounds, warm-up %d iterations" % (N, T, STEPS, ROUNDS, WARMUP))
    for b in handles.values():
        b.iterate(WARMUP)
        b.sync()
    ms = {k: [] for k in kinds}
    for _ in range(ROUNDS):
        for k in kinds:
            ms[k].append(window(handles[k], STEPS))
    for k in kinds:
        print("%-10s ms per iteration: %s   median %.4f" % (k, " ".join("%.4f" % v for v in ms[k]), float(np.median(ms[k]))))
    print("regressors - plain40 (median): %+.4f ms per iteration;  regressors - plain32: %+.4f" %
          (np.median(ms["regressors"]) - np.median(ms["plain40"]), np.median(ms["regressors"]) - np.median(ms["plain32"])))
    for k in kinds:
        b = handles[k]
        b.timing(True)
        b.iterate(STEPS)
        b.sync()
        kt = b.kernel_times()
        b.timing(False)
        # a sweep takes (T - 2) / 16 + J steps, J the warm-up k_prep chose for the replicate's recurrence: it depends on the fitted system
        w = b.get_warmup()
        print("%-10s warm-up steps J, median over the replicates: forward %d, backward %d (of %d steps per segment)" %
              (k, int(np.median(w[:, 0])), int(np.median(w[:, 1])), (T - 2 + 15) // 16))
        print("%-10s per iteration, ms (launches): %s" % (k, "  ".join("%s %.4f (%g)" % (nm, v[0] / STEPS, v[1] / STEPS) for nm, v in sorted(kt.items()) if v[1])))
        if "regressors" in kt:
            total = sum(v[0] for v in kt.values())
            print("%-10s the kernels of k_known.hip: %.4f ms of the %.4f ms the kernels of an iteration take, %.2f %%" %
                  (k, kt["regressors"][0] / STEPS, total / STEPS, 100.0 * kt["regressors"][0] / total))
        assert np.all(np.isfinite(b.elbo_history(1)))
        b.close()


if __name__ == "__main__":
    main()
