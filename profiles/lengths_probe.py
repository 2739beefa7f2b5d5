"""One handle with chain lengths against one handle per distinct length: DESIGN.md, "Per-replicate chain lengths".

    python profiles/lengths_probe.py [--runs 5] [--steps 50] [--out profiles/lengths_probe.txt]

256 series of the example's shape (D = 2, K = 5), lengths drawn once (seed 20240) uniformly from 50..200.
  (a) LDSBatch.from_series: one handle, T = the longest, every series with its own length;
  (b) what was possible before: the series grouped by length, one LDSBatch per distinct length, iterated in turn.
Both in one process on one GPU, alternating, `runs` timings of `steps` iterations each after a warm-up; the per-series lower
bounds of the two agree (printed).  The gate: the median of (a) does not exceed the median of (b).
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from pyvb_amd import synth
from pyvb_amd.lds import LDSBatch, pad_series

M, D, K = 256, 2, 5


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "lengths_probe.txt"))
    args = ap.parse_args()
    lengths = np.random.default_rng(20240).integers(50, 201, size=M)
    series = [(synth.simulate_lds(int(T), D, K, 1, seed=1000 + n)["Y"][0], synth.initial_state(int(T), D, K, 1, seed=5000 + n))
              for n, T in enumerate(lengths)]
    pri = synth.default_priors(D, K)
    one = LDSBatch.from_series(series, pri)
    groups = []                                         # (indices, handle) per distinct length
    for T in sorted(set(int(t) for t in lengths)):
        idx = [n for n in range(M) if lengths[n] == T]
        Y, st0, _ = pad_series([series[n] for n in idx])
        groups.append((idx, LDSBatch.from_problem(Y, st0, pri)))

    def run_one(steps):
        one.iterate(steps); one.sync()

    def run_groups(steps):
        for _ in range(steps):
            for _, h in groups:
                h.iterate(1)
        for _, h in groups:
            h.sync()

    run_one(3); run_groups(3)
    ta, tb = [], []
    for _ in range(args.runs):
        for fn, out in ((run_one, ta), (run_groups, tb)):
            t0 = time.perf_counter()
            fn(args.steps)
            out.append((time.perf_counter() - t0) * 1e3 / args.steps)
    ea = one.elbo().sum(1)
    eb = np.empty(M)
    for idx, h in groups:
        eb[idx] = h.elbo().sum(1)
    worst = float(np.max(np.abs(ea - eb) / np.abs(eb)))
    one.close()
    for _, h in groups:
        h.close()
    fmt = lambda v: " ".join("%.3f" % x for x in v)
    lines = [
        "%d series, D = %d, K = %d, lengths %d..%d (%d distinct), %d runs of %d iterations, ms per iteration over all series" % (
            M, D, K, lengths.min(), lengths.max(), len(groups), args.runs, args.steps),
        "(a) one handle with lengths, T = %d:                   median %.3f  min %.3f  max %.3f   runs %s" % (
            one.T, statistics.median(ta), min(ta), max(ta), fmt(ta)),
        "(b) one handle per distinct length (%d handles):     median %.3f  min %.3f  max %.3f   runs %s" % (
            len(groups), statistics.median(tb), min(tb), max(tb), fmt(tb)),
        "(b) / (a) = %.1f;  per-series lower bounds of (a) and (b) after %d iterations: worst relative difference %.2e" % (
            statistics.median(tb) / statistics.median(ta), 3 + args.runs * args.steps, worst),
    ]
    print("\n".join(lines))
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    if statistics.median(ta) > statistics.median(tb):
        raise SystemExit("one handle with lengths is slower than one handle per length")


if __name__ == "__main__":
    main()
