"""What DiagonalGamma precision parents for the columns of A and C (pyvb_lds_set_entry_precisions, k_ard.hip: k_entry) cost:
DESIGN.md section 23.

    python profiles/entry_timing.py [--runs 5] [--steps 10] [--label LABEL] [--out FILE]
    python profiles/entry_timing.py --parent [--label parent_run1] [--out FILE]

The headline shape (N = 1024, T = 10^4, D = K = 64; bench.py supplies the inputs), one process, one GPU, `runs` runs of `steps`
iterations per variant, the variants alternating inside every run.

 (a) pyvb_lds_iterate on a plain handle and on a handle with Gamma parents on both matrices: k_elbo's column() has one more uniform
     test, ParamArgs is larger.  --parent is the same measurement for a copy of this script inside a built checkout of the parent
     commit (it imports the package it lies beside), run before and after the run of this commit: the parent's times and its own
     run-to-run spread are the yardstick.
 (b) the same handle with DiagonalGamma parents on both matrices: one more launch per iteration, k_entry over (N, 2) workgroups of four wavefronts.
 (c) the precision update alone, update_entry_precisions("A") then ("C") = one launch per matrix, `steps` times, asynchronous, one
     sync at the end: what k_entry takes, and the bytes it moves per second.  Per matrix it reads M and V [N][D][rows] and writes qb
     and the expectations [N][D][rows]; the six [D][rows] prior arrays and the prior means are shared by the replicates.

A step that fails ends the run: nothing further is started on the GPU.
"""
import argparse
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

T, D, N = 10000, 64, 1024


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--label", default="")
    ap.add_argument("--parent", action="store_true")
    ap.add_argument("--out")
    args = ap.parse_args()
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    def finish():
        if args.out:
            with open(args.out, "a") as f:
                f.write("\n".join(lines) + "\n")

    import numpy as np
    from bench import make_inputs
    from pyvb_amd.lds import LDSBatch

    def timed(b, fn, per):
        t0 = time.perf_counter()
        fn(); b.sync()
        return (time.perf_counter() - t0) * 1e3 / per

    def row(name, ms):
        say("%-40s median %8.3f ms  min %8.3f  max %8.3f  spread %6.3f   runs %s" % (
            args.label + name, statistics.median(ms), min(ms), max(ms), max(ms) - min(ms), " ".join("%.3f" % v for v in ms)))

    rng = np.random.default_rng(7)
    Y, st0, pri = make_inputs(T, D, D, N, seed=20240)
    plain = LDSBatch.from_problem(Y, st0, pri)
    gamma = LDSBatch.from_problem(Y, st0, pri)
    prior = (np.full(D, 1e-3), np.full(D, 1e-3), 0.5 + rng.random((N, D)))
    gamma.set_column_precisions(A=prior, C=prior)
    variants = [("plain_iterate", plain, lambda: plain.iterate(args.steps)),
                ("gamma_parents_on_A_and_C_iterate", gamma, lambda: gamma.iterate(args.steps))]
    entry = None
    if not args.parent:
        entry = LDSBatch.from_problem(Y, st0, pri)
        each = (np.full((D, D), 1e-3), np.full((D, D), 1e-3), 0.5 + rng.random((N, D, D)))
        entry.set_entry_precisions(A=each, C=each)
        variants.append(("entry_parents_on_A_and_C_iterate", entry, lambda: entry.iterate(args.steps)))
    del Y
    for _, b, _ in variants:
        b.iterate(3); b.sync()
    ms = {name: [] for name, _, _ in variants}
    for r in range(args.runs):
        k = r % len(variants)
        for name, b, fn in variants[k:] + variants[:k]:
            ms[name].append(timed(b, fn, args.steps))
    for name, _, _ in variants:
        row(name, ms[name])
    if entry is not None:
        med = {k: statistics.median(v) for k, v in ms.items()}
        say("entry parents - plain = %+.3f ms per iteration (medians)" % (med["entry_parents_on_A_and_C_iterate"] - med["plain_iterate"]))

        def update_only():
            for _ in range(args.steps):         # (explicitly per matrix: nothing is read back between the launches)
                entry.update_entry_precisions("A")
                entry.update_entry_precisions("C")
        update_only(); entry.sync()
        a = [timed(entry, update_only, args.steps) for _ in range(args.runs)]
        row("entry_A_then_entry_C_two_launches", a)
        nbytes = 8.0 * (2 * N * 4 * D * D + 2 * 6 * D * D + 2 * D * D + 2 * 3 * N * D)
        say("k_entry moves %.1f MB per pair of launches (M, V read and qb, qa / qb written, [N][D][rows] each, for both matrices; the "
            "shared priors; 3 [N][D] sums per matrix): %.1f GB/s at the median (wall time of %d asynchronous calls and one sync, so "
            "the launch overhead of two calls per pair is inside)" % (nbytes / 1e6, nbytes / (statistics.median(a) * 1e-3) / 1e9, 2 * args.steps))
    for _, b, _ in variants:
        b.close()
    finish()


if __name__ == "__main__":
    main()
