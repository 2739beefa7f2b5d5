"""What Gamma precision parents for the columns of A and C (pyvb_lds_set_column_precisions, k_ard.hip) cost: DESIGN.md section 21.

    python profiles/ard_timing.py [--runs 5] [--steps 10] [--label LABEL] [--out FILE]
    python profiles/ard_timing.py --parent [--label parent_run1] [--out FILE]

The headline shape (N = 1024, T = 10^4, D = K = 64; bench.py supplies the inputs), one process, one GPU, `runs` runs of `steps`
iterations per variant, the variants alternating inside every run.

 (a) pyvb_lds_iterate on a plain handle: k_cols and k_elbo read the column priors through the strided view of params.h.  --parent
     is the same measurement for a copy of this script inside a built checkout of the parent commit (it imports the package it lies
     beside), run before and after the run of this commit: the parent's time and its own run-to-run spread are the yardstick.
 (b) the same handle with hyperpriors on both matrices: one more launch per iteration, k_ard over (N, 2) wavefronts.
 (c) the alpha update alone, update_column_precisions("A") then ("C") = one launch per matrix, `steps` times, asynchronous, one
     sync at the end: what k_ard takes, and the bytes it moves per second.  It reads M and V of both matrices and the prior means, and writes four [N][D] arrays per matrix.

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
        say("%-36s median %8.3f ms  min %8.3f  max %8.3f  spread %6.3f   runs %s" % (
            args.label + name, statistics.median(ms), min(ms), max(ms), max(ms) - min(ms), " ".join("%.3f" % v for v in ms)))

    Y, st0, pri = make_inputs(T, D, D, N, seed=20240)
    plain = LDSBatch.from_problem(Y, st0, pri)
    plain.iterate(3); plain.sync()
    if args.parent:
        del Y
        row("plain_iterate", [timed(plain, lambda: plain.iterate(args.steps), args.steps) for _ in range(args.runs)])
        plain.close()
        return finish()

    rng = np.random.default_rng(7)
    ard = LDSBatch.from_problem(Y, st0, pri)
    del Y
    prior = (np.full(D, 1e-3), np.full(D, 1e-3), 0.5 + rng.random((N, D)))
    ard.set_column_precisions(A=prior, C=prior)
    ard.iterate(3); ard.sync()
    variants = [("plain_iterate", plain, lambda: plain.iterate(args.steps)),
                ("hyperpriors_on_A_and_C_iterate", ard, lambda: ard.iterate(args.steps))]
    ms = {name: [] for name, _, _ in variants}
    for r in range(args.runs):
        k = r % len(variants)
        for name, b, fn in variants[k:] + variants[:k]:
            ms[name].append(timed(b, fn, args.steps))
    for name, _, _ in variants:
        row(name, ms[name])
    med = {k: statistics.median(v) for k, v in ms.items()}
    say("hyperpriors - plain = %+.3f ms per iteration (medians)" % (med["hyperpriors_on_A_and_C_iterate"] - med["plain_iterate"]))

    def alpha_only():
        for _ in range(args.steps):         # (explicitly per matrix: nothing is read back between the launches)
            ard.update_column_precisions("A")
            ard.update_column_precisions("C")
    alpha_only(); ard.sync()
    a = [timed(ard, alpha_only, args.steps) for _ in range(args.runs)]
    row("alpha_A_then_alpha_C_two_launches", a)
    nbytes = 8.0 * (N * (2 * D * D + 2 * D * D) + 2 * D * D + 2 * 4 * N * D + 2 * 3 * D)
    say("k_ard moves %.1f MB per pair of launches (M and V of both matrices, the prior means, 4 [N][D] arrays per matrix written): "
        "%.1f GB/s at the median (wall time of %d asynchronous calls and one sync, so the launch overhead of two calls per pair is inside)" % (nbytes / 1e6, nbytes / (statistics.median(a) * 1e-3) / 1e9, 2 * args.steps))
    plain.close(); ard.close()
    finish()


if __name__ == "__main__":
    main()
