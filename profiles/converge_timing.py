"""What per-replicate convergence (pyvb_lds_iterate_until) costs when nobody converges, and what it saves once rows have:
DESIGN.md section 18.

    python profiles/converge_timing.py [--runs 5] [--steps 10] [--out FILE]

One handle at the headline shape (N = 1024, T = 10^4, D = K = 64; bench.py supplies the inputs), one process, one GPU:

 (a) iterate(steps) against iterate_until(steps, tol = -1e300), `runs` runs of each, alternating.  With that tol nobody
     converges, so the difference is what the entry itself costs: the bound, the test and the totals on the main stream
     instead of beside the next iteration's k_prep and forward sweep.  Then the same with kernel timing on, once each, for
     k_elbo's own time (timing_get(PYVB_K_ELBO)): the overlap given up.
 (b) a tol that stops about half of the replicates, taken from the deltas of this batch itself: two single iterations give every
     replicate's delta twice, tol = the median delta extrapolated two iterations on by the ratio of the two medians.  Then
     iterate_until(2, tol) -- its second iteration applies the test -- and iterate(steps) again: ms per iteration with the
     converged rows frozen.  The number frozen is printed; compare profiles/active_mask_timing.txt (512 of 1024 rows switched off).

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
NEVER = -1e300


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--out")
    args = ap.parse_args()
    import numpy as np
    from bench import make_inputs
    from pyvb_amd.lds import LDSBatch
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    def timed(fn):
        t0 = time.perf_counter()
        fn(); b.sync()
        return (time.perf_counter() - t0) * 1e3 / args.steps

    def row(name, ms):
        say("%-34s median %8.3f ms  min %8.3f  max %8.3f  spread %6.3f   runs %s" % (
            name, statistics.median(ms), min(ms), max(ms), max(ms) - min(ms), " ".join("%.3f" % v for v in ms)))

    Y, st0, pri = make_inputs(T, D, D, N, seed=20240)
    b = LDSBatch.from_problem(Y, st0, pri)
    del Y
    b.iterate(3); b.sync()
    assert b.iterate_until(2, NEVER) == 2
    # (a)
    plain, until = [], []
    for _ in range(args.runs):
        plain.append(timed(lambda: b.iterate(args.steps)))
        until.append(timed(lambda: b.iterate_until(args.steps, NEVER)))
    row("iterate", plain)
    row("iterate_until_nobody_converges", until)
    say("extra cost of iterate_until: %.3f ms per iteration (medians)" % (statistics.median(until) - statistics.median(plain)))
    for name, fn in (("iterate", lambda: b.iterate(args.steps)), ("iterate_until", lambda: b.iterate_until(args.steps, NEVER))):
        b.timing(True)
        fn(); b.sync()
        kt = b.kernel_times()
        b.timing(False)
        say("kernel times inside %-14s " % name + "  ".join("%s %.3f ms x %d" % (k, v[0] / max(v[1], 1), v[1]) for k, v in sorted(kt.items()) if v[1]))
    assert not b.convergence()[1].any()
    # (b)
    llb = []
    for _ in range(3):
        b.iterate_until(1, NEVER)
        llb.append(b.convergence()[2].copy())
    d1, d2 = llb[1] - llb[0], llb[2] - llb[1]
    m1, m2 = float(np.median(d1)), float(np.median(d2))
    tol = m2 * (m2 / m1) ** 2 if m1 > 0 and m2 > 0 else m2
    say("deltas of two single iterations: medians %.6g, %.6g; tol = %.6g" % (m1, m2, tol))
    b.iterate_until(2, tol)
    frozen = int(b.convergence()[1].sum())
    say("iterate_until(2, tol) froze %d of %d replicates" % (frozen, N))
    after = [timed(lambda: b.iterate(args.steps)) for _ in range(args.runs)]
    row("iterate_%d_of_%d_converged" % (frozen, N), after)
    until_after = [timed(lambda: b.iterate_until(args.steps, NEVER)) for _ in range(args.runs)]
    row("iterate_until_%d_of_%d_converged" % (frozen, N), until_after)
    assert int(b.convergence()[1].sum()) == frozen
    b.close()
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
