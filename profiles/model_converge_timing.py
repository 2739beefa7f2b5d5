"""What per-model convergence (pyvb_lds_iterate_until_model, k_converge.hip) costs when nobody converges, what it saves once
models have, and what the stopping kernel and the totals kernel take per launch: DESIGN.md section 20.

    python profiles/model_converge_timing.py [--runs 5] [--steps 10] [--label LABEL] [--out FILE]
    python profiles/model_converge_timing.py --parent [--label parent_run1] [--out FILE]
    python profiles/model_converge_timing.py --trace                  (under rocprofv3 --kernel-trace --output-format csv)
    python profiles/model_converge_timing.py --summarise TRACE.csv [--out FILE]

The headline shape as in profiles/tied_timing.py (N = 1024 as 128 models of 8 chains, T = 10^4, D = K = 64; bench.py supplies the
inputs), one process, one GPU, `runs` runs of `steps` iterations per variant, the variants alternating inside every run.

 (a) nobody stops (tol = -inf): iterate_until_model on the tied handle against iterate on the same handle, and against
     iterate_until and iterate_until_model on a handle of singleton models.  --parent is the part of this that a build of the
     parent commit can run -- iterate on the tied handle -- for a copy of this script inside a built checkout of the parent (it
     imports the package it lies beside), run before and after the run of this commit: the parent's time and its own
     run-to-run spread.
 (b) about half of the models converged: a tol taken from the deltas of this batch itself (three single iterations give every
     model's delta twice; tol = the median delta extrapolated two iterations on by the ratio of the two medians), then
     iterate_until_model(2, tol), whose second iteration applies the test, and ms per iteration of both entries afterwards.
 (c) --trace: a short sequence for a kernel trace: eight iterations in which nothing stops, then every model but one is switched
     off and iterate_until_model(2, +inf) runs: the first iteration of a call stops nobody, the second stops the one model that
     runs, so the last launch of k_converge is the one in which a model of 8 chains freezes (in it the workgroups of the
     other models leave at their first instruction).  --summarise prints the durations of k_converge and k_elbo_sum from the trace.

A step that fails ends the run: nothing further is started on the GPU.
"""
import argparse
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

T, D, N, CHAINS = 10000, 64, 1024, 8
NEVER = -float("inf")


def summarise(path, say):
    import csv
    rows = sorted(csv.DictReader(open(path)), key=lambda r: int(r["Start_Timestamp"]))
    for kernel in ("k_converge", "k_elbo_sum"):         # (substrings: no other kernel of the library has either in its name)
        us = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in rows if kernel in r["Kernel_Name"]]
        if not us:
            say("%s: no launch in the trace" % kernel)
            continue
        us_sorted = sorted(us)
        say("%-20s %3d launches: median %8.2f us  min %8.2f  max %8.2f  last %8.2f"
            % (kernel, len(us), statistics.median(us), us_sorted[0], us_sorted[-1], us[-1]))
        say("  in order: " + " ".join("%.1f" % v for v in us))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--label", default="")
    ap.add_argument("--parent", action="store_true")
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--summarise")
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

    if args.summarise:
        summarise(args.summarise, say)
        return finish()

    import numpy as np
    from bench import make_inputs
    from pyvb_amd.lds import LDSBatch

    def timed(b, fn):
        t0 = time.perf_counter()
        fn(); b.sync()
        return (time.perf_counter() - t0) * 1e3 / args.steps

    def row(name, ms):
        say("%-44s median %8.3f ms  min %8.3f  max %8.3f  spread %6.3f   runs %s" % (
            args.label + name, statistics.median(ms), min(ms), max(ms), max(ms) - min(ms), " ".join("%.3f" % v for v in ms)))

    def model_tol(b, pick):
        """Three single iterations in which nothing stops: every model's delta twice, and a tol from pick(predicted deltas)."""
        llb = []
        for _ in range(3):
            assert b.iterate_until_model(1, NEVER) == 1
            llb.append(b.model_convergence()[2].copy())
        d1, d2 = llb[1] - llb[0], llb[2] - llb[1]
        return d1, d2, pick(d1, d2)

    Y, st0, pri = make_inputs(T, D, D, N, seed=20240)
    tied = LDSBatch.from_problem(Y, st0, pri, models=np.arange(N, dtype=np.int32) // CHAINS)
    tied.iterate(3); tied.sync()

    if args.parent:
        del Y
        row("tied_iterate", [timed(tied, lambda: tied.iterate(args.steps)) for _ in range(args.runs)])
        tied.close()
        return finish()

    if args.trace:
        del Y

        assert tied.iterate_until_model(8, NEVER) == 8
        only = np.zeros(N, dtype=bool)
        only[5 * CHAINS:6 * CHAINS] = True              # model 5 alone stays switched on ...
        tied.set_active(only)
        assert tied.iterate_until_model(2, float("inf")) == 2       # ... and any finite bound stops it in the second iteration
        conv = tied.model_convergence()[1]
        assert conv[5] and int(conv.sum()) == 1
        say("trace: 8 launches in which nothing stops, then model 5 alone switched on and iterate_until_model(2, +inf): its second "
            "launch freezes that one model of %d chains" % CHAINS)
        tied.close()
        return finish()

    single = LDSBatch.from_problem(Y, st0, pri, models=np.arange(N, dtype=np.int32))
    del Y
    single.iterate(3); single.sync()
    assert tied.iterate_until_model(2, NEVER) == 2 and single.iterate_until(2, NEVER) == 2 and single.iterate_until_model(2, NEVER) == 2
    # (a)
    variants = [("tied_iterate", tied, lambda: tied.iterate(args.steps)),
                ("tied_iterate_until_model_nobody_stops", tied, lambda: tied.iterate_until_model(args.steps, NEVER)),
                ("singletons_iterate_until_nobody_stops", single, lambda: single.iterate_until(args.steps, NEVER)),
                ("singletons_iterate_until_model_nobody_stops", single, lambda: single.iterate_until_model(args.steps, NEVER))]
    ms = {name: [] for name, _, _ in variants}
    for r in range(args.runs):
        k = r % len(variants)
        for name, b, fn in variants[k:] + variants[:k]:
            ms[name].append(timed(b, fn))
    for name, _, _ in variants:
        row(name, ms[name])
    med = {k: statistics.median(v) for k, v in ms.items()}
    say("tied: iterate_until_model - iterate = %+.3f ms per iteration;  singletons: iterate_until_model - iterate_until = %+.3f (medians)"
        % (med["tied_iterate_until_model_nobody_stops"] - med["tied_iterate"],
           med["singletons_iterate_until_model_nobody_stops"] - med["singletons_iterate_until_nobody_stops"]))
    assert not tied.model_convergence()[1].any() and not single.convergence()[1].any()
    single.close()
    # (b)
    def half(d1, d2):
        m1, m2 = float(np.median(d1)), float(np.median(d2))
        return m2 * (m2 / m1) ** 2 if m1 > 0 and m2 > 0 else m2
    d1, d2, tol = model_tol(tied, half)
    say("deltas of two single iterations: medians %.6g, %.6g; tol = %.6g" % (float(np.median(d1)), float(np.median(d2)), tol))
    tied.iterate_until_model(2, tol)
    conv = tied.model_convergence()[1]
    frozen = int(conv.sum())
    runs_of_frozen = int(np.count_nonzero(np.diff(conv.astype(int)) != 0)) + 1
    say("iterate_until_model(2, tol) froze %d of %d models (%d of %d chains), scattered over %d runs of consecutive models"
        % (frozen, N // CHAINS, frozen * CHAINS, N, runs_of_frozen))
    assert np.array_equal(tied.convergence()[1], np.repeat(conv, CHAINS))
    row("tied_iterate_%d_of_%d_models_converged" % (frozen, N // CHAINS), [timed(tied, lambda: tied.iterate(args.steps)) for _ in range(args.runs)])
    row("tied_iterate_until_model_%d_of_%d_converged" % (frozen, N // CHAINS),
        [timed(tied, lambda: tied.iterate_until_model(args.steps, NEVER)) for _ in range(args.runs)])
    assert int(tied.model_convergence()[1].sum()) == frozen
    tied.close()
    finish()


if __name__ == "__main__":
    main()
