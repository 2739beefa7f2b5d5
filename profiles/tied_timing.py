"""What sharing A, C, Q, R between chains (pyvb_lds_create_tied, k_tie.hip) costs per iteration, and that handles without tied
models cost what they did: DESIGN.md section 19.

    python profiles/tied_timing.py [--runs 6] [--steps 10] [--handles plain,singletons,tied_128x8] [--label LABEL] [--out FILE]

The headline shape (N = 1024, T = 10^4, D = K = 64; bench.py supplies the inputs), one process, one GPU.  Three handles on the
same inputs, `runs` runs of `steps` iterations each, the handles alternating inside every run and the order rotating from run to
run (a handle's place in the order is worth a few hundredths of a millisecond: the first window after another handle's sync):

    plain       LDSBatch.from_problem(Y, st0, pri)                                   pyvb_lds_create
    singletons  ... models = 0 .. N-1                                                pyvb_lds_create_tied, no model tied
    tied        ... models = 128 models of 8 chains                                  k_tie runs after k_moments

Then one pass of each with kernel timing on, and one of a plain handle of N / 8 = 128 replicates (the first of every model):
what k_prep and k_cols would take if they ran once per model instead of once per chain.  k_tie is timed under PYVB_K_PARAMS
with k_moments and k_cols, which run unchanged: its event time is the difference of that timer between the tied and the singleton handle.  It is set against the traffic it
moves, 2 x N x mom_total(D, K) x 8 bytes (every chain's moment block read once and written once).

--handles names the handles to create, in that order (a process gives its streams hardware queues in the order they are
created, and which queues the two streams of a handle get decides how well its lower bound overlaps the next iteration: the
same handle measures differently as the first and as the second of a process).  --label prefixes the lines.
`--handles plain --label parent_run1` in a copy of this script inside a built checkout of the parent commit (it imports the
package it lies beside), run before and after the run of this commit, gives the parent's time and its run-to-run spread.

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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=6)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--handles", default="plain,singletons,tied_128x8")
    ap.add_argument("--label", default="")
    ap.add_argument("--out")
    args = ap.parse_args()
    import numpy as np
    from bench import make_inputs
    from pyvb_amd.lds import LDSBatch
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    def timed(b):
        t0 = time.perf_counter()
        b.iterate(args.steps); b.sync()
        return (time.perf_counter() - t0) * 1e3 / args.steps

    def row(name, ms):
        say("%-22s median %8.3f ms  min %8.3f  max %8.3f  spread %6.3f   runs %s" % (
            name, statistics.median(ms), min(ms), max(ms), max(ms) - min(ms), " ".join("%.3f" % v for v in ms)))

    Y, st0, pri = make_inputs(T, D, D, N, seed=20240)
    make = {"plain": lambda: LDSBatch.from_problem(Y, st0, pri),
            "singletons": lambda: LDSBatch.from_problem(Y, st0, pri, models=np.arange(N, dtype=np.int32)),
            "tied_128x8": lambda: LDSBatch.from_problem(Y, st0, pri, models=np.arange(N, dtype=np.int32) // CHAINS)}
    names = args.handles.split(",")
    full = names == ["plain", "singletons", "tied_128x8"]
    handles = [(args.label + nm + ("_%d" % i if names.count(nm) > 1 else ""), make[nm]()) for i, nm in enumerate(names)]
    first = {k: np.ascontiguousarray(v[::CHAINS]) for k, v in st0.items()}
    Yfirst = np.ascontiguousarray(Y[::CHAINS])
    del Y
    for _, b in handles:        # warm-up: every kernel of the timed window has run, the classes are adopted
        b.iterate(3); b.sync()
    ms = {name: [] for name, _ in handles}
    for r in range(args.runs):
        k = r % len(handles)
        for name, b in handles[k:] + handles[:k]:
            ms[name].append(timed(b))
    for name, _ in handles:
        row(name, ms[name])
    params = {}
    for name, b in handles:
        b.timing(True)
        b.iterate(args.steps); b.sync()
        kt = b.kernel_times()
        b.timing(False)
        params[name] = kt["params"][0] / args.steps
        say("kernel times %-18s " % name + "  ".join("%s %.3f ms x %d" % (k, v[0] / max(v[1], 1), v[1]) for k, v in sorted(kt.items()) if v[1]))
    if full:
        med = {k: statistics.median(v) for k, v in ms.items()}
        say("singletons - plain: %+.3f ms per iteration;  tied - plain: %+.3f ms per iteration (medians)"
            % (med[args.label + "singletons"] - med[args.label + "plain"], med[args.label + "tied_128x8"] - med[args.label + "plain"]))
        mom_total = 3 * D * D + D * D + D
        gb = 2.0 * N * mom_total * 8 / 1e9
        tie_ms = params[args.label + "tied_128x8"] - params[args.label + "singletons"]
        say("k_tie: %.4f ms per iteration (PYVB_K_PARAMS, tied minus singletons) for %.3f GB moved = %.2f TB/s"
            % (tie_ms, gb, gb / tie_ms if tie_ms > 0 else float("nan")))
        e = handles[2][1].elbo()
        assert np.all(np.isfinite(e)) and np.all(e.reshape(N // CHAINS, CHAINS, 6)[:, 1:, 2:] == 0.0)
    for _, b in handles:
        b.close()
    if full:
        b = LDSBatch.from_problem(Yfirst, first, pri)
        b.iterate(3); b.sync()
        b.timing(True)
        b.iterate(args.steps); b.sync()
        kt = b.kernel_times()
        b.close()
        say("kernel times %-18s " % "plain_N128" + "  ".join("%s %.3f ms x %d" % (k, v[0] / max(v[1], 1), v[1]) for k, v in sorted(kt.items()) if v[1]))
    if args.out:
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
