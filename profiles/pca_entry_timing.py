"""What DiagonalGamma precision parents on the entries of W (pyvb_pca_set_entry_precisions, k_pca.hip: PCA_ENTRY) cost: DESIGN.md
section 24.

    python profiles/pca_entry_timing.py [--runs 5] [--steps 100] [--label LABEL] [--out FILE]
    python profiles/pca_entry_timing.py --parent [--label parent_run1] [--out FILE]

bench.py's pca_config5 (N = 10^6, d = 256, q = 16, 10 % missing; pyvb_amd.synth supplies the rows as it does for bench.py), one
process, one GPU, `runs` runs of `steps` iterations per variant, the variants alternating inside every run.

 (a) pyvb_pca_iterate on a plain handle: the same kernels with the same arguments as in the parent.
 (b) the same on a handle with Gamma parents on the columns (pyvb_pca_set_column_precisions): likewise the parent's kernels.
     --parent measures (a) and (b) for a copy of this script inside a built checkout of the parent commit (it imports the package
     it lies beside), run before and after the run of this commit: the parent's times and their own run-to-run spread are the
     yardstick.
 (c) the same handle with DiagonalGamma parents: one more step, PCA_ENTRY, inside the head launch of every iteration.
 (d) the parents' update alone, update_entry_precisions() `steps` times, asynchronous, one sync at the end: one launch of one
     workgroup each.

A step that fails ends the run: nothing further is started on the GPU.
"""
import argparse
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

N, d, q = 1000000, 256, 16


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--rows", type=int, default=N)
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
    from pyvb_amd import synth
    from pyvb_amd.pca import PCABatch

    def timed(b, fn, per):
        t0 = time.perf_counter()
        fn(); b.sync()
        return (time.perf_counter() - t0) * 1e3 / per

    def row(name, ms):
        say("%-36s median %8.4f ms  min %8.4f  max %8.4f  spread %6.4f   runs %s" % (
            args.label + name, statistics.median(ms), min(ms), max(ms), max(ms) - min(ms), " ".join("%.4f" % v for v in ms)))

    rows = args.rows
    pri = synth.pca_problem(16, d, q, 33)[1]
    X, obs, Z0, W0 = synth.pca_rows(0, rows, d, q, 33)
    data, start = np.where(obs, X, np.nan), np.where(obs, X, 0.0)
    del X, obs

    def handle():
        b = PCABatch(rows, d, q)
        b.set_priors(pri)
        b.set_data(data)
        b.set_state(X_missing=start, W_mean=W0, Z=Z0, Z_cov=np.eye(q), Mu_mean=np.zeros(d), beta_b=1.0)
        return b

    rng = np.random.default_rng(7)
    plain = handle()
    plain.iterate(10); plain.sync()
    gamma = handle()
    gamma.set_column_precisions(1e-3, 1e-3, 0.5 + rng.random(q))
    gamma.iterate(10); gamma.sync()
    variants = [("plain_iterate", plain, lambda: plain.iterate(args.steps)),
                ("gamma_parents_iterate", gamma, lambda: gamma.iterate(args.steps))]
    entry = None
    if not args.parent:
        entry = handle()
        entry.set_entry_precisions(1e-3, 1e-3, 0.5 + rng.random((q, d)))
        entry.iterate(10); entry.sync()
        variants.append(("entry_parents_iterate", entry, lambda: entry.iterate(args.steps)))
    ms = {name: [] for name, _, _ in variants}
    for r in range(args.runs):
        k = r % len(variants)
        for name, b, fn in variants[k:] + variants[:k]:
            ms[name].append(timed(b, fn, args.steps))
    for name, _, _ in variants:
        row(name, ms[name])
    med = {k: statistics.median(v) for k, v in ms.items()}
    if entry is not None:
        say("entry parents - plain = %+.4f ms per iteration (medians)" % (med["entry_parents_iterate"] - med["plain_iterate"]))
        say("entry parents - gamma parents = %+.4f ms per iteration (medians)" % (med["entry_parents_iterate"] - med["gamma_parents_iterate"]))

        def entry_only():
            for _ in range(args.steps):
                entry.update_entry_precisions()
        entry_only(); entry.sync()
        row("entry_update_alone_one_launch", [timed(entry, entry_only, args.steps) for _ in range(args.runs)])
        entry.close()
    plain.close(); gamma.close()
    finish()


if __name__ == "__main__":
    main()
