"""The part of a sweep launch that is not its loop: DESIGN.md section 4, profiles/sweep_boundary_timing.txt.

    python profiles/sweep_fixed_cost.py [--steps 6] [--warmup 3] [--label LABEL] [--out FILE]

The loop of k_sweep takes ceil((T - 2) / 16) + J steps (J: the warm-up length k_prep derives, pyvb_lds_get_warmup) and its time
is linear in that count.  The two boundary nodes, the load of the F / B / G operands and the epilogue are paid once per launch,
whatever T is.  The headline's D = K = 64 and 1024 replicates (bench.py supplies the inputs, cut to the first T time points)
at T = 2 502, 5 002, 10 002 -- 157, 313 and 626 loop steps before the warm-up -- `steps` iterations each with the library's
event timers on (as bench.py --full), then a least-squares line  ms = a + b * steps  through the three points of the forward
and of the backward launch.  `a` is the fixed part in ms per launch; it is printed with the points it was fitted to.

The step count uses the mean J over the replicates (all 1024 wavefronts are resident at once and share the power budget, so a
launch's time follows the total work, not the slowest chain); the fit with the largest J is printed beside it.

A step that fails ends the run: nothing further is started on the GPU.
"""
import argparse
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

D, N = 64, 1024
LENGTHS = (2502, 5002, 10002)


def fit(x, y):
    """Least-squares a, b of y = a + b x, and the largest residual."""
    import numpy as np
    x, y = np.asarray(x, dtype=float), np.asarray(y, dtype=float)
    b, a = np.polyfit(x, y, 1)
    return a, b, float(np.abs(a + b * x - y).max())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=6)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--label", default="")
    ap.add_argument("--out")
    args = ap.parse_args()
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    from bench import make_inputs
    from pyvb_amd.lds import LDSBatch

    Yfull, st_full, pri = make_inputs(max(LENGTHS), D, D, N, seed=20240)
    pts = {"sweep_fwd": [], "sweep_bwd": []}
    steps_mean, steps_max = {"sweep_fwd": [], "sweep_bwd": []}, {"sweep_fwd": [], "sweep_bwd": []}
    for T in LENGTHS:
        st0 = {k: (v[:, :T] if k == "X" else v) for k, v in st_full.items()}
        b = LDSBatch.from_problem(Yfull[:, :T], st0, pri)
        assert b.get_time_split() == 1
        b.iterate(args.warmup); b.sync()
        b.timing(True)
        b.iterate(args.steps); b.sync()
        kt = b.kernel_times()
        b.timing(False)
        w = b.get_warmup()
        b.close()
        lseg = (T - 2 + 15) // 16
        for col, nm in enumerate(("sweep_fwd", "sweep_bwd")):
            ms, cnt = kt[nm]
            assert cnt == args.steps, (nm, cnt)
            pts[nm].append(ms / cnt)
            steps_mean[nm].append(lseg + float(w[:, col].mean()))
            steps_max[nm].append(lseg + int(w[:, col].max()))
            say("%sT %6d  %-9s %8.4f ms per launch   loop steps %4d + J (mean %.1f, max %d)" % (
                args.label, T, nm, ms / cnt, lseg, w[:, col].mean(), w[:, col].max()))
    for nm in ("sweep_fwd", "sweep_bwd"):
        a, bb, res = fit(steps_mean[nm], pts[nm])
        a2, b2, res2 = fit(steps_max[nm], pts[nm])
        say("%s%-9s a = %7.4f ms per launch, b = %.5f ms per step (largest residual %.4f ms);  with the largest J: a = %7.4f, b = %.5f (%.4f)" % (
            args.label, nm, a, bb, res, a2, b2, res2))
    if args.out:
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
