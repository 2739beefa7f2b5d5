"""What the activity mask (pyvb_lds_set_active) costs, and what switching replicates off saves: DESIGN.md section 12.

    python profiles/active_mask_timing.py [--parent-tree DIR] [--runs 5] [--steps 10] [--out FILE]

Times pyvb_lds_iterate at the headline shape (T = 10^4, D = K = 64) and at the 128-wide class's (D = K = 128), five runs of
`steps` iterations each after a warm-up, every case in a fresh child process, one after the other on one GPU:

    this build     N = 1024, all active             against   parent build, N = 1024   (the cost of the mask)
    this build     N = 1024, every second row off   against   parent build, N = 512    (what an inactive row still costs)
    this build     N = 1024, the first 512 active   against   parent build, N = 512
    this build     the last two again, with pyvb_lds_set_time_split(the split pyvb_lds_create picks for 512 replicates) after the mask
    this build     D = K = 128, N = 1024            against   parent build, the same

--parent-tree: a checkout of the parent commit with its library built (the child imports pyvb_amd and bench from there; it has
no mask, so only the all-active cases run on it).  Without it only this build's cases run.  A case that fails ends the run: nothing further is
started on the GPU.  bench.py supplies the inputs (make_inputs), so the numbers are those of its workload.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# name -> (D = K, N, mask, which build)
CASES = [
    ("parent_n1024", 64, 1024, "all", "parent"),
    ("this_n1024_all_active", 64, 1024, "all", "this"),
    ("parent_n512", 64, 512, "all", "parent"),
    ("this_n512_all_active", 64, 512, "all", "this"),
    ("this_n1024_every_second_active", 64, 1024, "alternate", "this"),
    ("this_n1024_first_512_active", 64, 1024, "first_half", "this"),
    ("this_n1024_every_second_active_resplit", 64, 1024, "alternate+split", "this"),
    ("this_n1024_first_512_active_resplit", 64, 1024, "first_half+split", "this"),
    ("parent_d128_n1024", 128, 1024, "all", "parent"),
    ("this_d128_n1024_all_active", 128, 1024, "all", "this"),
]
T = 10000


def create_time_split(N, T, slots=1024):
    """pyvb_lds_create's choice of wavefronts per replicate for N replicates (api.hip; D, K <= 64)."""
    best, W_best, W = 1e300, 1, 1
    while W <= 128 and (W == 1 or (T - 2) // W >= 64):
        part = (((T - 2 + W - 1) // W) + 15) & ~15
        cost = ((N * W + slots - 1) // slots) * ((part + 15) // 16 + 32)
        if cost < best * 0.97:
            best, W_best = cost, W
        W += 1
    return W_best


def one_case(name, runs, steps, tree):
    sys.path.insert(0, tree)
    import numpy as np
    from bench import make_inputs
    from pyvb_amd.lds import LDSBatch
    _, D, N, mask, _ = [c for c in CASES if c[0] == name][0]
    Y, st0, pri = make_inputs(T, D, D, N, seed=777 if D > 64 else 20240)
    b = LDSBatch.from_problem(Y, st0, pri)
    del Y
    b.iterate(2); b.sync()
    if mask != "all":
        m = np.zeros(N, dtype=bool)
        if mask.startswith("alternate"):
            m[::2] = True
        else:
            m[:N // 2] = True
        b.set_active(m)
        if mask.endswith("+split"):
            # the sweeps are a sequential chain per wavefront: 512 chains of full length take as long as 1024.  A handle
            # of 512 replicates deals the time axis of each to two wavefronts (pyvb_lds_create: W); so can this one now.
            b.set_time_split(create_time_split(int(m.sum()), T))
    b.iterate(3); b.sync()
    ms = []
    for _ in range(runs):
        t0 = time.perf_counter()
        b.iterate(steps); b.sync()
        ms.append((time.perf_counter() - t0) * 1e3 / steps)
    tot = b.elbo_total()
    b.close()
    print(json.dumps({"case": name, "ms_per_iteration": ms, "median": statistics.median(ms), "min": min(ms), "max": max(ms),
                      "elbo_total": float(tot.sum())}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-tree")
    ap.add_argument("--tree", default=REPO, help=argparse.SUPPRESS)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--out")
    ap.add_argument("--case")
    args = ap.parse_args()
    if args.case:
        return one_case(args.case, args.runs, args.steps, os.path.abspath(args.tree))
    lines = []
    for name, D, N, mask, build in CASES:
        if build == "parent" and not args.parent_tree:
            continue
        tree = os.path.abspath(args.parent_tree) if build == "parent" else REPO
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--case", name, "--runs", str(args.runs), "--steps", str(args.steps),
                            "--tree", tree], cwd=tree, capture_output=True, text=True, timeout=600)
        if r.returncode != 0:
            sys.stderr.write(r.stdout + r.stderr)
            raise SystemExit("case %s failed (exit %d): stopping" % (name, r.returncode))
        line = [l for l in r.stdout.splitlines() if l.startswith("{")][-1]
        res = json.loads(line)
        text = "%-34s median %8.3f ms  min %8.3f  max %8.3f  spread %6.3f   runs %s" % (
            name, res["median"], res["min"], res["max"], res["max"] - res["min"], " ".join("%.3f" % v for v in res["ms_per_iteration"]))
        print(text, flush=True)
        lines.append(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
