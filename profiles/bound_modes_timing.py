"""Time one headline iteration (T = 1e4, D = K = 64, N = 1024) in each bound mode: four rounds of five iterations per mode,
alternating, medians.  python profiles/bound_modes_timing.py"""
import sys, time, os
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from pyvb_amd import synth
from pyvb_amd.lds import LDSBatch

T, D, K, N = 10000, 64, 64, 1024
Y, st0, pri = synth.make_problem(T, D, K, 8, seed=3)
Y = np.tile(Y, (N // 8, 1, 1)); st0 = {k: np.tile(v, (N // 8,) + (1,) * (v.ndim - 1)) for k, v in st0.items()}
b = LDSBatch.from_problem(Y, st0, pri)
b.iterate(3); b.sync()
res = {"reference": [], "exact": []}
for rnd in range(4):
    for mode in ("reference", "exact"):
        b.set_bound_mode(mode)
        b.sync()
        t0 = time.perf_counter(); b.iterate(5); b.sync(); t1 = time.perf_counter()
        res[mode].append((t1 - t0) / 5 * 1e3)
for m, v in res.items():
    print("%-9s ms/iter: %s  median %.3f" % (m, " ".join("%.3f" % x for x in v), float(np.median(v))))
print("exact / reference: %.4f" % (np.median(res["exact"]) / np.median(res["reference"])))
b.set_bound_mode("exact"); b.iterate(2); print("exact history tail", b.elbo_history()[-2:].sum(axis=1))
