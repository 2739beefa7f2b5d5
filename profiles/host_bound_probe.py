"""A configuration whose iteration is bound by the host, not by the kernels: N 4, T 40, D 12, K 9, iterate(200), five timings in one
process.  Prints one line: the five ms-per-iteration values and their median.  Two builds are compared with PYVB_HIP_LIB
(profiles/lds_flow_refactor.txt)."""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from pyvb_amd import synth
from pyvb_amd.lds import LDSBatch

T, D, K, N, ITERS = 40, 12, 9, 4, 200
Y, st0, pri = synth.make_problem(T, D, K, N, seed=3)
b = LDSBatch.from_problem(Y, st0, pri)
b.iterate(20); b.sync()
runs = []
for _ in range(5):
    t0 = time.perf_counter(); b.iterate(ITERS); b.sync()
    runs.append((time.perf_counter() - t0) / ITERS * 1e3)
b.close()
print("host_bound N=%d T=%d D=%d K=%d iterate(%d) ms/iteration: %s median %.5f" % (N, T, D, K, ITERS, " ".join("%.5f" % r for r in runs), float(np.median(runs))), flush=True)
