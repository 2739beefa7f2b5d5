"""k_prep with one work matrix in LDS and the three inversions in turn (pyvb_amd/csrc/k_prep.hip): four workgroups share a CU.

Shapes: every path of the kernel -- full tiles, padded rows and columns, a single partial tile, K < D, the non-staged path
(K tile count above D's) and Wishart noise -- at T = 12 (every segment's warm-up reaches the boundary) and T = 66, after one
iterate() against the oracle in extended precision at the envelope's yardstick (tests/test_envelope_gpu.py: 16 times what
the float64 oracle loses on the same problem), and the warm-up lengths against the rule as tests/test_param_tail_gpu.py.

Residency: 1024 distinct replicates on one handle -- the smallest case in which four workgroups share a CU's LDS -- computed
again in handles of eight: replicates share no arithmetic, so bit for bit (two iterations at T = 16, where both handles add
the statistics up in one chunk; at T = 20 the first iteration's classes, warm-up lengths and states: see the test).

Status: one replicate whose precision is not positive definite fails alone among 1024."""
import functools

import numpy as np
import pytest

import bench
import extended_ref as E
from pyvb_amd import _capi

pytestmark = pytest.mark.gpu

N = 9
SHAPES = [(64, 64, False), (17, 33, False), (3, 4, False), (64, 16, False), (16, 64, False), (8, 8, True)]
LENGTHS = (12, 66)


def _case(D, K, T, wishart):
    seed = 9000 + 100 * D + K + T
    c = E._wishart(T, D, K, N, seed, iters=1) if wishart else E._plain(T, D, K, N, seed)
    c["iters"] = 1
    return c


@functools.lru_cache(maxsize=None)
def _reference(D, K, T, wishart):
    """({name: long-double array}, {name: distance of the float64 oracle from it}, (F, B) [N, D, D] of the extended run) for
    the states X and the classes Sigma after the two sweeps of the first iteration: what k_prep's results go into (the
    parameter updates behind them change neither).  Computed once per case, never modified."""
    c = _case(D, K, T, wishart)
    copy = lambda d: {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in d.items()}
    m64 = E.OracleLDS(c["Y"].copy(), copy(c["st0"]), c["pri"])
    mx = E.OracleLDS(E.to_long(c["Y"]), E.to_long(c["st0"]), E.to_long(c["pri"]))
    ext, e64 = {}, {}
    for m in (m64, mx):
        m.sweep("forward")
        m.sweep("backward")
    for name in ("X", "Sigma"):
        ax = np.array(mx.read(name))
        assert ax.dtype == E.LD
        ax.setflags(write=False)
        ext[name], e64[name] = ax, E.rel(m64.read(name), ax)
    return ext, e64, mx.recurrences[0]


@pytest.mark.parametrize("T", LENGTHS)
@pytest.mark.parametrize("D,K,wishart", SHAPES)
def test_one_iterate_against_the_extended_oracle(D, K, wishart, T):
    from pyvb_amd.lds import LDSBatch
    c = _case(D, K, T, wishart)
    ext, e64, (F, B) = _reference(D, K, T, wishart)
    b = LDSBatch.from_problem(c["Y"], c["st0"], c["pri"])
    try:
        b.iterate(1)
        b.sync()
        h = E.HandleLDS(b)
        n, over = max(D, K, T), []
        for name in ext:
            got = np.array(h.read(name))
            assert np.all(np.isfinite(got)), name
            e_gpu = E.rel(got, ext[name])
            ratio = e_gpu / E.yardstick(e64[name], n)
            print("d%d k%d t%d %-6s e64 %.2e  e_gpu %.2e  e_gpu/y %6.2f%s"
                  % (D, K, T, name, e64[name], e_gpu, ratio, "  <-- over" if ratio > E.FACTOR else ""))
            assert e64[name] <= E.CAP, name
            if not ratio <= E.FACTOR:
                over.append((name, e_gpu, ratio))
        assert not over, over
        w, bad = b.get_warmup(), []
        for r in range(N):
            for M, which, J, what in ((F[r], "inf", int(w[r, 0]), "forward"), (B[r], "1", int(w[r, 1]), "backward")):
                Jstar = E.warmup_rule(M, which)
                print("d%d k%d t%d replicate %d %-8s J %4d  rule %4d%s" % (D, K, T, r, what, J, Jstar, "" if J == Jstar else "  <-- differs"))
                if J != Jstar:
                    bad.append((r, what, J, Jstar))
        assert not bad, "(replicate, sweep, J, rule) %r" % bad
    finally:
        b.close()


def _rows(Y, st0, rows):
    return Y[rows].copy(), {k: v[rows].copy() for k, v in st0.items()}


def _results(b):
    S, q = b.get_posterior_classes()
    return {"Sigma": S, "qld_x": q, "warm": b.get_warmup(), "X": b.get_state(("X",))["X"], "elbo": b.elbo()}


ALL = ("Sigma", "qld_x", "warm", "X", "elbo")


# A handle of eight cuts the time axis of its statistics into min(32, ceil(T / 16)) chunks where one of 1024 takes it whole
# (geometry.h), so from T = 17 on the two add the moments up in another order: the bound of the first iteration and everything
# of the second then differ in the last bits, on any kernel.  Two iterations with everything equal therefore run at T = 16
# (k_prep does not see T); at T = 20 the comparison is what k_prep and the sweeps of the first iteration produce.
@pytest.mark.parametrize("T,iters,keys", [(16, 2, ALL), (20, 1, ("Sigma", "qld_x", "warm", "X"))])
def test_1024_resident_replicates_equal_handles_of_eight(T, iters, keys):
    from pyvb_amd.lds import LDSBatch
    D, K, NR = 64, 64, 1024
    Y, st0, pri = bench.make_inputs(T, D, K, NR, 31)
    b = LDSBatch.from_problem(Y, st0, pri)
    try:
        b.iterate(iters)
        b.sync()
        assert not b.status().any()
        whole, split = _results(b), b.get_time_split()
    finally:
        b.close()
    assert len({whole["X"][r].tobytes() for r in range(NR)}) == NR, "the replicates are not distinct problems"
    for lo in (0, 508, 1016):
        rows = np.arange(lo, lo + 8)
        Yr, sr = _rows(Y, st0, rows)
        s = LDSBatch.from_problem(Yr, sr, pri)
        try:
            assert s.get_time_split() == split
            s.iterate(iters)
            s.sync()
            part = _results(s)
        finally:
            s.close()
        for k in keys:
            assert np.array_equal(whole[k][rows], part[k]), "replicates %d-%d: %s" % (lo, lo + 7, k)


def test_one_ill_posed_replicate_among_1024_fails_alone():
    from pyvb_amd.lds import LDSBatch
    T, D, K, NR, r = 20, 64, 64, 1024, 515
    Y, st0, pri = bench.make_inputs(T, D, K, NR, 32)
    bad = {k: v.copy() for k, v in st0.items()}
    bad["Q_b"][r] = -np.abs(bad["Q_b"][r]) * 1e-9       # as tests/test_status_mask_gpu.py::test_one_ill_posed_replicate_fails_alone
    b = LDSBatch.from_problem(Y, bad, pri)
    try:
        assert b.active().all() and not b.status().any()
        b.sweep("forward")
        with pytest.raises(np.linalg.LinAlgError) as ei:
            b.sync()
        assert ei.value.replicates == [r], ei.value.replicates
        st = b.status()
        assert st[r] & _capi.FAIL_STATES and not np.delete(st, r).any(), st[st != 0]
    finally:
        b.close()
