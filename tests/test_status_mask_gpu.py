"""Per-replicate failure status and the activity mask of an LDS handle (include/pyvb_hip.h: pyvb_lds_get_status,
pyvb_lds_set_active), through pyvb_amd.lds.LDSBatch.

"Bitwise" below is justified, not measured: replicates share no arithmetic, and a twin handle of the same N, T, D, K has
the same time split and chunking (pyvb_lds_create), so the rows that are computed on both go through the same instructions
in the same order.  The one tolerance: elbo_total() sums the rows in another order than numpy does -- at most N additions
per part, so N * 2^-53 of the sum of the magnitudes.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

from pyvb_amd import synth

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


def _gamma(pri):
    pri["noise"] = "gamma"
    for k in ("Q_a0", "Q_b0", "R_a0", "R_b0"):
        pri[k] = np.float64(1e-3)


def _wishart(pri, D, K):
    rng = np.random.default_rng(D + K)
    pri["noise"] = "wishart"
    W = rng.standard_normal((D, D)); pri["Q_b0"] = 0.05 * (W @ W.T + D * np.eye(D)); pri["Q_a0"] = np.float64(0.5 * D + 1.0)
    W = rng.standard_normal((K, K)); pri["R_b0"] = 0.05 * (W @ W.T + K * np.eye(K)); pri["R_a0"] = np.float64(0.5 * K + 0.5)


# name -> (T, D, K, N, noise, outputs with NaN, the time split must be > 1)
CASES = {
    "diagonal_gamma_small": (600, 8, 6, 5, "diagonal_gamma", False, True),
    "gamma_small": (600, 16, 12, 4, "gamma", False, True),
    "wishart_small": (400, 6, 5, 4, "wishart", False, True),
    "diagonal_gamma_big": (200, 96, 80, 3, "diagonal_gamma", False, False),
    "gamma_big": (40, 70, 128, 3, "gamma", False, False),
    "wishart_big": (40, 72, 66, 3, "wishart", False, False),
    "diagonal_gamma_nan": (600, 8, 6, 5, "diagonal_gamma", True, True),
    "wishart_nan": (300, 6, 5, 4, "wishart", True, True),
}


def _problem(name):
    T, D, K, N, noise, nan, split = CASES[name]
    Y, st0, pri = synth.make_problem(T, D, K, N, seed=4100 + len(name))
    if noise == "gamma":
        _gamma(pri)
    elif noise == "wishart":
        _wishart(pri, D, K)
    if nan:
        rng = np.random.default_rng(5)
        Y = Y.copy()
        Y[rng.random(Y.shape) < 0.1] = np.nan
        Y[:, 3] = np.nan                              # a row that is not observed at all
        st0["Yq"] = rng.standard_normal(Y.shape)
        st0["Yrowvar"] = 0.5 + rng.random(Y.shape[:2])
    return Y, st0, pri, nan, split


def _batch(Y, st0, pri):
    from pyvb_amd.lds import LDSBatch
    return LDSBatch.from_problem(Y, st0, pri)


def _everything(b):
    """Every getter of the handle, as one dict of arrays with leading axis N."""
    out = dict(b.get_state())
    out["Sigma"], out["qld_x"] = b.get_posterior_classes()
    out["qld_A"], out["qld_C"] = b.get_column_qld()
    for k, v in b.get_logdets().items():
        out["lnd_" + k] = v
    out["Yq"], out["Yvar"], out["Yqld"] = b.get_outputs(with_qld=True)
    if b.noise == "wishart":
        out.update(b.get_wishart_state())
        out["A_cov"], out["C_cov"] = b.get_column_cov()
    out["elbo"] = b.elbo()
    return out


def _same_rows(a, b, rows, what):
    for k in a:
        assert np.array_equal(a[k][rows], b[k][rows], equal_nan=True), (what, k)


@pytest.mark.parametrize("name", sorted(CASES))
def test_one_ill_posed_replicate_fails_alone(name):
    Y, st0, pri, nan, split = _problem(name)
    N, r = Y.shape[0], 1
    bad = {k: v.copy() for k, v in st0.items()}
    bad["Q_b"][r] = -np.abs(bad["Q_b"][r]) * 1e-9       # as tests/test_gpu_parity.py::test_not_positive_definite_raises
    b, twin = _batch(Y, bad, pri), _batch(Y, st0, pri)
    try:
        if split:
            assert b.get_time_split() > 1
        assert b.get_time_split() == twin.get_time_split()
        assert b.active().all() and not b.status().any()
        b.sweep("forward"); twin.sweep("forward")
        with pytest.raises(np.linalg.LinAlgError) as ei:
            b.sync()
        assert ei.value.replicates == [r], ei.value.replicates
        assert "replicate %d" % r in str(ei.value)
        st = b.status()
        assert st[r] != 0 and not np.delete(st, r).any(), st
        twin.sync()
        mask = np.ones(N, dtype=bool); mask[r] = False
        b.set_active(mask)
        assert np.array_equal(b.active(), mask)
        if nan:                                         # (the bound is undefined until every unobserved output has been updated)
            b.update_Y(); twin.update_Y()
        b.iterate(3); twin.iterate(3)
        b.sync()                                        # the switched-off row does not raise again
        assert not b.status().any()                     # a successful sync forgets what the failed one reported
        tot, rows = b.elbo_total(), b.elbo()
        assert np.isfinite(tot).all(), tot
        want = rows[mask].sum(0)
        assert np.all(np.abs(tot - want) <= N * 2.0 ** -52 * np.abs(rows[mask]).sum(0)), (tot, want)
        hist = b.elbo_history()
        assert hist.shape == (3, 6) and np.isfinite(hist).all(), hist
        twin.elbo_total(); twin.elbo()
        _same_rows(_everything(b), _everything(twin), mask, "active rows against the healthy twin")
    finally:
        b.close(); twin.close()


def _mixed_updates(b, nan, probe):
    """iterate and the stage-wise calls mixed; probe(b) is called where the X buffers have flipped an odd number of times."""
    D = b.D
    b.iterate(1)
    b.sweep("forward")
    probe(b)
    b.sweep("backward")
    b.update_x(0); b.update_x(b.T // 2); b.update_x(b.T - 1)
    b.update_columns("A", 0, D); b.update_columns("C", 0, max(1, D // 2)); b.update_columns("C", max(1, D // 2), D) if D > 1 else None
    b.update_Q(); b.update_R()
    if nan:
        b.update_Y()
    b.elbo()
    b.iterate(2)
    b.sweep("forward")                                  # (odd again: the getters below meet the parked rows in the other buffer)


@pytest.mark.parametrize("name", sorted(CASES))
def test_switched_off_rows_stand_still_and_the_others_do_not_notice(name):
    from pyvb_amd import _capi
    Y, st0, pri, nan, split = _problem(name)
    N = Y.shape[0]
    b, twin = _batch(Y, st0, pri), _batch(Y, st0, pri)
    try:
        if split:
            assert b.get_time_split() > 1
        b.iterate(2); twin.iterate(2)
        before, _ = _everything(b), _everything(twin)
        mask = np.ones(N, dtype=bool); mask[[0, N - 1]] = False
        b.set_active(mask)
        probes = []
        _mixed_updates(b, nan, lambda h: probes.append(h.get_state(("X",))["X"]))
        _mixed_updates(twin, nan, lambda h: probes.append(h.get_state(("X",))["X"]))
        assert np.array_equal(probes[0][~mask], before["X"][~mask])
        assert np.array_equal(probes[0][mask], probes[1][mask])
        after, ref = _everything(b), _everything(twin)
        _same_rows(after, before, ~mask, "switched-off rows against their values when they were switched off")
        _same_rows(after, ref, mask, "active rows against the unmasked twin")
        tot = b.elbo_total()
        assert np.all(np.abs(tot - after["elbo"][mask].sum(0)) <= N * 2.0 ** -52 * np.abs(after["elbo"][mask]).sum(0))
        # the mask can only shrink
        with pytest.raises(_capi.PyvbHipError) as ei:
            b.set_active(np.ones(N, dtype=bool))
        assert ei.value.code == _capi.E_ARG and "shrink" in str(ei.value)
        assert np.array_equal(b.active(), mask)
        # every row off: the update entries are no-ops, the totals are zero
        b.set_active(np.zeros(N, dtype=bool))
        still = _everything(b)
        b.timing(True)
        _mixed_updates(b, nan, lambda h: None)
        assert all(cnt == 0 for _, cnt in b.kernel_times().values()), b.kernel_times()
        _same_rows(_everything(b), still, np.ones(N, dtype=bool), "all rows off")
        assert np.array_equal(b.elbo_total(), np.zeros(6))
        assert np.array_equal(b.elbo_history()[-1], np.zeros(6))
    finally:
        b.close(); twin.close()


def test_a_switched_off_row_does_not_reach_the_other_ranks(tmp_path):
    """Two ranks on one GPU over the host transport (tests/test_multirank_gpu.py), a fresh child process each: rank 0 holds an
    ill-posed replicate, switches it off, and its NaN reach neither rank's totals nor the history of iterate()."""
    worker = os.path.join(HERE, "status_mask_worker.py")
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT="29810", HSA_ENABLE_IPC_MODE_LEGACY="0")
    prefix = str(tmp_path / "mask")
    procs = [subprocess.Popen([sys.executable, worker, str(r), "2", prefix], env=env, stdout=subprocess.PIPE,
                              stderr=subprocess.STDOUT, text=True) for r in range(2)]
    outs = []
    for p in procs:
        try:
            out, _ = p.communicate(timeout=300)
        except subprocess.TimeoutExpired:
            for q in procs:
                q.kill()
            raise
        outs.append(out)
    assert all(p.returncode == 0 for p in procs), "\n".join(outs)[-3000:]
    res = [dict(np.load(prefix + "_%d.npz" % r)) for r in range(2)]
    assert list(res[0]["failed"]) == [1] and list(res[1]["failed"]) == []
    assert np.isnan(res[0]["elbo_rows"][1]).any()       # the row itself was garbage when it was switched off
    total = res[0]["elbo_local"] + res[1]["elbo_local"]
    for m in res:
        assert np.isfinite(m["elbo_total"]).all() and np.isfinite(m["history"]).all(), (m["elbo_total"], m["history"])
        assert np.all(np.abs(m["elbo_total"] - total) <= 1e-13 * np.abs(total)), (m["elbo_total"], total)
    assert np.array_equal(res[0]["elbo_total"], res[1]["elbo_total"])
    assert np.array_equal(res[0]["history"], res[1]["history"])
