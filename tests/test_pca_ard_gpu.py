"""GPU: Gamma precision parents for the columns of W on VB-PCA handles (pyvb_pca_set_column_precisions; k_pca.hip: PCA_ARD).

Shapes (N, d, q) -- each with per-column a0, b0, qb and non-zero prior means, so that a stride of 0 or a dropped pm shows:
    (20, 5, 2)      a partly filled block of 16 columns (the example's shape)
    (30, 70, 5)     k < d tails inside a wavefront; rows left unpinned
    (24, 250, 16)   one full block, d over four wavefronts
    (36, 40, 32)    two column blocks: block 2's W_pp is read after block 1 was updated
    (20, 256, 17)   full height, one column into the second block
    (3, 1, 1)       the smallest handle

Accuracy: the handle against the reference's own run (tests/golden/ward_*.npz) and against tests/pca_ard_ref.py at the parity
tolerance RTOL = 1e-8 after every iteration, and against the comparator's long-double run by the rule of DESIGN.md section 17,
e_gpu <= 16 max(e64, n 2^-52), n = max(d, q, N), after iterations 1 and 2, for W, W_var, Z, Z_cov, X, Mu, Beta, qb and the five
parts of both bounds.

Measured on an MI355X (test_envelope prints every figure): e_gpu <= 3.1e-15 on every state quantity, at most
0.21 of the rule's bound except on the 3 x 1 x 1 handle (2.8 of the 16 allowed, n 2^-52 = 6.7e-16 there); the worst part of the
bound is off by 4.1e-16 of the bound's sum of |part| (L_Z at (30, 70, 5), reference mode), at most 0.13 of the rule's bound.
"""
import glob
import os
import subprocess
import sys

import numpy as np
import pytest

import extended_ref as ER
import pca_ard_ref as PR
from conftest import GOLDEN_DIR
from pyvb_amd import _capi

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
WARD = sorted(glob.glob(os.path.join(GOLDEN_DIR, "ward_*.npz")))
RTOL = 1e-8
STATE = ("X", "X_rowvar", "W_mean", "W_var", "Z", "Z_cov", "Mu_mean", "Mu_var", "beta_ab")


def _close(a, b, what, rtol=RTOL):
    a, b = np.asarray(a, dtype=float), np.asarray(b, dtype=float)
    assert np.all(np.isfinite(a)), what + ": non-finite"
    err = np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)
    assert err <= rtol, "%s: rel err %.3e" % (what, err)


def _handle(N, d, q, sweep=None, mode=None):
    from pyvb_amd.pca import PCABatch
    b = PCABatch.from_problem(*PR.handle_problem(*PR.problem(N, d, q)))
    if sweep is not None:
        b.set_sweep(sweep)
    if mode not in (None, "reference"):
        b.set_bound_mode(mode)
    return b


def _stagewise(b, N, n=1):
    for _ in range(n):
        b.update_W(); b.update_Z(); b.update_column_precisions(); b.update_X(0, 1); b.update_Mu(); b.update_X(1, N); b.update_Beta()


def _everything(b):
    """every array a handle gives back, the bound and qb included"""
    g = b.get_state()
    out = {k: g[k] for k in STATE}
    out["elbo"] = b.elbo()
    out["alpha_a"], out["alpha_b"] = b.column_precisions()
    return out


def _assert_bitwise(a, b, what):
    assert sorted(a) == sorted(b)
    for k in a:
        assert np.array_equal(a[k], b[k]), "%s: %s differs" % (what, k)


# ---- accuracy -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", WARD, ids=lambda p: os.path.basename(p)[5:-4])
def test_reference_fixtures(path):
    from pyvb_amd.pca import PCABatch
    N, d, q, init, pri, z = PR.load_fixture(path)
    b = PCABatch.from_problem(*PR.handle_problem(init, pri))
    for it in range(1, int(max(z["iters"])) + 1):
        b.iterate(1)
        if it in z["iters"]:
            tag = "it%d_" % it
            g = b.get_state()
            for k in ("W_mean", "W_var", "Z", "Z_cov", "X", "Mu_mean", "Mu_var", "beta_a", "beta_b"):
                _close(g[k], z[tag + k], tag + k)
            qa, qb = b.column_precisions()
            assert np.array_equal(qa, z[tag + "W_alpha_a"])
            _close(qb, z[tag + "W_alpha_b"], tag + "W_alpha_b")
            parts, ref = b.elbo(), z[tag + "elbo_parts"]
            assert np.all(np.abs(parts - ref) <= RTOL * np.abs(ref).sum()), (parts, ref)
    b.close()


@pytest.mark.parametrize("mode", ER.BOUND_MODES)
@pytest.mark.parametrize("N,d,q", PR.SHAPES)
def test_envelope(N, d, q, mode):
    """Stage-wise in the crawl order, read at the end of each iteration: every quantity and the five parts of the bound of `mode`
    against the float64 comparator at RTOL and against its long-double run by the rule of section 17."""
    n, ext, e64, bnd, hld, f64 = PR.reference(N, d, q)
    assert max(e64.values()) <= ER.CAP and hld >= 0.25
    b = _handle(N, d, q, mode=mode)
    tag = "pca_ard_%d_%d_%d %s" % (N, d, q, mode)
    rows, brows = [], []
    for key, arr in PR.trace(b, N, bounds=(mode,), parts=ER.pca_handle_parts(b), qb=lambda: b.column_precisions()[1]):
        assert np.all(np.isfinite(arr)), key
        if ER.is_bound(key):
            x, e, _ = bnd[key]
            brows += [(key,) + row for row in ER.compare_bound(arr, x, e, n)]
            assert np.all(np.abs(arr - f64[key]) <= RTOL * np.abs(f64[key]).sum()), (key, arr, f64[key])
            continue
        _close(arr, f64[key], "%s %r" % (tag, key))
        e_gpu = ER.rel(arr, ext[key])
        rows.append((key, e64[key], e_gpu, e_gpu / ER.yardstick(e64[key], n)))
    b.close()
    for key, e, eg, ratio in rows:
        print("%-28s it%d %-10s e64 %.2e  e_gpu %.2e  e_gpu/y %6.2f%s" % (tag, key[0] + 1, key[2], e, eg, ratio, "  <-- over" if ratio > ER.FACTOR else ""))
    for key, rep, p, e, eg, ratio, own in brows:
        print("%-28s it%d %-10s e64 %.2e  e_gpu %.2e  e_gpu/y %6.2f  (of the part itself %.2e)%s"
              % (tag, key[0] + 1, ER.PCA_PARTS[p], e, eg, ratio, own, "  <-- over" if ratio > ER.FACTOR else ""))
    worst_b = max(brows, key=lambda r: r[4])
    print("%-28s SUMMARY  state: max e_gpu %.2e  max e_gpu/y %.2f;  bound: worst e_gpu %.2e (its share of the bound) on %s, max e_gpu/y %.2f"
          % (tag, max(r[2] for r in rows), max(r[3] for r in rows), worst_b[4], ER.PCA_PARTS[worst_b[2]], max(r[5] for r in brows)))
    assert len(rows) == PR.ITERS * len(PR.NAMES) and len(brows) == PR.ITERS * 5
    over = [r for r in rows if not r[3] <= ER.FACTOR] + [r for r in brows if not r[5] <= ER.FACTOR]
    assert not over, "%s: %d quantities beyond %g x yardstick: %r" % (tag, len(over), ER.FACTOR, over)


# ---- behaviour ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,d,q", [(20, 5, 2), (36, 40, 32), (20, 256, 17)])
def test_stagewise_calls_equal_iterate_bitwise(N, d, q):
    a, b = _handle(N, d, q), _handle(N, d, q)
    a.iterate(3)
    _stagewise(b, N, 3)
    _assert_bitwise(_everything(a), _everything(b), "iterate(3) against stage-wise calls")
    a.close(); b.close()


@pytest.mark.parametrize("sweep", ["columns", "pairs"])
def test_stagewise_calls_equal_iterate_through_the_chosen_sweeps(sweep):
    N, d, q = 600, 250, 16
    a, b = _handle(N, d, q, sweep), _handle(N, d, q, sweep)
    assert a.sweep == b.sweep == sweep
    a.iterate(2)
    _stagewise(b, N, 2)
    ea, eb = _everything(a), _everything(b)
    for k in ea:
        if k == "elbo":
            assert np.all(np.abs(ea[k] - eb[k]) <= RTOL * np.abs(eb[k]).sum()), (ea[k], eb[k])
        else:
            _close(ea[k], eb[k], "%s sweep: %s" % (sweep, k))
    # and the run is the comparator's
    init, pri = PR.problem(N, d, q)
    st = PR.make_state(init, pri, N, d, q)
    for _ in range(2):
        parts = PR.iterate(st, pri)
    _close(ea["alpha_b"], st["W_alpha_b"], "alpha_b")
    _close(ea["W_mean"], st["W_mean"], "W_mean")
    assert np.all(np.abs(ea["elbo"] - parts) <= RTOL * np.abs(parts).sum()), (ea["elbo"], parts)
    a.close(); b.close()


def test_two_runs_give_bitwise_equal_qb():
    N, d, q = 20, 256, 17
    runs = []
    for _ in range(2):
        b = _handle(N, d, q)
        b.iterate(3)
        runs.append(_everything(b))
        b.close()
    assert np.array_equal(runs[0]["alpha_b"], runs[1]["alpha_b"])
    _assert_bitwise(runs[0], runs[1], "two runs")


def test_set_priors_takes_the_hyperpriors_away_bitwise():
    """pyvb_pca_set_priors after the setter: the handle is the one that never had hyperpriors."""
    from pyvb_amd.pca import PCABatch
    N, d, q = 36, 40, 32
    init, pri = ER.pca_problem(N, d, q)
    plain = PCABatch.from_problem(init, pri)
    was = PCABatch.from_problem(init, dict(pri, W_alpha=(2.0, 0.7, np.linspace(0.5, 1.5, q))))
    assert np.array_equal(was.column_precisions()[1], np.linspace(0.5, 1.5, q))
    was.set_priors(pri)
    with pytest.raises(_capi.PyvbHipError) as e:
        was.column_precisions()
    assert e.value.code == _capi.E_ARG
    plain.iterate(3); was.iterate(3)
    for k, v in plain.get_state().items():
        assert np.array_equal(v, was.get_state()[k]), k
    assert np.array_equal(plain.elbo(), was.elbo())
    plain.close(); was.close()


def test_a_handle_without_hyperpriors_is_the_parent_handle():
    """It never makes the new call: the same kernels with the same arguments.  Held to values the suite pins already -- the
    reference's fixture at RTOL (tests/test_pca_gpu.py: test_golden_fixtures) -- and two fresh handles equal each other bitwise."""
    from pyvb_amd.pca import PCABatch
    from test_pca_oracle_golden import load_pca
    path = sorted(p for p in glob.glob(os.path.join(GOLDEN_DIR, "pca_*.npz")) if "default_init" not in p)[0]
    N, d, q, init, pri, z = load_pca(path)
    a, b = PCABatch.from_problem(init, pri), PCABatch.from_problem(init, pri)
    its = int(min(z["iters"]))
    a.iterate(its); b.iterate(its)
    ga, gb = a.get_state(), b.get_state()
    for k in ga:
        assert np.array_equal(ga[k], gb[k]), k
    assert np.array_equal(a.elbo(), b.elbo())
    for k in ("W_mean", "W_var", "Z", "Z_cov", "X", "Mu_mean", "Mu_var", "beta_a", "beta_b"):
        _close(ga[k], z["it%d_%s" % (its, k)], k)
    ref = z["it%d_elbo_parts" % its]
    assert np.all(np.abs(a.elbo() - ref) <= RTOL * np.abs(ref).sum())
    for h in (a, b):
        with pytest.raises(_capi.PyvbHipError):
            h.update_column_precisions()
    a.close(); b.close()


def _ranks(world, tmp_path, port):
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY="0")
    prefix = str(tmp_path / ("ard_w%d" % world))
    worker = os.path.join(HERE, "pca_ard_multirank_worker.py")
    procs = [subprocess.Popen([sys.executable, worker, str(r), str(world), prefix], env=env, stdout=subprocess.PIPE,
                              stderr=subprocess.STDOUT, text=True) for r in range(world)]
    outs = []
    for p in procs:
        try:
            out, _ = p.communicate(timeout=300)
        except subprocess.TimeoutExpired:
            for other in procs:
                other.kill()
            raise
        outs.append(out)
    assert all(p.returncode == 0 for p in procs), "\n".join(outs)[-3000:]
    return [dict(np.load(prefix + "_%d.npz" % r)) for r in range(world)]


def test_two_ranks_on_one_gpu(tmp_path):
    """Rows sharded over two ranks (host transport): the alpha update is a local launch, W is the same on every rank, so qb is
    bitwise the same; global quantities against the single-rank run at 1e-10, the figure of tests/test_multirank_gpu.py."""
    one = _ranks(1, tmp_path, 29810)[0]
    many = _ranks(2, tmp_path, 29820)
    assert [tuple(m["rows"]) for m in many] == [(0, 21), (21, 41)]
    assert np.array_equal(many[0]["alpha_b"], many[1]["alpha_b"]) and np.array_equal(many[0]["alpha_a"], many[1]["alpha_a"])
    rel = lambda a, b: float(np.abs(np.asarray(a) - np.asarray(b)).max() / max(np.abs(np.asarray(b)).max(), 1e-300))
    for m in many:
        for k in ("W_mean", "W_var", "Mu_mean", "Mu_var", "Z_cov", "beta_ab", "elbo", "alpha_b"):
            assert rel(m[k], one[k]) < 1e-10, (k, rel(m[k], one[k]))
    for k in ("X", "Z", "X_rowvar"):
        assert rel(np.concatenate([m[k] for m in many]), one[k]) < 1e-10, k


# ---- refusals -----------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_handle_alone():
    N, d, q = 20, 5, 2
    b = _handle(N, d, q)
    b.iterate(1)
    before = _everything(b)
    good = np.ones(q)
    for bad in (0.0, -1.0, np.nan, np.inf):
        v = np.array([1.0, bad])
        for args in ((v, good, good), (good, v, good), (good, good, v)):
            with pytest.raises(_capi.PyvbHipError) as e:
                b.set_column_precisions(*args)
            assert e.value.code == _capi.E_ARG and "finite and positive" in str(e.value) and "column 1" in str(e.value)
    p = _capi.dptr(good)
    assert _capi.lib.pyvb_pca_set_column_precisions(b._h, p, None, p) == _capi.E_ARG
    _assert_bitwise(before, _everything(b), "after the refused calls")         # nothing was uploaded, nothing launched
    b.close()
    from pyvb_amd.pca import PCABatch
    plain = PCABatch.from_problem(*ER.pca_problem(N, d, q))
    for call in (plain.update_column_precisions, plain.column_precisions):
        with pytest.raises(_capi.PyvbHipError) as e:
            call()
        assert e.value.code == _capi.E_ARG and "Constant precision parents" in str(e.value)
    with pytest.raises(_capi.PyvbHipError):
        plain.set_column_precisions(1.0, 1.0, [1.0, -2.0])
    with pytest.raises(_capi.PyvbHipError):                                       # the refused setter did not switch them on
        plain.column_precisions()
    plain.close()
