"""GPU: DiagonalGamma precision parents, a Gamma per entry of W, on VB-PCA handles (pyvb_pca_set_entry_precisions; k_pca.hip:
PCA_ENTRY).

Shapes (N, d, q) -- each with per-entry a0, b0, qb and non-zero prior means, so that a stride of 0, a transposed index or a dropped
pm shows:
    (20, 5, 2)      the first fixture's shape: a partly filled block of eight columns
    (30, 70, 5)     rows left unpinned; d spans two wavefronts, the second partial
    (24, 250, 16)   the lazy sweep's widest; two full column blocks
    (36, 40, 32)    largest q: four column blocks
    (20, 256, 17)   full width, q > 16 (the write-back sweep): one column into the third block
    (3, 1, 1)       the smallest handle

Accuracy: the handle against the reference's own run (tests/golden/wentry_*.npz) and against tests/pca_entry_ref.py at the parity
tolerance RTOL = 1e-8 after every iteration, and against the comparator's long-double run by the rule of DESIGN.md section 17,
e_gpu <= 16 max(e64, n 2^-52), n = max(d, q, N), after iterations 1 and 2, for W, W_var, Z, Z_cov, X, Mu, Beta, qb and the five
parts of both bounds.  test_envelope prints every figure; the measured worst cases are in DESIGN.md section 24.
"""
import glob
import os
import subprocess
import sys

import numpy as np
import pytest

import extended_ref as ER
import pca_ard_ref as AR
import pca_entry_ref as PR
from conftest import GOLDEN_DIR
from pyvb_amd import _capi

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
WARD = sorted(glob.glob(os.path.join(GOLDEN_DIR, "ward_*.npz")))
WENTRY = sorted(glob.glob(os.path.join(GOLDEN_DIR, "wentry_*.npz")))
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
        b.update_W(); b.update_Z(); b.update_entry_precisions(); b.update_X(0, 1); b.update_Mu(); b.update_X(1, N); b.update_Beta()


def _everything(b):
    """every array a handle gives back, the bound and qb included"""
    g = b.get_state()
    out = {k: g[k] for k in STATE}
    out["elbo"] = b.elbo()
    out["entry_a"], out["entry_b"] = b.entry_precisions()
    return out


def _assert_bitwise(a, b, what):
    assert sorted(a) == sorted(b)
    for k in a:
        assert np.array_equal(a[k], b[k]), "%s: %s differs" % (what, k)


# ---- accuracy -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", WENTRY, ids=lambda p: os.path.basename(p)[7:-4])
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
            qa, qb = b.entry_precisions()
            assert np.array_equal(qa, z[tag + "W_entry_a"])
            _close(qb, z[tag + "W_entry_b"], tag + "W_entry_b")
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
    tag = "pca_entry_%d_%d_%d %s" % (N, d, q, mode)
    rows, brows = [], []
    for key, arr in PR.trace(b, N, bounds=(mode,), parts=ER.pca_handle_parts(b), qb=lambda: b.entry_precisions()[1]):
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
    _close(ea["entry_b"], st["W_entry_b"], "entry_b")
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
    assert np.array_equal(runs[0]["entry_b"], runs[1]["entry_b"])
    _assert_bitwise(runs[0], runs[1], "two runs")


def _entry_args(d, q, seed=5):
    rng = np.random.default_rng(seed)
    return rng.uniform(1.0, 3.0, (q, d)), rng.uniform(0.5, 1.5, (q, d)), rng.uniform(0.5, 1.5, (q, d))


def _state_and_bound(b):
    out = dict(b.get_state())
    out["elbo"] = b.elbo()
    return out


def test_set_priors_takes_the_parents_away_bitwise():
    """pyvb_pca_set_priors after the setter: the handle is the one that never had parents."""
    from pyvb_amd.pca import PCABatch
    N, d, q = 36, 40, 32
    init, pri = ER.pca_problem(N, d, q)
    a0, b0, qb = _entry_args(d, q)
    plain = PCABatch.from_problem(init, pri)
    was = PCABatch.from_problem(init, dict(pri, W_entry=(a0, b0, qb)))
    got = was.entry_precisions()
    assert np.array_equal(got[0], a0 + 0.5) and np.array_equal(got[1], qb)
    was.set_priors(pri)
    for call in (was.entry_precisions, was.update_entry_precisions):
        with pytest.raises(_capi.PyvbHipError) as e:
            call()
        assert e.value.code == _capi.E_ARG
    plain.iterate(3); was.iterate(3)
    _assert_bitwise(_state_and_bound(plain), _state_and_bound(was), "set_priors after set_entry_precisions")
    plain.close(); was.close()


@pytest.mark.parametrize("last", ["entry", "column"])
def test_of_the_two_setters_the_last_one_holds_bitwise(last):
    """Either order of pyvb_pca_set_column_precisions and pyvb_pca_set_entry_precisions: the handle is the one that only ever
    had the last; get / update of the other kind are argument errors."""
    from pyvb_amd.pca import PCABatch
    N, d, q = 20, 70, 17
    init, pri = ER.pca_problem(N, d, q)
    entry, column = _entry_args(d, q), (np.linspace(1.0, 3.0, q), np.linspace(0.5, 1.5, q), np.linspace(1.5, 0.5, q))
    both = PCABatch.from_problem(init, pri)
    if last == "entry":
        both.set_column_precisions(*column); both.set_entry_precisions(*entry)
        only = PCABatch.from_problem(init, dict(pri, W_entry=entry))
        mine, other = (lambda h: h.entry_precisions()), (both.column_precisions, both.update_column_precisions)
    else:
        both.set_entry_precisions(*entry); both.set_column_precisions(*column)
        only = PCABatch.from_problem(init, dict(pri, W_alpha=column))
        mine, other = (lambda h: h.column_precisions()), (both.entry_precisions, both.update_entry_precisions)
    for call in other:
        with pytest.raises(_capi.PyvbHipError) as e:
            call()
        assert e.value.code == _capi.E_ARG
    both.iterate(3); only.iterate(3)
    _assert_bitwise(_state_and_bound(both), _state_and_bound(only), "the last setter")
    assert np.array_equal(mine(both)[1], mine(only)[1])
    both.close(); only.close()


def test_a_handle_without_these_parents_is_the_parent_handle():
    """It never makes the new call: the same kernels with the same arguments.  Held to values the suite pins already -- the
    reference's fixtures at RTOL, one with Constant parents (tests/test_pca_gpu.py) and one with Gamma parents
    (tests/test_pca_ard_gpu.py) -- and the new entries refuse it."""
    from pyvb_amd.pca import PCABatch
    from test_pca_oracle_golden import load_pca
    path = sorted(p for p in glob.glob(os.path.join(GOLDEN_DIR, "pca_*.npz")) if "default_init" not in p)[0]
    N, d, q, init, pri, z = load_pca(path)
    a = PCABatch.from_problem(init, pri)
    its = int(min(z["iters"]))
    a.iterate(its)
    ga = a.get_state()
    for k in ("W_mean", "W_var", "Z", "Z_cov", "X", "Mu_mean", "Mu_var", "beta_a", "beta_b"):
        _close(ga[k], z["it%d_%s" % (its, k)], k)
    ref = z["it%d_elbo_parts" % its]
    assert np.all(np.abs(a.elbo() - ref) <= RTOL * np.abs(ref).sum())
    N, d, q, init, pri, z = AR.load_fixture(sorted(p for p in WARD if "default_init" not in p)[0])
    b = PCABatch.from_problem(*AR.handle_problem(init, pri))
    done = 0
    for it in [int(i) for i in z["iters"]]:
        b.iterate(it - done)
        done = it
        g = b.get_state()
        for k in ("W_mean", "W_var", "Z", "Z_cov", "X", "Mu_mean", "Mu_var", "beta_a", "beta_b"):
            _close(g[k], z["it%d_%s" % (it, k)], k)
        _close(b.column_precisions()[1], z["it%d_W_alpha_b" % it], "W_alpha_b")
        ref = z["it%d_elbo_parts" % it]
        assert np.all(np.abs(b.elbo() - ref) <= RTOL * np.abs(ref).sum())
    for h in (a, b):
        for call in (h.update_entry_precisions, h.entry_precisions):
            with pytest.raises(_capi.PyvbHipError) as e:
                call()
            assert e.value.code == _capi.E_ARG and "no DiagonalGamma precision parents" in str(e.value)
    a.close(); b.close()


def _ranks(world, tmp_path, port):
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY="0")
    prefix = str(tmp_path / ("entry_w%d" % world))
    worker = os.path.join(HERE, "pca_entry_multirank_worker.py")
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
    """Rows sharded over two ranks (host transport): the parents' update is a local launch, W is the same on every rank, so qb is
    bitwise the same; global quantities against the single-rank run at 1e-10, the figure of tests/test_multirank_gpu.py."""
    one = _ranks(1, tmp_path, 29830)[0]
    many = _ranks(2, tmp_path, 29840)
    assert [tuple(m["rows"]) for m in many] == [(0, 21), (21, 41)]
    assert np.array_equal(many[0]["entry_b"], many[1]["entry_b"]) and np.array_equal(many[0]["entry_a"], many[1]["entry_a"])
    rel = lambda a, b: float(np.abs(np.asarray(a) - np.asarray(b)).max() / max(np.abs(np.asarray(b)).max(), 1e-300))
    for m in many:
        for k in ("W_mean", "W_var", "Mu_mean", "Mu_var", "Z_cov", "beta_ab", "elbo", "entry_b"):
            assert rel(m[k], one[k]) < 1e-10, (k, rel(m[k], one[k]))
    for k in ("X", "Z", "X_rowvar"):
        assert rel(np.concatenate([m[k] for m in many]), one[k]) < 1e-10, k


# ---- refusals -----------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_handle_alone():
    N, d, q = 20, 5, 2
    b = _handle(N, d, q)
    b.iterate(1)
    before = _everything(b)
    good = np.ones((q, d))
    for bad in (0.0, -1.0, np.nan, np.inf):
        v = good.copy()
        v[1, 3] = bad
        for args in ((v, good, good), (good, v, good), (good, good, v)):
            with pytest.raises(_capi.PyvbHipError) as e:
                b.set_entry_precisions(*args)
            assert e.value.code == _capi.E_ARG and "finite and positive" in str(e.value) and "entry 3 of column 1" in str(e.value)
    p = _capi.dptr(good)
    assert _capi.lib.pyvb_pca_set_entry_precisions(b._h, p, None, p) == _capi.E_ARG
    for call in (b.column_precisions, b.update_column_precisions):      # the other kind of parent is not what this handle has
        with pytest.raises(_capi.PyvbHipError) as e:
            call()
        assert e.value.code == _capi.E_ARG
    _assert_bitwise(before, _everything(b), "after the refused calls")         # nothing was uploaded, nothing launched
    b.close()
    from pyvb_amd.pca import PCABatch
    plain = PCABatch.from_problem(*ER.pca_problem(N, d, q))
    for call in (plain.update_entry_precisions, plain.entry_precisions):
        with pytest.raises(_capi.PyvbHipError) as e:
            call()
        assert e.value.code == _capi.E_ARG and "no DiagonalGamma precision parents" in str(e.value)
    bad = good.copy()
    bad[0, 0] = -2.0
    with pytest.raises(_capi.PyvbHipError):
        plain.set_entry_precisions(1.0, 1.0, bad)
    with pytest.raises(_capi.PyvbHipError):                                       # the refused setter did not switch them on
        plain.entry_precisions()
    plain.close()
