"""CPU: Gamma precision parents for the columns of W on the VB-PCA path (pyvb_pca_set_column_precisions) -- what needs no device.

1. tests/pca_ard_ref.py, the composition of oracle functions that the GPU tests compare against, reproduces the reference's own
   run of such graphs (tests/golden/ward_*.npz, written by tests/golden/make_golden_pca_ard.py) at 1e-10 relative, the project's
   figure for a comparator against the reference, and follows the crawl order the fixtures record.
2. On the cases the device is measured on, the float64 comparator lies within the guard of DESIGN.md section 17 of its own
   extended-precision run: e64 <= 1e-11 on every quantity and every part of both bounds after both iterations; no column's
   1/2 ln det qprec is near the pole of q_ln_det (quirk Q1) on any of them.
3. The exact bound, whose alpha terms the reference cannot pin, never decreases over 30 iterations in long double.
4. The yardstick of section 17 sees a sum over a column's variances that is wrong by 1e-10; a tolerance of 1e-8 does not.
5. The three C ABI entries exist everywhere they must, with the declared signatures; NULL arguments are argument errors before
   any HIP call.
"""
import glob
import os
import re
import subprocess

import numpy as np
import pytest

import extended_ref as ER
import pca_ard_ref as PR
from conftest import GOLDEN_DIR
from pyvb_amd import _capi

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("pyvb_pca_set_column_precisions", "pyvb_pca_get_column_precisions", "pyvb_pca_update_column_precisions")
WARD = sorted(glob.glob(os.path.join(GOLDEN_DIR, "ward_*.npz")))
RTOL = 1e-10        # comparator against reference (tests/test_pca_oracle_golden.py, tests/test_oracle_golden.py)


def _close(a, b, what, rtol=RTOL):
    a, b = np.asarray(a, dtype=float), np.asarray(b, dtype=float)
    err = np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)
    assert err <= rtol, "%s: rel err %.3e" % (what, err)


def test_the_three_fixtures_are_present():
    assert [os.path.basename(p) for p in WARD] == ["ward_default_init_n15_d4_q2.npz", "ward_example_n20_d5_q2.npz",
                                                  "ward_means_n12_d7_q3.npz"]


# ---- 1. the comparator against the reference --------------------------------------------------------------------------------
@pytest.mark.parametrize("path", WARD, ids=lambda p: os.path.basename(p)[5:-4])
def test_fixture_structure(path):
    N, d, q, init, pri, z = PR.load_fixture(path)
    order = [str(s) for s in z["order"]]
    assert order == ["W%d" % i for i in range(q)] + ["Z%d" % n for n in range(N)] + ["A%d" % i for i in range(q)] + \
        ["X0", "Mu"] + ["X%d" % n for n in range(1, N)] + ["Beta"]
    assert PR.stage_order(order) == PR.ORDER
    assert list(z["iters"]) == [1, 2, 5]
    assert np.isnan(np.where(init["obs"], 0.0, np.nan)).any()           # entries are missing in every fixture
    assert ("X_full" in init) == ("default_init" in path)
    if "means" in path:
        assert np.all(pri["W_prior_mean"] != 0) and len(set(pri["W_alpha_a0"])) == q and len(set(pri["W_alpha_b0"])) == q
    for it in z["iters"]:
        assert z["it%d_Z_cov_spread" % it] <= 1e-14          # every Z_n has the same covariance
        assert z["it%d_W_cov_offdiag_max" % it] == 0.0       # column covariances stay diagonal: thread = row survives
        assert np.array_equal(z["it%d_W_alpha_a" % it], pri["W_alpha_a0"] + 0.5 * d)


@pytest.mark.parametrize("path", WARD, ids=lambda p: os.path.basename(p)[5:-4])
def test_comparator_reproduces_the_reference(path):
    N, d, q, init, pri, z = PR.load_fixture(path)
    st = PR.make_state(init, pri, N, d, q)
    order = PR.stage_order(z["order"])
    for it in range(1, int(max(z["iters"])) + 1):
        parts = PR.iterate(st, pri, order)
        if it in z["iters"]:
            tag = "it%d_" % it
            for k in ("W_mean", "W_var", "Z", "Z_cov", "X", "X_var", "Mu_mean", "Mu_var", "beta_a", "beta_b", "W_alpha_a", "W_alpha_b"):
                _close(st[k], z[tag + k], tag + k)
            ref = z[tag + "elbo_parts"]
            print(tag, "parts", parts, "reference", ref)
            assert np.all(np.abs(parts - ref) <= RTOL * np.abs(ref).sum()), (parts, ref)


def test_the_alpha_update_commutes_with_the_z_update():
    """What lets the device run it right behind the W update, inside the same launch."""
    N, d, q, init, pri, z = PR.load_fixture(WARD[2])
    a, b = PR.make_state(init, pri, N, d, q), PR.make_state(init, pri, N, d, q)
    for _ in range(3):
        pa = PR.iterate(a, pri, PR.ORDER)
        pb = PR.iterate(b, pri, ("W", "alpha", "Z", "X0", "Mu", "X", "Beta"))
        assert np.array_equal(pa, pb)
    for k in ("W_mean", "Z", "X", "W_alpha_b", "beta_b"):
        assert np.array_equal(a[k], b[k]), k


# ---- 2. the float64 comparator against its extended-precision run -----------------------------------------------------------
@pytest.mark.parametrize("N,d,q", PR.SHAPES)
def test_float64_comparator_is_inside_the_guard(N, d, q):
    n, ext, e64, bnd, hld, _ = PR.reference(N, d, q)
    assert ext[(0, "update_Beta", "X")].dtype == ER.LD
    assert len(ext) == PR.ITERS * len(PR.NAMES) and len(bnd) == PR.ITERS * len(PR.BOUNDS)
    for k, e in e64.items():
        print("iteration %d %-10s e64 %.2e" % (k[0] + 1, k[2], e))
        assert e <= ER.CAP, (k, e)
    for k, (_, e, _) in bnd.items():
        print("iteration %d bound %-9s e64 %.2e" % (k[0] + 1, k[2], e.max()))
        assert e.max() <= ER.CAP, (k, e)
    # quirk Q1: q_ln_det = 1 / ln det qprec has a pole where a column's 1/2 ln det qprec passes through 0
    print("min |1/2 ln det qprec| of a column: %.3f" % hld)
    assert hld >= 0.25


# ---- 3. the exact bound ----------------------------------------------------------------------------------------------------
def test_exact_bound_never_decreases_in_long_double():
    """The only check of the exact-mode terms that the reference cannot pin: a mis-derived alpha term breaks the monotonicity
    every update of a variational family guarantees for E_q[ln p] - E_q[ln q]."""
    N, d, q = 20, 5, 2
    init, pri = PR.problem(N, d, q)
    st = PR.make_state(ER.to_long(init), ER.to_long(pri), N, d, q)
    tot = [PR.iterate(st, ER.to_long(pri), PR.ORDER, mode="exact").sum() for _ in range(30)]
    assert tot[0].dtype == ER.LD
    steps = np.diff(np.array(tot, dtype=ER.LD))
    print("exact bound: first %.6f last %.6f smallest step %.3e" % (tot[0], tot[-1], steps.min()))
    assert np.all(steps >= -1e-15 * np.abs(np.array(tot[1:], dtype=ER.LD)))
    assert tot[-1] > tot[0]


# ---- 4. the yardstick sees a wrong sum --------------------------------------------------------------------------------------
def test_a_wrong_variance_sum_is_caught_by_the_yardstick_and_missed_at_1e_8():
    """One column's sum of variances enters qb scaled by 1 + 1e-10.  That moves qb by 1e-10 times the share s of the variances
    in qb, and the rule of section 17 resolves nothing below 16 n 2^-52 = 7.1e-14 at n = 20: the mutant is visible where
    s > 7.1e-4.  On the measured cases the first W update leaves s between 7e-7 and 2e-2 (the noise precision is high there), so
    this runs the example's shape with the noise rate beta_b raised 1e4-fold, where the variances are a tenth of qb or more."""
    N, d, q = 20, 5, 2
    init, pri = PR.problem(N, d, q)
    init["beta_b"] = init["beta_b"] * 1e4
    key = (0, "update_Beta", "W_alpha_b")
    runs = {}
    for name, cast, scale in (("f64", lambda v: v, None), ("ext", ER.to_long, None), ("mutant", lambda v: v, np.array([1.0, 1.0 + 1e-10]))):
        m = PR.OraclePCAARD(cast(init), cast(pri), N, d, q)
        if scale is not None:
            m.update_column_precisions = lambda m=m, scale=scale: PR.stage(m.st, m.pri, "alpha", scale)
        runs[name] = dict(PR.trace(m, N, iters=1))[key]
        if name == "f64":
            share = 0.5 * m.st["W_var"].sum(axis=1) / m.st["W_alpha_b"]
    assert runs["ext"].dtype == ER.LD and share[1] > 0.1, share
    e64, e = ER.rel(runs["f64"], runs["ext"]), ER.rel(runs["mutant"], runs["ext"])
    y = ER.yardstick(e64, max(N, d, q))
    print("share of the variances in qb %r; e64 %.3e, mutant %.3e, yardstick %.3e, ratio %.1f" % (share, e64, e, y, e / y))
    assert e64 <= ER.CAP and e64 <= ER.FACTOR * y       # the clean comparator passes the rule
    assert e > ER.FACTOR * y                             # the rule rejects the mutant
    assert e < 1e-8                                      # the parity tolerance would have let it pass


# ---- 5. the C ABI -----------------------------------------------------------------------------------------------------------
def test_entries_are_declared_exported_and_bound():
    header = open(os.path.join(REPO, "include", "pyvb_hip.h")).read()
    decl = {
        ENTRIES[0]: r"int pyvb_pca_set_column_precisions\(pyvb_pca\* h, const double\* a0, const double\* b0, const double\* qb\);",
        ENTRIES[1]: r"int pyvb_pca_get_column_precisions\(pyvb_pca\* h, double\* qa, double\* qb\);",
        ENTRIES[2]: r"int pyvb_pca_update_column_precisions\(pyvb_pca\* h\);",
    }
    c, dp, h = _capi.ctypes.c_int, _capi._dp, _capi._h
    args = {ENTRIES[0]: [h, dp, dp, dp], ENTRIES[1]: [h, dp, dp], ENTRIES[2]: [h]}
    for name in ENTRIES:
        assert re.search("^" + decl[name], header, re.M), name + " is not declared as specified in include/pyvb_hip.h"
        assert _capi.SIGNATURES[name] == (c, args[name]), name
        assert getattr(_capi.lib, name).argtypes == args[name]
    out = subprocess.run(["nm", "-D", "--defined-only", _capi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert set(ENTRIES) <= exported
    assert _capi.lib.pyvb_version() >= 106


def test_a_null_handle_is_an_argument_error():
    v = np.ones(4)
    p = _capi.dptr(v)
    for rc in (_capi.lib.pyvb_pca_set_column_precisions(None, p, p, p), _capi.lib.pyvb_pca_get_column_precisions(None, p, p),
               _capi.lib.pyvb_pca_update_column_precisions(None)):
        assert rc == _capi.E_ARG
        assert b"handle is NULL" in _capi.lib.pyvb_last_error()


def test_python_layer_has_the_three_methods():
    from pyvb_amd.pca import PCABatch
    for name in ("set_column_precisions", "column_precisions", "update_column_precisions"):
        assert callable(getattr(PCABatch, name))
