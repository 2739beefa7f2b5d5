"""CPU: DiagonalGamma precision parents, one Gamma per entry of W, on the VB-PCA path (pyvb_pca_set_entry_precisions) -- what needs
no device.

1. tests/pca_entry_ref.py, the composition of oracle functions that the GPU tests compare against, reproduces the reference's own
   run of such graphs (tests/golden/wentry_*.npz, written by tests/golden/make_golden_pca_entry.py) at 1e-10 relative, the
   project's figure for a comparator against the reference, and follows the crawl order the fixtures record.
2. On the cases the device is measured on, the float64 comparator lies within the guard of DESIGN.md section 17 of its own
   extended-precision run: e64 <= 1e-11 on every quantity and every part of both bounds after both iterations; no column's
   1/2 ln det qprec is near the pole of q_ln_det (quirk Q1) on any of them.
3. The exact bound, whose parent terms the reference cannot pin, never decreases over 30 iterations in long double.
4. The yardstick of section 17 sees one entry's variance enter qb wrong by 1e-10; a tolerance of 1e-8 does not.
5. The three C ABI entries exist everywhere they must, with the declared signatures; NULL arguments are argument errors before
   any HIP call.
6. _recognise.describe_pca on graphs built with pyvb_amd.nodes accepts Gamma and DiagonalGamma parents on the columns of W with
   the right pri entries, and declines mixed kinds, a shared parent, a parent with further children and a Wishart, each with
   its reason.
"""
import glob
import os
import re
import subprocess

import numpy as np
import pytest

import extended_ref as ER
import pca_entry_ref as PR
from conftest import GOLDEN_DIR
from pyvb_amd import _capi

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("pyvb_pca_set_entry_precisions", "pyvb_pca_get_entry_precisions", "pyvb_pca_update_entry_precisions")
WENTRY = sorted(glob.glob(os.path.join(GOLDEN_DIR, "wentry_*.npz")))
RTOL = 1e-10        # comparator against reference (tests/test_pca_oracle_golden.py, tests/test_oracle_golden.py)


def _close(a, b, what, rtol=RTOL):
    a, b = np.asarray(a, dtype=float), np.asarray(b, dtype=float)
    err = np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)
    assert err <= rtol, "%s: rel err %.3e" % (what, err)


def test_the_three_fixtures_are_present():
    assert [os.path.basename(p) for p in WENTRY] == ["wentry_broad_n20_d5_q2.npz", "wentry_default_init_n15_d4_q2.npz",
                                                    "wentry_means_n12_d7_q3.npz"]
    assert [(int(z["N"]), int(z["d"]), int(z["q"])) for z in map(np.load, WENTRY)] == [(20, 5, 2), (15, 4, 2), (12, 7, 3)]


# ---- 1. the comparator against the reference --------------------------------------------------------------------------------
@pytest.mark.parametrize("path", WENTRY, ids=lambda p: os.path.basename(p)[7:-4])
def test_fixture_structure(path):
    N, d, q, init, pri, z = PR.load_fixture(path)
    order = [str(s) for s in z["order"]]
    assert order == ["W%d" % i for i in range(q)] + ["Z%d" % n for n in range(N)] + ["D%d" % i for i in range(q)] + \
        ["X0", "Mu"] + ["X%d" % n for n in range(1, N)] + ["Beta"]
    assert PR.stage_order(order) == PR.ORDER
    assert list(z["iters"]) == [1, 2, 5]
    assert np.isnan(np.where(init["obs"], 0.0, np.nan)).any()           # entries are missing in every fixture
    assert ("X_full" in init) == ("default_init" in path)
    assert init["W_entry_b"].shape == pri["W_entry_a0"].shape == pri["W_entry_b0"].shape == (q, d)
    if "broad" in path:
        assert np.all(pri["W_entry_a0"] == 1e-3) and np.all(pri["W_entry_b0"] == 1e-3)
    if "means" in path:
        assert np.all(pri["W_prior_mean"] != 0)
        assert len(set(pri["W_entry_a0"].ravel())) == q * d and len(set(pri["W_entry_b0"].ravel())) == q * d
    for it in z["iters"]:
        assert z["it%d_Z_cov_spread" % it] <= 1e-14          # every Z_n has the same covariance
        assert z["it%d_W_cov_offdiag_max" % it] == 0.0       # column covariances stay diagonal: thread = row survives
        assert np.array_equal(z["it%d_W_entry_a" % it], pri["W_entry_a0"] + 0.5)


@pytest.mark.parametrize("path", WENTRY, ids=lambda p: os.path.basename(p)[7:-4])
def test_comparator_reproduces_the_reference(path):
    N, d, q, init, pri, z = PR.load_fixture(path)
    st = PR.make_state(init, pri, N, d, q)
    order = PR.stage_order(z["order"])
    for it in range(1, int(max(z["iters"])) + 1):
        parts = PR.iterate(st, pri, order)
        if it in z["iters"]:
            tag = "it%d_" % it
            for k in ("W_mean", "W_var", "Z", "Z_cov", "X", "X_var", "Mu_mean", "Mu_var", "beta_a", "beta_b", "W_entry_a", "W_entry_b"):
                _close(st[k], z[tag + k], tag + k)
            ref = z[tag + "elbo_parts"]
            print(tag, "parts", parts, "reference", ref)
            assert np.all(np.abs(parts - ref) <= RTOL * np.abs(ref).sum()), (parts, ref)


def test_the_comparator_keeps_the_dtype_it_is_given():
    N, d, q, init, pri, z = PR.load_fixture(WENTRY[0])
    for cast, dt in ((lambda v: v, np.float64), (ER.to_long, ER.LD)):
        st = PR.make_state(cast(init), cast(pri), N, d, q)
        parts = PR.iterate(st, cast(pri))
        assert parts.dtype == dt and st["W_entry_b"].dtype == dt and st["W_entry_a"].dtype == dt and st["W_mean"].dtype == dt


def test_the_parent_update_commutes_with_the_z_update():
    """What lets the device run it right behind the W update, inside the same launch."""
    N, d, q, init, pri, z = PR.load_fixture(WENTRY[2])
    a, b = PR.make_state(init, pri, N, d, q), PR.make_state(init, pri, N, d, q)
    for _ in range(3):
        pa = PR.iterate(a, pri, PR.ORDER)
        pb = PR.iterate(b, pri, ("W", "entry", "Z", "X0", "Mu", "X", "Beta"))
        assert np.array_equal(pa, pb)
    for k in ("W_mean", "Z", "X", "W_entry_b", "beta_b"):
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
    """The only check of the exact-mode terms that the reference cannot pin: a mis-derived parent term breaks the monotonicity
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


# ---- 4. the yardstick sees a wrong term -------------------------------------------------------------------------------------
def test_a_wrong_variance_term_is_caught_by_the_yardstick_and_missed_at_1e_8():
    """One entry's variance enters its qb scaled by 1 + 1e-10.  That moves that qb by 1e-10 times the share s of the variance in
    it, and the rule of section 17 resolves nothing below 16 n 2^-52 = 7.1e-14 at n = 20 (relative to the largest qb): the mutant is
    visible where the variance is a visible share of qb.  As in tests/test_pca_ard_cpu.py this runs the (20, 5, 2) shape with the
    noise rate beta_b raised 1e4-fold, where the first W update leaves variances that are a tenth of qb or more; the mutated
    entry is the one with the largest 1/2 var."""
    N, d, q = 20, 5, 2
    init, pri = PR.problem(N, d, q)
    init["beta_b"] = init["beta_b"] * 1e4
    key = (0, "update_Beta", "W_entry_b")
    clean = PR.OraclePCAEntry(init, pri, N, d, q)
    f64 = dict(PR.trace(clean, N, iters=1))[key]
    half_var = 0.5 * clean.st["W_var"]
    at = np.unravel_index(np.argmax(half_var), half_var.shape)
    share = half_var[at] / f64.max()            # of the largest qb, which is what ER.rel divides by
    scale = np.ones((q, d))
    scale[at] = 1.0 + 1e-10
    ext = dict(PR.trace(PR.OraclePCAEntry(ER.to_long(init), ER.to_long(pri), N, d, q), N, iters=1))[key]
    m = PR.OraclePCAEntry(init, pri, N, d, q)
    m.update_entry_precisions = lambda: PR.stage(m.st, m.pri, "entry", scale)
    mutant = dict(PR.trace(m, N, iters=1))[key]
    assert ext.dtype == ER.LD and share > 0.05, share
    e64, e = ER.rel(f64, ext), ER.rel(mutant, ext)
    y = ER.yardstick(e64, max(N, d, q))
    print("share of the variance in the largest qb %.3f; e64 %.3e, mutant %.3e, yardstick %.3e, ratio %.1f" % (share, e64, e, y, e / y))
    assert e64 <= ER.CAP and e64 <= ER.FACTOR * y       # the clean comparator passes the rule
    assert e > ER.FACTOR * y                             # the rule rejects the mutant
    assert e < 1e-8                                      # the parity tolerance would have let it pass


# ---- 5. the C ABI -----------------------------------------------------------------------------------------------------------
def test_entries_are_declared_exported_and_bound():
    header = open(os.path.join(REPO, "include", "pyvb_hip.h")).read()
    decl = {
        ENTRIES[0]: r"int pyvb_pca_set_entry_precisions\(pyvb_pca\* h, const double\* a0, const double\* b0, const double\* qb\);",
        ENTRIES[1]: r"int pyvb_pca_get_entry_precisions\(pyvb_pca\* h, double\* qa, double\* qb\);",
        ENTRIES[2]: r"int pyvb_pca_update_entry_precisions\(pyvb_pca\* h\);",
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
    assert _capi.lib.pyvb_version() >= 108


def test_a_null_handle_is_an_argument_error():
    v = np.ones(4)
    p = _capi.dptr(v)
    for rc in (_capi.lib.pyvb_pca_set_entry_precisions(None, p, p, p), _capi.lib.pyvb_pca_get_entry_precisions(None, p, p),
               _capi.lib.pyvb_pca_update_entry_precisions(None)):
        assert rc == _capi.E_ARG
        assert b"handle is NULL" in _capi.lib.pyvb_last_error()


def test_python_layer_has_the_three_methods():
    from pyvb_amd.pca import PCABatch
    for name in ("set_entry_precisions", "entry_precisions", "update_entry_precisions"):
        assert callable(getattr(PCABatch, name))


# ---- 6. the recogniser ------------------------------------------------------------------------------------------------------
def _graph(parent_of, N=6, d=4, q=3, extra=None):
    """The PCA graph on pyvb_amd.nodes; parent_of(nodes, i) is the precision parent of column i.  Nothing here touches a device:
    the nodes stay unbound."""
    from pyvb_amd import nodes
    np.random.seed(3)
    rng = np.random.default_rng(4)
    parents = [parent_of(nodes, i) for i in range(q)]
    Ws = [nodes.Gaussian(d, 0.1 * rng.standard_normal((d, 1)), parents[i]) for i in range(q)]
    W = nodes.hstack(Ws)
    Mu = nodes.Gaussian(d, np.zeros((d, 1)), np.eye(d) * 1e-3)
    Beta = nodes.Gamma(d, 1e-3, 1e-3)
    Zs = [nodes.Gaussian(q, np.zeros((q, 1)), np.eye(q)) for _ in range(N)]
    Xs = [nodes.Gaussian(d, W * z + Mu, Beta) for z in Zs]
    X = rng.standard_normal((N, d))
    X[1, 2] = np.nan
    [x.observe(row.reshape(d, 1)) for x, row in zip(Xs, X)]
    if extra:
        extra(nodes, parents, Ws)
    return dict(Ws=Ws, W=W, Mu=Mu, Beta=Beta, parents=parents)


A0 = np.array([1.5, 2.0, 2.5, 3.0])
B0 = np.array([0.5, 0.75, 1.0, 1.25])


def test_describe_pca_accepts_gamma_parents():
    from pyvb_amd import _recognise
    g = _graph(lambda nodes, i: nodes.Gamma(4, 1.0 + i, 0.5 + i))
    for i, p in enumerate(g["parents"]):
        p.qb = 0.25 * (i + 1)               # an assignment on an unbound graph: the description reads it back
    dsc = _recognise.describe_pca(g["Mu"])
    assert [id(p) for p in dsc["parents"]] == [id(p) for p in g["parents"]] and dsc["Beta"] is g["Beta"]
    a0, b0, qb = dsc["pri"]["W_alpha"]
    assert np.array_equal(a0, [1.0, 2.0, 3.0]) and np.array_equal(b0, [0.5, 1.5, 2.5]) and np.array_equal(qb, [0.25, 0.5, 0.75])
    assert "W_entry" not in dsc["pri"] and dsc["pri"]["W_prior_prec"].shape == (3, 4)
    assert [p.qa for p in g["parents"]] == [3.0, 4.0, 5.0]          # a0 + d / 2 stays the host attribute


def test_describe_pca_accepts_diagonal_gamma_parents():
    from pyvb_amd import _recognise
    g = _graph(lambda nodes, i: nodes.DiagonalGamma(4, A0 + i, B0 * (i + 1)))
    g["parents"][1].qb = np.array([0.1, 0.2, 0.3, 0.4])
    dsc = _recognise.describe_pca(g["W"])
    assert [id(p) for p in dsc["parents"]] == [id(p) for p in g["parents"]]
    a0, b0, qb = dsc["pri"]["W_entry"]
    assert a0.shape == b0.shape == qb.shape == (3, 4)
    assert np.array_equal(a0, np.stack([A0, A0 + 1, A0 + 2])) and np.array_equal(b0, np.stack([B0, 2 * B0, 3 * B0]))
    assert np.array_equal(qb[1], [0.1, 0.2, 0.3, 0.4])
    for i in (0, 2):                        # the constructor's scalar draw (nodes_todo.py:177) stands for every entry
        assert np.array_equal(qb[i], np.full(4, g["parents"][i].__dict__["_h_qb"]))
    assert "W_alpha" not in dsc["pri"]


def test_describe_pca_keeps_constant_parents_as_they_were():
    from pyvb_amd import _recognise
    dsc = _recognise.describe_pca(_graph(lambda nodes, i: np.eye(4) * (i + 1.0))["W"])
    assert dsc["parents"] == [] and "W_alpha" not in dsc["pri"] and "W_entry" not in dsc["pri"]
    assert np.array_equal(dsc["pri"]["W_prior_prec"], np.outer([1.0, 2.0, 3.0], np.ones(4)))


def _shared(nodes, i, box={}):
    if i == 0:
        box["p"] = nodes.Gamma(4, 1.0, 1.0)
    return box["p"] if i < 2 else nodes.Gamma(4, 1.0, 1.0)


def _further_child(nodes, parents, Ws):
    nodes.Gaussian(4, np.zeros((4, 1)), parents[1])


@pytest.mark.parametrize("parent_of,extra,reason", [
    (lambda nodes, i: nodes.Gamma(4, 1.0, 1.0) if i else nodes.DiagonalGamma(4, A0, B0), None, "mixed kinds"),
    (lambda nodes, i: nodes.Gamma(4, 1.0, 1.0) if i else np.eye(4), None, "mixed kinds"),
    (_shared, None, "shared by two columns"),
    (lambda nodes, i: nodes.DiagonalGamma(4, A0, B0), _further_child, "further children"),
    (lambda nodes, i: nodes.Wishart(4, 5.0, np.eye(4)) if i == 2 else nodes.Gamma(4, 1.0, 1.0), None, "Wishart"),
    (lambda nodes, i: nodes.Wishart(4, 5.0, np.eye(4)), None, "Wishart"),
], ids=["gamma+diagonal_gamma", "gamma+constant", "shared", "further_child", "one_wishart", "all_wishart"])
def test_describe_pca_declines_malformed_parents_with_a_reason(parent_of, extra, reason):
    from pyvb_amd import _recognise
    g = _graph(parent_of, extra=extra)
    with pytest.raises(NotImplementedError) as e:
        _recognise.describe_pca(g["W"])
    assert reason in str(e.value), str(e.value)
