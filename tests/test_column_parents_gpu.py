"""GPU: the one record of the columns' precision parents (pyvb_amd/csrc/column_parents.h) behind LDS and VB-PCA handles.  A handle
taken through several kinds of parent computes, bit for bit, what a fresh handle computes that was only ever given the final ones:
nothing of an earlier kind -- its block stays allocated -- leaks into the launches.  Shapes for the tails: D = 3 columns against
k_entry's four per pass, rows != D, a tied model; q = 3, d = 5 with missing entries.  profiles/column_parents_dump.py dumps the same
problems for the comparison of two builds.
"""
import numpy as np
import pytest

from pyvb_amd import synth

LDS_SHAPE = dict(N=3, T=6, D=3, K=5, models=[0, 0, 1])
PCA_SHAPE = dict(N=7, d=5, q=3)
MODES = ("reference", "exact")


def lds_problem():
    """(Y, st0, pri, models) and the hyperpriors {"gamma": {"A", "C"}, "diagonal_gamma": {"A", "C"}}, each (a0, b0, qb), all distinct"""
    s = LDS_SHAPE
    Y, st0, pri = synth.make_problem(s["T"], s["D"], s["K"], s["N"], seed=31)
    rng = np.random.default_rng(32)
    draw = lambda *shape: 0.2 + rng.random(shape)
    hyper = {"gamma": {}, "diagonal_gamma": {}}
    for w, rows in (("A", s["D"]), ("C", s["K"])):
        hyper["gamma"][w] = (draw(s["D"]), draw(s["D"]), draw(s["N"], s["D"]))
        hyper["diagonal_gamma"][w] = (draw(s["D"], rows), draw(s["D"], rows), draw(s["N"], s["D"], rows))
    return Y, st0, pri, np.array(s["models"], dtype=np.int32), hyper


def pca_problem():
    """(init, pri) with four missing entries, one row without any, and the hyperpriors {"gamma", "diagonal_gamma"}, each (a0, b0, qb)"""
    s = PCA_SHAPE
    init, pri = synth.pca_problem(s["N"], s["d"], s["q"], seed=41)
    obs = np.ones((s["N"], s["d"]), dtype=bool)
    obs[1, 2] = obs[4, 0] = obs[4, 4] = obs[6, 3] = False
    init = dict(init, obs=obs, X=np.where(obs, init["X"], 0.1))
    rng = np.random.default_rng(42)
    draw = lambda *shape: 0.2 + rng.random(shape)
    hyper = {"gamma": tuple(draw(s["q"]) for _ in range(3)), "diagonal_gamma": tuple(draw(s["q"], s["d"]) for _ in range(3))}
    return init, pri, hyper


def lds_outputs(b):
    """Every array of get_state(), column_precisions(), entry_precisions() and the parts of the bound, by name"""
    out = dict(b.get_state())
    for name, got in (("column", b.column_precisions()), ("entry", b.entry_precisions())):
        for w, (qa, qb) in got.items():
            out["%s_%s_qa" % (name, w)], out["%s_%s_qb" % (name, w)] = qa, qb
    out["elbo"] = b.elbo()
    return out


def pca_outputs(b, kind):
    out = {k: np.asarray(v) for k, v in b.get_state().items()}
    if kind != "constant":
        out["parent_qa"], out["parent_qb"] = b.column_precisions() if kind == "gamma" else b.entry_precisions()
    out["elbo"] = b.elbo()
    return out


def _same(a, b, tag):
    assert sorted(a) == sorted(b), tag
    for k in a:
        assert np.array_equal(a[k], b[k]), "%s: %s differs" % (tag, k)


@pytest.mark.gpu
def test_lds_handle_taken_through_the_kinds_equals_a_fresh_one():
    from pyvb_amd.lds import LDSBatch
    Y, st0, pri, models, hyper = lds_problem()
    other = {k: {w: tuple(v + 0.5 for v in t) for w, t in d.items()} for k, d in hyper.items()}      # what the earlier setters give
    b = LDSBatch.from_problem(Y, st0, pri, models=models)
    steps = [(lambda: None, ("constant", "constant")),
             (lambda: b.set_entry_precisions(C=other["diagonal_gamma"]["C"]), ("constant", "diagonal_gamma")),
             (lambda: b.set_priors(pri), ("constant", "constant")),
             (lambda: b.set_column_precisions(A=other["gamma"]["A"]), ("gamma", "constant")),
             (lambda: b.set_entry_precisions(A=other["diagonal_gamma"]["A"]), ("diagonal_gamma", "constant")),
             (lambda: b.set_entry_precisions(C=hyper["diagonal_gamma"]["C"]), ("diagonal_gamma", "diagonal_gamma")),
             (lambda: b.set_column_precisions(A=hyper["gamma"]["A"]), ("gamma", "diagonal_gamma"))]
    for i, (step, want) in enumerate(steps):
        step()
        assert b.column_parents() == {"A": want[0], "C": want[1]}, i
    fresh = LDSBatch.from_problem(Y, st0, pri, models=models)
    fresh.set_column_precisions(A=hyper["gamma"]["A"])
    fresh.set_entry_precisions(C=hyper["diagonal_gamma"]["C"])
    assert fresh.column_parents() == b.column_parents()
    for mode in MODES:
        for h in (b, fresh):
            h.set_bound_mode(mode)
            h.iterate(2)
        got = lds_outputs(b)
        assert sorted(k for k in got if k.endswith("_qb")) == ["column_A_qb", "entry_C_qb"]
        assert got["entry_C_qb"].shape == (3, 3, 5) and np.all(np.isfinite(got["elbo"]))
        _same(got, lds_outputs(fresh), mode)
    b.close(); fresh.close()


@pytest.mark.gpu
def test_pca_handle_taken_through_the_kinds_equals_a_fresh_one():
    from pyvb_amd.pca import PCABatch
    init, pri, hyper = pca_problem()
    b = PCABatch.from_problem(init, pri)
    steps = [(lambda: None, "constant"),
             (lambda: b.set_column_precisions(*[v + 0.5 for v in hyper["gamma"]]), "gamma"),
             (lambda: b.set_entry_precisions(*hyper["diagonal_gamma"]), "diagonal_gamma"),
             (lambda: b.set_priors(pri), "constant"),
             (lambda: b.set_column_precisions(*hyper["gamma"]), "gamma")]
    for i, (step, want) in enumerate(steps):
        step()
        assert b.column_parents() == want, i
    fresh = PCABatch.from_problem(dict(init), dict(pri, W_alpha=hyper["gamma"]))
    assert fresh.column_parents() == "gamma"
    for mode in MODES:
        for h in (b, fresh):
            h.set_bound_mode(mode)
            h.iterate(2)
        got = pca_outputs(b, "gamma")
        assert np.all(np.isfinite(got["elbo"])) and np.all(got["parent_qb"] != hyper["gamma"][2])
        _same(got, pca_outputs(fresh, "gamma"), mode)
    b.close(); fresh.close()


@pytest.mark.gpu
def test_update_none_serves_exactly_the_matrices_of_its_kind_and_the_other_getters_refuse():
    """A: Gamma, C: DiagonalGamma.  Before any iteration the rates are the caller's, so an update shows."""
    from pyvb_amd import _capi
    from pyvb_amd.lds import LDSBatch
    Y, st0, pri, models, hyper = lds_problem()
    b = LDSBatch.from_problem(Y, st0, pri, models=models)
    b.set_column_precisions(A=hyper["gamma"]["A"])
    b.set_entry_precisions(C=hyper["diagonal_gamma"]["C"])
    first = lambda a: a[[0, 0, 2]]          # a model's rate is its first replicate's
    col, ent = b.column_precisions(), b.entry_precisions()
    assert list(col) == ["A"] and list(ent) == ["C"]
    assert np.array_equal(col["A"][1], first(hyper["gamma"]["A"][2])) and np.array_equal(ent["C"][1], first(hyper["diagonal_gamma"]["C"][2]))
    assert np.array_equal(col["A"][0], np.broadcast_to(hyper["gamma"]["A"][0] + 1.5, (3, 3)))       # a0 + rows / 2, rows = D = 3
    assert np.array_equal(ent["C"][0], np.broadcast_to(hyper["diagonal_gamma"]["C"][0] + 0.5, (3, 3, 5)))
    b.update_column_precisions()            # None: every matrix with Gamma parents -- A alone
    assert np.all(b.column_precisions()["A"][1] != col["A"][1]) and np.array_equal(b.entry_precisions()["C"][1], ent["C"][1])
    col = b.column_precisions()
    b.update_entry_precisions()             # None: every matrix with DiagonalGamma parents -- C alone
    assert np.all(b.entry_precisions()["C"][1] != ent["C"][1]) and np.array_equal(b.column_precisions()["A"][1], col["A"][1])
    refusals = [(lambda: b.update_column_precisions("C"), "the columns of C have DiagonalGamma precision parents, one per entry: "
                 "pyvb_lds_get_entry_precisions / pyvb_lds_update_entry_precisions serve them"),
                (lambda: b.update_entry_precisions("A"), "the columns of A have no DiagonalGamma precision parents: no per-entry "
                 "hyperpriors were given (pyvb_lds_set_entry_precisions)")]
    buf = np.empty((3, 3, 5))
    p = _capi.dptr(buf)
    refusals += [(lambda: _capi.check(_capi.lib.pyvb_lds_get_column_precisions(b._h, 1, p, p)), refusals[0][1]),
                 (lambda: _capi.check(_capi.lib.pyvb_lds_get_entry_precisions(b._h, 0, p, p)), refusals[1][1])]
    for call, text in refusals:
        with pytest.raises(_capi.PyvbHipError) as e:
            call()
        assert e.value.code == _capi.E_ARG and text in str(e.value), str(e.value)
    b.set_priors(pri)
    assert b.column_precisions() == {} and b.entry_precisions() == {}
    with pytest.raises(_capi.PyvbHipError) as e:
        b.update_column_precisions("C")
    assert "the columns of C have Constant precision parents: no hyperpriors were given (pyvb_lds_set_column_precisions)" in str(e.value)
    b.update_column_precisions(); b.update_entry_precisions()      # None with nothing to serve: no call, no error
    b.close()
