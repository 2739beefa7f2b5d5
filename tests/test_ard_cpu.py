"""CPU: Gamma precision parents for the columns of A and C (pyvb_lds_set_column_precisions) -- what needs no device.

1. tests/ard_ref.py, the composition of oracle functions that the GPU tests compare against, reproduces the reference's own run
   of such graphs (tests/golden/ard_*.npz, written by tests/golden/make_golden_ard.py) at 1e-10 relative, the figure
   tests/test_tied_cpu.py holds tests/tied_ref.py to against its fixtures.
2. On the cases the device is measured on, the float64 comparator lies within the guard of DESIGN.md section 17 of its own
   extended-precision run: e64 <= 1e-11 on every quantity and every part of both bounds, after every iteration of that run (two;
   one at D = K = 64, where a long-double iteration takes seconds).
3. The three C ABI entries exist everywhere they must, with the declared signatures; a NULL handle is an argument error.
"""
import glob
import os
import re
import subprocess

import numpy as np
import pytest

import ard_ref as AR
import extended_ref as ER
from conftest import GOLDEN_DIR
from pyvb_amd import _capi
from test_oracle_golden import _close, _close_qld, RTOL

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("pyvb_lds_set_column_precisions", "pyvb_lds_get_column_precisions", "pyvb_lds_update_column_precisions")
ARD = sorted(glob.glob(os.path.join(GOLDEN_DIR, "ard_*.npz")))


def test_the_four_fixtures_are_present():
    assert [os.path.basename(p) for p in ARD] == ["ard_d3k4_t12.npz", "ard_gamma_d2k5_t20.npz", "ard_knowns_d3k4_t15.npz",
                                                  "ard_tied_d3k4.npz"]
    assert RTOL == 1e-10


# ---- 1. the comparator against the reference --------------------------------------------------------------------------------
def _check(m, parts, z, tag, lengths):
    for n, (st, Tn) in enumerate(zip(m.chains, lengths)):
        what = "%schain %d " % (tag, n)
        _close(st["X"][0], z[tag + "X"][n, :Tn], what + "X")
        cls = [0, 1, 2] if Tn > 2 else [0, 2]
        _close(st["Sigma"][0][cls], z[tag + "Sigma"][n][cls], what + "Sigma")
        _close_qld(st["qld_x"][0][cls], z[tag + "qld_x"][n][cls], what + "qld_x")
    st = m.chains[0]
    _close(st["A_mean"][0], z[tag + "A_mean"], tag + "A_mean")
    _close(st["C_mean"][0], z[tag + "C_mean"], tag + "C_mean")
    for nm in ("A", "C"):
        _close(np.einsum("ikk->ik", st[nm + "_cov"][0]), z[tag + nm + "_colvar"], tag + nm + "_colvar")
        assert z[tag + nm + "_cov_offdiag_max"] == 0.0         # the columns stay diagonal: lane = row survives
        _close_qld(st["qld_" + nm][0], z[tag + "qld_" + nm], tag + "qld_" + nm)
    for nm in ("Q_a", "Q_b", "R_a", "R_b"):
        _close(st[nm][0], z[tag + nm], tag + nm)
    for w, al in m.alpha.items():
        assert np.array_equal(al["qa"], z[tag + w + "_alpha_a"]), tag + w + ": qa = a0 + rows / 2"
        _close(al["qb"], z[tag + w + "_alpha_b"], tag + w + "_alpha_b")
    ref = z[tag + "elbo_parts"]
    print(tag, "parts", parts, "reference", ref)
    _close(parts, ref, tag + "elbo_parts")
    assert abs(parts.sum() - ref.sum()) <= RTOL * abs(ref.sum())


@pytest.mark.parametrize("path", ARD, ids=lambda p: os.path.basename(p)[4:-4])
def test_ard_ref_reproduces_the_reference(path):
    meta, Y, st0, pri, lengths, z = AR.load_ard(path)
    (rows, m), = AR.models(Y, st0, pri, lengths, [0] * len(lengths))
    assert sorted(m.alpha) == sorted(meta["which"])
    assert meta["iters"] == [1, 2, 5]
    for it in range(1, 6):
        parts = m.iterate()
        if it in meta["iters"]:
            _check(m, parts, z, "it%d_" % it, lengths)


def test_the_knowns_fixture_has_a_fully_and_a_partly_known_column():
    meta, Y, st0, pri, lengths, z = AR.load_ard(os.path.join(GOLDEN_DIR, "ard_knowns_d3k4_t15.npz"))
    known = ~np.isnan(pri["A_obs"])
    assert known[:, 0].all() and 0 < known[:, 1].sum() < 3 and not known[:, 2].any()
    # a fully known column's alpha still updates (Gamma.update does not look at `observed`): V = 0, M = the value
    want = pri["A_alpha_b0"][0] + 0.5 * ((pri["A_obs"][:, 0] - pri["A_prior_mean"][:, 0]) ** 2).sum()
    assert abs(z["it1_A_alpha_b"][0] - want) <= 1e-12 * want
    assert z["it1_A_alpha_b"][0] != z["init_A_alpha_b"][0]


def test_without_hyperpriors_the_comparator_is_tied_ref():
    import tied_ref as TR
    from pyvb_amd import synth
    Y, st0, pri = synth.make_problem(9, 3, 4, 2, seed=5)
    (_, m0), (_, m1) = AR.models(Y, st0, pri)
    chains = TR.make_model([Y[1:2]], [{k: v[1:2] for k, v in st0.items()}], pri)
    for _ in range(2):
        assert np.array_equal(m1.iterate(), TR.iterate(chains, pri, [Y[1:2]]))


def test_pad_series_carries_the_alpha_state():
    """from_series / from_trials go through pad_series: qb of the columns' Gamma parents travels with every series' state."""
    from pyvb_amd.lds import pad_series
    Y, st0, pri, ln, md = AR.tied_problem()
    series = [(Y[n, :Tn], {k: (v[n:n + 1, :Tn] if k == "X" else v[n:n + 1]) for k, v in st0.items()}) for n, Tn in enumerate(ln)]
    Yp, sp, lp = pad_series(series)
    assert sorted(sp) == sorted(st0) and list(lp) == list(ln)
    for k in st0:
        assert np.array_equal(sp[k], st0[k]), k
    assert np.array_equal(Yp, Y)
    plain = [(y, {k: v for k, v in s.items() if not k.endswith("_alpha_b")}) for y, s in series]
    assert not any(k.endswith("_alpha_b") for k in pad_series(plain)[1])


# ---- 2. the float64 comparator against its extended-precision run -----------------------------------------------------------
@pytest.mark.parametrize("name", sorted(AR.CASES))
def test_float64_comparator_is_inside_the_guard(name):
    f64, ext = AR.trace(name), AR.trace(name, extended=True)
    assert ext[0][0]["X"].dtype == ER.LD
    assert len(f64) == AR.ITERS and len(ext) == AR.CASES[name][6] == (1 if name == "d64k64_AC" else AR.ITERS)
    for it, ((s64, p64), (sx, px)) in enumerate(zip(f64, ext)):
        for k in sx:
            e = ER.rel(s64[k], sx[k])
            print("iteration %d %-10s e64 %.2e" % (it + 1, k, e))
            assert e <= ER.CAP, (name, it, k, e)
        for mode in AR.BOUNDS:
            e = ER.bound_errors(p64[mode], px[mode])[0].max()
            print("iteration %d bound %-9s e64 %.2e" % (it + 1, mode, e))
            assert e <= ER.CAP, (name, it, mode, e)


# ---- 3. the C ABI -----------------------------------------------------------------------------------------------------------
def test_entries_are_declared_exported_and_bound():
    header = open(os.path.join(REPO, "include", "pyvb_hip.h")).read()
    decl = {
        "pyvb_lds_set_column_precisions": r"int pyvb_lds_set_column_precisions\(pyvb_lds\* h, int which, const double\* a0, const double\* b0, const double\* qb\);",
        "pyvb_lds_get_column_precisions": r"int pyvb_lds_get_column_precisions\(pyvb_lds\* h, int which, double\* qa, double\* qb\);",
        "pyvb_lds_update_column_precisions": r"int pyvb_lds_update_column_precisions\(pyvb_lds\* h, int which\);",
    }
    c, dp, h = _capi.ctypes.c_int, _capi._dp, _capi._h
    args = {ENTRIES[0]: [h, c, dp, dp, dp], ENTRIES[1]: [h, c, dp, dp], ENTRIES[2]: [h, c]}
    for name in ENTRIES:
        assert re.search("^" + decl[name], header, re.M), name + " is not declared as specified in include/pyvb_hip.h"
        assert _capi.SIGNATURES[name] == (c, args[name]), name
        assert getattr(_capi.lib, name).argtypes == args[name]
    out = subprocess.run(["nm", "-D", "--defined-only", _capi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert set(ENTRIES) <= exported
    assert _capi.lib.pyvb_version() >= 105


def test_a_null_handle_is_an_argument_error():
    v = np.ones(4)
    p = _capi.dptr(v)
    for rc in (_capi.lib.pyvb_lds_set_column_precisions(None, 0, p, p, p), _capi.lib.pyvb_lds_get_column_precisions(None, 0, p, p),
               _capi.lib.pyvb_lds_update_column_precisions(None, 1)):
        assert rc == _capi.E_ARG
        assert b"handle is NULL" in _capi.lib.pyvb_last_error()
