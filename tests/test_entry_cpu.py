"""CPU: DiagonalGamma precision parents for the columns of A and C, one precision per entry (pyvb_lds_set_entry_precisions) -- what
needs no device.

1. tests/entry_ref.py, the composition of oracle functions that the GPU tests compare against, reproduces the reference's own run
   of such graphs (tests/golden/entry_*.npz, written by tests/golden/make_golden_entry.py) at 1e-10 relative, tests/test_ard_cpu.py's
   figure.
2. On the cases the device is measured on, the float64 comparator lies within the guard of DESIGN.md section 17 of its own
   extended-precision run: e64 <= 1e-11 on every quantity and every part of both bounds, after every iteration of that run (two;
   one at D = K = 64); no column's 1/2 ln det qprec is near the pole of q_ln_det (quirk Q1) on any of them.
3. The exact bound, whose terms for these nodes the reference cannot pin, never decreases over 30 iterations in long double.
4. The yardstick of section 17 sees one entry's variance entering qb scaled by 1 + 1e-10; a tolerance of 1e-8 does not.
5. The three C ABI entries exist everywhere they must, with the declared signatures, and refuse bad arguments with no device.
"""
import ctypes
import glob
import os
import re
import subprocess

import numpy as np
import pytest

import entry_ref as NR
import extended_ref as ER
from conftest import GOLDEN_DIR
from pyvb_amd import _capi, synth
from test_oracle_golden import _close, _close_qld, RTOL

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("pyvb_lds_set_entry_precisions", "pyvb_lds_get_entry_precisions", "pyvb_lds_update_entry_precisions")
ENTRY = sorted(glob.glob(os.path.join(GOLDEN_DIR, "entry_*.npz")))


def test_the_four_fixtures_are_present():
    assert [os.path.basename(p) for p in ENTRY] == ["entry_d3k4_t12.npz", "entry_knowns_d3k4_t15.npz", "entry_mixed_d2k5_t20.npz",
                                                    "entry_tied_d3k4.npz"]
    assert RTOL == 1e-10
    for p in ENTRY:
        assert os.path.getsize(p) < 16384


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
    for w, e in m.entry.items():
        assert e["qb"].shape == z[tag + w + "_entry_b"].shape == (m.D, NR.ROWS[w](m.D, m.K))
        assert np.array_equal(e["qa"], z[tag + w + "_entry_a"]), tag + w + ": qa = a0 + 1 / 2"
        _close(e["qb"], z[tag + w + "_entry_b"], tag + w + "_entry_b")
    ref = z[tag + "elbo_parts"]
    print(tag, "parts", parts, "reference", ref)
    _close(parts, ref, tag + "elbo_parts")
    assert abs(parts.sum() - ref.sum()) <= RTOL * abs(ref.sum())


@pytest.mark.parametrize("path", ENTRY, ids=lambda p: os.path.basename(p)[6:-4])
def test_entry_ref_reproduces_the_reference(path):
    meta, Y, st0, pri, lengths, z = NR.load_entry(path)
    (rows, m), = NR.models(Y, st0, pri, lengths, [0] * len(lengths))
    assert sorted(m.entry) == sorted(meta["which"]) and sorted(m.alpha) == sorted(meta["gamma"])
    assert meta["iters"] == [1, 2, 5]
    for it in range(1, 6):
        parts = m.iterate()
        if it in meta["iters"]:
            _check(m, parts, z, "it%d_" % it, lengths)


def test_the_fixtures_cover_what_they_are_for():
    metas = {os.path.basename(p)[6:-4]: NR.load_entry(p) for p in ENTRY}
    assert (metas["d3k4_t12"][0]["which"], metas["d3k4_t12"][0]["noise"]) == ("AC", "diagonal_gamma")
    mixed = metas["mixed_d2k5_t20"][0]
    assert (mixed["which"], mixed["gamma"], mixed["noise"]) == ("C", "A", "gamma")
    assert metas["tied_d3k4"][0]["lengths"] == [9, 5]
    meta, Y, st0, pri, lengths, z = metas["knowns_d3k4_t15"]
    known = ~np.isnan(pri["A_obs"])
    assert known[:, 0].all() and 0 < known[:, 1].sum() < 3 and not known[:, 2].any()
    # the parents of a fully known column still update (DiagonalGamma.update does not look at `observed`): V = 0, M = the value
    want = pri["A_entry_b0"][0] + 0.5 * (pri["A_obs"][:, 0] - pri["A_prior_mean"][:, 0]) ** 2
    assert np.all(np.abs(z["it1_A_entry_b"][0] - want) <= 1e-12 * want)
    assert np.all(z["it1_A_entry_b"][0] != z["init_A_entry_b"][0])
    # every a0, b0 and qb differs from entry to entry
    for meta, Y, st0, pri, lengths, z in metas.values():
        for w in meta["which"]:
            for a in (pri[w + "_entry_a0"], pri[w + "_entry_b0"], z["init_" + w + "_entry_b"]):
                assert np.unique(a).size == a.size


def test_without_parents_the_comparator_is_ard_ref():
    import ard_ref as AR
    Y, st0, pri = synth.make_problem(9, 3, 4, 2, seed=5)
    AR.add_hyperpriors(st0, pri, "A", 6)
    for (_, a), (_, b) in zip(NR.models(Y, st0, pri), AR.models(Y, st0, pri)):
        for _ in range(2):
            assert np.array_equal(a.iterate(), b.iterate())


def test_pad_series_carries_the_entry_state():
    """from_series / from_trials go through pad_series: qb of the DiagonalGamma parents travels with every series' state."""
    from pyvb_amd.lds import pad_series
    Y, st0, pri, ln, md = NR.tied_problem()
    series = [(Y[n, :Tn], {k: (v[n:n + 1, :Tn] if k == "X" else v[n:n + 1]) for k, v in st0.items()}) for n, Tn in enumerate(ln)]
    Yp, sp, lp = pad_series(series)
    assert sorted(sp) == sorted(st0) and list(lp) == list(ln) and "C_entry_b" in sp
    for k in st0:
        assert np.array_equal(sp[k], st0[k]), k
    plain = [(y, {k: v for k, v in s.items() if not k.endswith("_entry_b")}) for y, s in series]
    assert not any(k.endswith("_entry_b") for k in pad_series(plain)[1])


# ---- 2. the float64 comparator against its extended-precision run -----------------------------------------------------------
@pytest.mark.parametrize("name", sorted(NR.CASES))
def test_float64_comparator_is_inside_the_guard(name):
    (f64, hld64), (ext, hldx) = NR.trace(name), NR.trace(name, extended=True)
    assert ext[0][0]["X"].dtype == ER.LD
    assert len(f64) == NR.ITERS and len(ext) == NR.CASES[name][7] == (1 if name == "d64k64_AC" else NR.ITERS)
    for it, ((s64, p64), (sx, px)) in enumerate(zip(f64, ext)):
        assert sorted(s64) == sorted(sx) and any(k.endswith("_entry_b") for k in sx)
        for k in sx:
            e = ER.rel(s64[k], sx[k])
            print("iteration %d %-10s e64 %.2e" % (it + 1, k, e))
            assert e <= ER.CAP, (name, it, k, e)
        for mode in NR.BOUNDS:
            e = ER.bound_errors(p64[mode], px[mode])[0].max()
            print("iteration %d bound %-9s e64 %.2e" % (it + 1, mode, e))
            assert e <= ER.CAP, (name, it, mode, e)
    # quirk Q1: q_ln_det = 1/2 / (1/2 ln det qprec) has a pole where a column's 1/2 ln det qprec passes through 0
    print("min |1/2 ln det qprec| of a column: %.3f (float64), %.3f (long double)" % (hld64, hldx))
    assert min(hld64, hldx) >= 0.25


def test_tied_problem_is_clear_of_the_pole():
    Y, st0, pri, ln, md = NR.tied_problem()
    for rows, m in NR.models(Y, st0, pri, ln, md):
        for _ in range(NR.ITERS):
            m.iterate()
            assert m.half_lndet_qprec() >= 0.25


# ---- 3. the exact bound ----------------------------------------------------------------------------------------------------
def test_exact_bound_never_decreases_in_long_double():
    """The only check of the exact-mode terms that the reference cannot pin: a mis-derived term of the new nodes breaks the
    monotonicity every update of a variational family guarantees for E_q[ln p] - E_q[ln q]."""
    Y, st0, pri = NR.problem("d3k4_AC")
    (_, m) = NR.models(ER.to_long(Y), ER.to_long(st0), ER.to_long(pri))[0]
    tot = [m.iterate("exact").sum() for _ in range(30)]
    assert tot[0].dtype == ER.LD
    steps = np.diff(np.array(tot, dtype=ER.LD))
    print("exact bound: first %.6f last %.6f smallest step %.3e" % (tot[0], tot[-1], steps.min()))
    assert np.all(steps >= -1e-15 * np.abs(np.array(tot[1:], dtype=ER.LD)))
    assert tot[-1] > tot[0]


# ---- 4. the yardstick sees a wrong sum --------------------------------------------------------------------------------------
def test_a_wrong_variance_term_is_caught_by_the_yardstick_and_missed_at_1e_8():
    """One entry's variance enters qb scaled by 1 + 1e-10.  That moves that qb by 1e-10 times the share s of 1/2 V in it, and the
    rule of section 17 resolves nothing below 16 n 2^-52 = 2.5e-14 at n = 7; qb is compared in the max-norm, so the entry must also
    carry the largest qb or close to it.  The initial noise rates are raised 1e4-fold: the first column update then leaves
    variances that are a visible share of every qb; the entry with the largest share times qb is the one that is scaled."""
    name = "d3k4_AC"
    T, D, K = NR.CASES[name][:3]
    Y, st0, pri = NR.problem(name)
    st0 = dict(st0, Q_b=st0["Q_b"] * 1e4, R_b=st0["R_b"] * 1e4)
    clean = NR.models(Y, st0, pri)
    for _, m in clean:
        m.iterate()
    m0 = clean[0][1]
    V = np.einsum("ikk->ik", m0.chains[0]["C_cov"][0])
    i, k = np.unravel_index(np.argmax(0.5 * V), V.shape)
    share = 0.5 * V[i, k] / m0.entry["C"]["qb"][i, k]
    scale = np.ones((D, K)); scale[i, k] = 1.0 + 1e-10
    runs = {}
    for nm, cast, vs in (("f64", lambda v: v, None), ("ext", ER.to_long, None), ("mutant", lambda v: v, {"C": scale})):
        ms = NR.models(cast(Y), cast(st0), cast(pri), vscale=vs)
        for _, m in ms:
            m.iterate()
        runs[nm] = ms[0][1].entry["C"]["qb"]
    assert runs["ext"].dtype == ER.LD
    weight = runs["f64"][i, k] / runs["f64"].max()
    e64, e = ER.rel(runs["f64"], runs["ext"]), ER.rel(runs["mutant"], runs["ext"])
    y = ER.yardstick(e64, max(T, D, K))
    print("share of the variance in qb[%d][%d] %.3f, that qb / max qb %.3f; e64 %.3e, mutant %.3e, yardstick %.3e, ratio %.1f"
          % (i, k, share, weight, e64, e, y, e / y))
    assert share * weight > 0.01, (share, weight)
    assert e64 <= ER.CAP and e64 <= ER.FACTOR * y       # the clean comparator passes the rule
    assert e > ER.FACTOR * y                             # the rule rejects the mutant
    assert e < 1e-8                                      # the parity tolerance would have let it pass


# ---- 5. the C ABI -----------------------------------------------------------------------------------------------------------
def test_entries_are_declared_exported_and_bound():
    header = open(os.path.join(REPO, "include", "pyvb_hip.h")).read()
    decl = {
        ENTRIES[0]: r"int pyvb_lds_set_entry_precisions\(pyvb_lds\* h, int which, const double\* a0, const double\* b0, const double\* qb\);",
        ENTRIES[1]: r"int pyvb_lds_get_entry_precisions\(pyvb_lds\* h, int which, double\* qa, double\* qb\);",
        ENTRIES[2]: r"int pyvb_lds_update_entry_precisions\(pyvb_lds\* h, int which\);",
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
    assert _capi.lib.pyvb_version() >= 107


def test_argument_checks_need_no_device():
    """A NULL handle is refused by all three; so is `which` outside {0, 1}, before the handle is read (tests/test_converge_cpu.py: the
    handle behind `fake` is never dereferenced by a check that fails first)."""
    v = np.ones(4)
    p = _capi.dptr(v)
    lib = _capi.lib
    for rc in (lib.pyvb_lds_set_entry_precisions(None, 0, p, p, p), lib.pyvb_lds_get_entry_precisions(None, 0, p, p),
               lib.pyvb_lds_update_entry_precisions(None, 1)):
        assert rc == _capi.E_ARG
        assert b"handle is NULL" in lib.pyvb_last_error()
    buf = ctypes.create_string_buffer(1 << 16)      # zeroed, larger than a handle: every flag false, every pointer null
    fake = ctypes.c_void_p(ctypes.addressof(buf))
    for which in (-1, 2):
        for rc in (lib.pyvb_lds_set_entry_precisions(fake, which, p, p, p), lib.pyvb_lds_get_entry_precisions(fake, which, p, p),
                   lib.pyvb_lds_update_entry_precisions(fake, which)):
            assert rc == _capi.E_ARG
            assert b"which must be 0 (A) or 1 (C)" in lib.pyvb_last_error()
    # a matrix without DiagonalGamma parents: get and update are argument errors before anything is copied or launched
    for which, nm in ((0, b"A"), (1, b"C")):
        assert lib.pyvb_lds_get_entry_precisions(fake, which, p, p) == _capi.E_ARG
        assert b"columns of " + nm + b" have no DiagonalGamma precision parents" in lib.pyvb_last_error()
        assert lib.pyvb_lds_update_entry_precisions(fake, which) == _capi.E_ARG


def test_python_layer_has_the_three_methods():
    from pyvb_amd.lds import LDSBatch
    for name in ("set_entry_precisions", "entry_precisions", "update_entry_precisions"):
        assert callable(getattr(LDSBatch, name))
