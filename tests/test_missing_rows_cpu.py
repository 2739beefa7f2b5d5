"""CPU: the reference side of tests/test_missing_rows_gpu.py, alone.

  * the row patterns are what they are named (extended_ref._missing_rows);
  * for every (case, iteration, row, quantity) the GPU file compares row by row, the float64 oracle is within CAP = 1e-11 of the
    long-double run in the row's own unit -- so the bound 16 max(e64_row, n 2^-52) never exceeds 1.6e-10 of a row's largest
    missing entry -- and the whole-array quantities and the parts of the bound of the orders only that file runs are within it too;
  * before the first update_Y the reference's bound is NaN in both oracles (the GPU file does not compare the handle's there);
  * extended_ref.compare_rows, fed a float64 oracle run with one defect planted in update_Y, flags exactly the rows concerned,
    and none of the unmutated run.
"""
import numpy as np
import pytest

import extended_ref as E

LD = np.longdouble

ROW_CASES = E.ROWS_ENVELOPE + ["t7_d65_k128_rows_big", "t11_d9_k128_rows_big"]
ORDER = (False, True)           # outputs never updated in the first iteration, updated in the second
ORDER_CASES = ["t11_d5_k9_wishart_rows", "t11_d6_k64_wishart_rows", "t11_d12_k100_rows_big"]
DEFAULT_CASES = ["t11_d5_k9_wishart_rows", "t11_d12_k100_rows_big"]


@pytest.mark.parametrize("K", [2, 9, 33, 64, 70, 128])
def test_row_patterns_are_what_they_are_named(K):
    T = 23
    mask, names = E._missing_rows(T, K, np.random.default_rng(0))
    assert mask.shape == (T, K) and mask.dtype == bool and len(names) == T
    table = list(E.ROW_PATTERNS)
    if K > 64:
        for i, nm in E.ROW_PATTERNS_BIG.items():
            table[i] = nm
    assert names == [table[t % 11] for t in range(T - 1)] + ["all"]
    assert names[0] == names[-1] == names[10] == names[11] == "all"
    k = np.arange(K)
    for t, nm in enumerate(names):
        m = mask[t]
        if nm == "all":
            assert m.all()
        elif nm == "one known, first":
            assert not m[0] and m[1:].all()
        elif nm == "one known, last":
            assert not m[-1] and m[:-1].all()
        elif nm == "one missing, first":
            assert m[0] and not m[1:].any()
        elif nm == "one missing, last":
            assert m[-1] and not m[:-1].any()
        elif nm == "a tile":
            assert np.array_equal(np.nonzero(m)[0], np.arange(min(8, K - 1)))
        elif nm == "alternating":
            assert np.array_equal(m, k % 2 == 0)
        elif nm == "upper half":
            assert np.array_equal(m, k >= K // 2)
        elif nm == "observed":
            assert not m.any()
        elif nm == "low half":
            assert np.array_equal(np.nonzero(m)[0], np.arange(64))
        elif nm == "high half":
            assert np.array_equal(np.nonzero(m)[0], np.arange(64, K))
        elif nm == "the seam":
            assert np.array_equal(np.nonzero(m)[0], [63, 64])
        else:
            assert nm == "Bernoulli"


def test_cases_carry_the_patterns():
    for name in ROW_CASES:
        c = E.lds_case(name)
        N, T, K = c["Y"].shape
        miss = np.isnan(c["Y"])
        assert miss[0, 0].all() and miss[0, T - 1].all(), name          # the ends of the chain are unobserved
        assert len(c["patterns"]) == N and all(len(p) == T for p in c["patterns"])
        assert c["st0"]["Yq"].shape == (N, T, K) and c["st0"]["Yrowvar"].shape == (N, T)
        if N == 2:              # a replicate with almost nothing to do beside a full one
            assert miss[1].sum() == 1 and miss[1, 2, 1]
    assert E.lds_case("t11_d6_k64_wishart_rows")["Y"].shape[2] == 64
    for name in ("t11_d12_k100_rows_big", "t11_d9_k128_rows_big"):
        assert set(E.lds_case(name)["patterns"][0]) >= {"low half", "high half", "the seam"}
    for name in E.ROWS_ENVELOPE:
        assert not E.LDS_CASES[name][1] and name in E.EXACT_BOUND_CASES and E.lds_case(name)["iters"] == 2


def _check_rows_within_cap(tag, ref, c):
    its = E.row_iterations(ref["updates"])
    assert its, tag
    seen = 0
    for key in sorted(ref["rows"]):
        if key[0] not in its:
            continue
        e = ref["rows"][key]
        has = ref["miss"].any(axis=2)
        assert np.array_equal(np.isnan(e), ~has), (tag, key)
        r, t = np.unravel_index(np.nanargmax(e), e.shape)
        print("%-36s it%d %-4s largest e64_row %.2e (r%d row %d, %s)" % (tag, key[0], key[2], e[r, t], r, t, c["patterns"][r][t]))
        assert np.all(e[has] <= E.CAP), "%s %r: float64 oracle %.3e from the extended run in a row's own unit (r%d row %d, %s), cap %.0e" \
            % (tag, key, e[r, t], r, t, c["patterns"][r][t], E.CAP)
        seen += 1
    assert seen == 2 * len(its)


@pytest.mark.parametrize("name", ROW_CASES)
def test_float64_oracle_is_within_the_cap_row_by_row(name):
    ref = E.rows_reference(name)
    assert all(v.dtype == LD for v in ref["ext"].values())
    _check_rows_within_cap(name, ref, E.lds_case(name))
    if name in E.ROWS_ENVELOPE:      # the run is the envelope's own: the same two oracles, the same calls
        (rows, T, n, ext, e64, _, _), = E.lds_reference(name)
        assert n == ref["n"] and set(ext) == set(ref["ext"])
        assert all(np.array_equal(ext[k], ref["ext"][k]) for k in ext) and e64 == ref["e64"]


def _check_whole_arrays_within_cap(tag, ref, skip_bound=()):
    worst = max(ref["e64"], key=ref["e64"].get)
    print("%-36s largest e64 %.2e at %r" % (tag, ref["e64"][worst], worst))
    for key, e in ref["e64"].items():
        assert e <= E.CAP, "%s %r: float64 oracle %.3e from the extended run, cap %.0e" % (tag, key, e, E.CAP)
    for key, (ext, e64, _) in sorted(ref["bound"].items()):
        if key[0] in skip_bound:
            continue
        print("%-36s it%d %-9s " % (tag, key[0], key[2]) + "  ".join("%s %.1e" % (nm, e64[:, p].max()) for p, nm in enumerate(E.LDS_PARTS)))
        assert ext.dtype == LD and np.all(np.isfinite(ext)) and np.all(e64 <= E.CAP), (tag, key, e64)


@pytest.mark.parametrize("name", ORDER_CASES)
def test_outputs_never_updated_then_updated_reference(name):
    """The default order: iterate() leaves the outputs alone.  Every quantity of both iterations within the cap, the rows after
    the one update_Y too, the bound after the second iteration -- and after the first both oracles give NaN (L_Y of a
    replicate that has a row nothing of which is observed: the reference's q_ln_det of such a row does not exist before its first
    update)."""
    ref = E.rows_reference(name, ORDER)
    c = E.lds_case(name)
    assert (0, "outputs kept", "Yq") in ref["ext"] and (1, "update_Y", "Yvar") in ref["ext"]
    assert E.row_iterations(ORDER) == (1,)
    _check_rows_within_cap(name + " kept, updated", ref, c)
    _check_whole_arrays_within_cap(name + " kept, updated", ref, skip_bound=(0,))
    for mode in E.BOUND_MODES:
        ext, e64, _ = ref["bound"][(0, "bound", mode)]
        latent = np.isnan(c["Y"]).all(axis=2).any(axis=1)          # the replicates that have a row nothing of which is observed
        assert latent[0] and np.all(np.isnan(ext[latent, 1])) and np.all(np.isnan(e64[latent, 1])), (mode, ext, e64)
        assert np.all(np.isfinite(np.delete(np.asarray(ext, dtype=float), 1, axis=1))) and np.all(np.isfinite(ext[~latent, 1]))
    run64 = dict(E.lds_float64_rows(name, updates=ORDER))
    assert set(run64) == set(ref["ext"])


@pytest.mark.parametrize("name", DEFAULT_CASES)
def test_default_initial_outputs_reference(name):
    """N(0, I) on the rows that hold NaN, spelled out: one iteration, rows and whole arrays within the cap.  (The oracle needs
    the initial outputs in the state; a handle that is told none is compared with the one that is, bitwise.)"""
    c, d = E.lds_case(name + "_explicit"), E.lds_case(name + "_default")
    has = np.isnan(c["Y"]).any(axis=2)
    assert np.all(c["st0"]["Yq"][has] == 0.0) and np.all(c["st0"]["Yrowvar"] == 1.0) and c["iters"] == d["iters"] == 1
    assert "Yq" not in d["st0"] and "Yrowvar" not in d["st0"] and np.array_equal(np.isnan(d["Y"]), np.isnan(c["Y"]))
    ref = E.rows_reference(name + "_explicit")
    _check_rows_within_cap(name + "_explicit", ref, c)
    _check_whole_arrays_within_cap(name + "_explicit", ref)


# ----------------------------------------------------------------------------------------------------------------------------
# mutants of update_Y
# ----------------------------------------------------------------------------------------------------------------------------
def _miss(c):
    return np.isnan(c["Y"])


def _rows_named(c, pattern):
    return {(r, t) for r, names in enumerate(c["patterns"]) for t, nm in enumerate(names) if nm == pattern}


def _first_partial(c):
    """(row, entry) of replicate 0: the first row with both known and missing entries, its first known entry"""
    m = _miss(c)[0]
    t = int(np.nonzero(m.any(axis=1) & ~m.all(axis=1))[0][0])
    return t, int(np.nonzero(~m[t])[0][0])


def _plant_pin(run, c):
    t, k = _first_partial(c)
    run.st["Yvar"][0, t, k] = 1e-13


def _plant_sign(run, c):
    """qmu_u = pmu_u - gain (y_o - pmu_o) for pmu_u + gain (y_o - pmu_o)"""
    pmu = np.einsum("nkj,ntj->ntk", run.st["C_mean"], run.st["X"])
    for r, t in _rows_named(c, "one known, last"):
        u = _miss(c)[r, t]
        run.st["Yq"][r, t, u] = 2.0 * pmu[r, t, u] - run.st["Yq"][r, t, u]


def _plant_odd(run, c):
    """the variances of an alternating row's (even) missing entries from the pivot set of the odd ones: the j-th of them takes
    the j-th diagonal entry of inv(<R>_oo), o the odd entries (the last one again where the even ones are one more)"""
    K = c["Y"].shape[2]
    Rb = run.O.noise_expect(run.pri["noise"], run.st["R_a"], run.st["R_b"], K)
    odd, even = np.arange(1, K, 2), np.arange(0, K, 2)
    for r, t in _rows_named(c, "alternating"):
        wrong = np.diag(np.linalg.inv(Rb[r][np.ix_(odd, odd)]))
        run.st["Yvar"][r, t, even] = wrong[np.minimum(np.arange(even.size), odd.size - 1)]


def _plant_last(run, c):
    K = c["Y"].shape[2]
    for r, t in zip(*np.nonzero(_miss(c)[:, :, K - 1])):
        run.st["Yq"][r, t, K - 1] = c["st0"]["Yq"][r, t, K - 1]
        run.st["Yvar"][r, t, K - 1] = c["st0"]["Yrowvar"][r, t]


def _plant_64(run, c):
    for r, t in zip(*np.nonzero(_miss(c)[:, :, 64])):
        run.st["Yq"][r, t, 64] = 0.0            # (nan_to_num of the observation)
        run.st["Yvar"][r, t, 64] = 0.0


# name -> (the cases it is planted in, plant(run, case), the rows it concerns).  The first update_Y of a Wishart case meets the
# initial qw, which is diagonal: no regression term, a diagonal covariance, and the two mutants of those are no defect yet.  They
# show after the second update_Y.
ROW_MUTANTS = {
    "a pinned variance of 1e-13 on one known entry":
        (["t11_d5_k9_wishart_rows", "t11_d6_k64_wishart_rows", "t11_d12_k100_rows_big"], _plant_pin, lambda c: {(0, _first_partial(c)[0])}),
    "sign of the regression term on the one-known-last rows":
        (["t11_d5_k9_wishart_rows", "t11_d6_k64_wishart_rows", "t11_d17_k9_wishart_known_rows"], _plant_sign, lambda c: _rows_named(c, "one known, last")),
    "covariance of an alternating row from the odd entries":
        (["t11_d5_k9_wishart_rows", "t11_d6_k64_wishart_rows", "t11_d17_k9_wishart_known_rows"], _plant_odd, lambda c: _rows_named(c, "alternating")),
    "entry K - 1 left at its initial value":
        (["t11_d5_k9_wishart_rows", "t11_d6_k64_wishart_rows", "t3_d17_k33_wishart_rows", "t11_d12_k100_rows_big", "t11_d9_k128_rows_big"],
         _plant_last, lambda c: set(zip(*np.nonzero(_miss(c)[:, :, -1])))),
    "entry 64 treated as observed":
        (["t11_d12_k100_rows_big", "t7_d72_k70_gamma_rows_big", "t11_d9_k128_rows_big"], _plant_64, lambda c: set(zip(*np.nonzero(_miss(c)[:, :, 64])))),
}


@pytest.mark.parametrize("mutant", list(ROW_MUTANTS))
def test_row_comparison_catches_mutants(mutant):
    """compare_rows on the float64 oracle with one defect planted in update_Y (applied after every call of it, so it carries over
    into the next iteration as a kernel's would).  After the first update_Y whose outputs the defect changes, exactly the rows
    concerned are flagged, every one of them; before it none; after a later one they still are, beside whatever the carried-over
    defect has reached.  Every case catches the mutant.  The unmutated oracle is within its own yardstick on every row
    (e_row = e64_row <= y)."""
    cases, plant, concerned = ROW_MUTANTS[mutant]
    for name in cases:
        c = E.lds_case(name)
        want = {(int(r), int(t)) for r, t in concerned(c)}
        assert want, "%s: %s concerns no row" % (mutant, name)

        class Mutant(E.OracleLDS):
            O = E.O

            def update_Y(self):
                E.OracleLDS.update_Y(self)
                plant(self, c)

        run64, runm = E.lds_float64_rows(name), E.lds_float64_rows(name, make=Mutant)
        clean = E.compare_rows(name, run64, tag=name + " float64")
        assert clean and not E.offending_rows(clean) and max(r[6] for r in clean) <= 1.0 + 1e-9
        rows = E.compare_rows(name, runm, tag=name + " mutant")
        differs = {it for (k, a), (km, am) in zip(run64, runm) if E.is_rows_key(k) and not np.array_equal(a, am) for it in [k[0]]}
        caught = False
        for it in sorted({r[0][0] for r in rows}):
            flagged = {(r[1], r[2]) for r in E.offending_rows(rows) if r[0][0] == it}
            print("%-56s %-32s it%d flags %s" % (mutant, name, it, sorted(flagged)))
            if not caught and it not in differs:
                assert not flagged
            elif not caught:
                assert flagged == want, "%s, %s: flagged %r, concerned %r" % (mutant, name, sorted(flagged), sorted(want))
                caught = True
            else:
                assert flagged >= want, "%s, %s it%d: flagged %r, concerned %r" % (mutant, name, it, sorted(flagged), sorted(want))
        assert caught, "%s: not caught on %s" % (mutant, name)


def test_exact_entropy_of_latent_rows_is_of_the_covariance_they_carry():
    """The exact bound's entropy of the outputs (tests/exact_bound_ref.py: _y_entropy_exact) in the envelope's order -- update_Y,
    then the parameters, R among them, then the bound -- against the covariances written out: a row nothing of which is observed
    carries inv <R> of the <R> its update met, a partially observed one inv(<R>_uu) of the same <R>; the <R> the bound meets is
    another one.  (The restatement used to take a latent row's ln det of the current <R> under Wishart noise, which is right
    only straight after update_Y; the row-wise GPU tests found the handle, which stores the value at the update, 2e-2 of the
    bound away from it.)"""
    import exact_bound_ref as XR
    from oracle import lds_closed_form as O
    c = E.lds_case("t11_d5_k9_wishart_rows")
    K = c["Y"].shape[2]
    m = E.OracleLDS(E.to_long(c["Y"]), E.to_long(c["st0"]), E.to_long(c["pri"]))
    for it in range(2):
        m.sweep("forward"); m.sweep("backward")
        Rb = O.noise_expect("wishart", m.st["R_a"], m.st["R_b"], K).copy()
        m.update_Y(); m.update_A(); m.update_C(); m.update_Q(); m.update_R()
        now = O.noise_expect("wishart", m.st["R_a"], m.st["R_b"], K)
        miss = np.isnan(c["Y"])
        want = np.zeros(miss.shape[0], dtype=LD)
        stale = np.zeros(miss.shape[0], dtype=LD)
        for n, t in zip(*np.nonzero(miss.any(axis=2))):
            u = np.nonzero(miss[n, t])[0]
            ld = -O.XL.slogdet(Rb[n][np.ix_(u, u)])[1]
            want[n] += 0.5 * u.size * XR.ln2pi(Rb) + 0.5 * ld + 0.5 * u.size
            stale[n] += 0.5 * (-O.XL.slogdet(now[n][np.ix_(u, u)])[1] - ld)
        got = XR._y_entropy_exact(m.st)
        print("it%d exact entropy of the outputs %r, written out %r; with the current <R> it would be off by %r" % (it, got, want, stale))
        assert got.dtype == LD and np.all(np.abs(got - want) <= 1e-16 * np.abs(want))
        assert np.abs(stale[0]) > 1e-3 * np.abs(want[0])
