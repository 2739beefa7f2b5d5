"""GPU: the HIP paths at their real accuracy.  Every kernel instantiation is driven stage by stage through the example's
loop and compared, after every stage, with the oracles run in extended precision (tests/extended_ref.py) -- not at the
suite's RTOL = 1e-8 but at 16 times what the float64 oracle itself loses on the same problem:

    e_gpu <= 16 max(e64, n 2^-52),   n = max(D, K, T)  (PCA: max(d, q, N)),

with e64 <= 1e-11 enforced on every case by tests/test_extended_ref_cpu.py.  The bound is set by the reference side only;
the factor covers Gauss-Jordan without pivoting against LAPACK, the MFMA accumulation order, v_rcp_f64 + Newton against
IEEE division and the carry-over across two iterations (which also has the measured table).

The lower bound is held to the same yardstick part by part, in units of s_r = sum_p |part_p| of its replicate in the extended
run (oracle/_xspecial.py has digamma and gammaln in long double): both bound modes, every instantiation, a chain of length 2,
a PCA handle whose digamma argument is below 10 -- and the device's own digamma and lgamma on the arguments the bounds give
them, against the long-double values.

The warm-up contract: the lengths get_warmup() reports are sufficient (||M^J|| <= 1e-18 for the recurrence matrices of the
extended run) and not wasteful (at most one step of the rule's granularity above what the documented rule gives in NumPy).

Every test prints what it measured before it asserts (-s shows it; profiles/accuracy_envelope.txt is such an output).
"""
import functools

import numpy as np
import pytest

import extended_ref as E

pytestmark = pytest.mark.gpu


def _run_handle(name, mode="reference"):
    return _run_handle_cached(name, mode)


@functools.lru_cache(maxsize=None)
def _run_handle_cached(name, mode):
    """The case on a handle: ([(key, array)] as E.lds_trace gives it, [get_warmup() after each iteration's sweeps]).  The
    trace carries the parts of the bound of `mode` after each iteration; the exact bound is asked for before the first update
    (DESIGN.md section 13)."""
    from pyvb_amd.lds import LDSBatch
    c = E.lds_case(name)
    Y, T = c["Y"], c["Y"].shape[1]
    lengths = c.get("lengths")
    b = LDSBatch.from_problem(Y, c["st0"], c["pri"], lengths=None if lengths is None else np.asarray(lengths, dtype=np.int32))
    if c.get("W"):
        b.set_time_split(c["W"])
        assert b.get_time_split() == c["W"]
    if c.get("split_chosen"):
        assert b.get_time_split() > 1, "the library did not split the time axis of %s" % name
    if mode != "reference":
        b.set_bound_mode(mode)
    trace, warm = [], []
    for key, arr in E.lds_trace(E.HandleLDS(b), c["iters"], bool(np.isnan(Y).any()), (mode,)):
        trace.append((key, arr))
        if key[1:] == ("backward sweep", "X"):
            warm.append(b.get_warmup())
    if c.get("headline"):       # as test_headline_instantiation_one_wavefront_per_replicate_warmup: the warm-up path is exercised
        for w in warm:
            assert np.all(w > 0) and np.all(w < (T - 2) // 16), "warm-up path not exercised: J = %r, Lseg = %d" % (w, (T - 2) // 16)
    b.close()
    return trace, warm


def _report(tag, rows):
    """rows: [(replicate or None, key, e64, e_gpu, ratio)] -> prints them, returns the offenders"""
    for rep, key, e64, e_gpu, ratio in rows:
        print("%-28s %-4s it%d %-15s %-9s e64 %.2e  e_gpu %.2e  e_gpu/y %6.2f%s"
              % (tag, "" if rep is None else "r%d" % rep, key[0], key[1], key[2], e64, e_gpu, ratio, "  <-- over" if ratio > E.FACTOR else ""))
    print("%-28s SUMMARY  max e64 %.2e  max e_gpu %.2e  max e_gpu/y %.2f"
          % (tag, max(r[2] for r in rows), max(r[3] for r in rows), max(r[4] for r in rows)))
    return [r for r in rows if not r[4] <= E.FACTOR]


@pytest.mark.parametrize("name", list(E.LDS_CASES))
def test_lds_envelope(name):
    trace, _ = _run_handle(name)
    rows = E.compare_with_reference(name, trace)
    assert all(max(r[4].values()) <= E.CAP for r in E.lds_reference(name))   # (tests/test_extended_ref_cpu.py reports it quantity by quantity)
    over = _report(name, rows)
    assert not over, "%s: %d quantities beyond %g x yardstick, worst %r" % (name, len(over), E.FACTOR, max(over, key=lambda r: r[4]))


@pytest.mark.parametrize("name", E.WARMUP_CASES)
def test_warmup_lengths_are_sufficient_and_not_wasteful(name):
    _, warm = _run_handle(name)
    runs = E.lds_reference(name)
    per_replicate = runs[0][0] is not None
    bad = []
    for it, w in enumerate(warm):
        assert np.all(w < (1 << 30)), "%s: no contraction found, J = %r" % (name, w)
        for n in range(w.shape[0]):         # the recurrence matrices of replicate n: of its own run, or row n of the batch's
            F, B = (m[0] for m in runs[n][5][it]) if per_replicate else (m[n] for m in runs[0][5][it])
            for M, which, J, what in ((F, "inf", int(w[n, 0]), "forward"), (B, "1", int(w[n, 1]), "backward")):
                Jstar = E.warmup_rule(M, which)
                nrm = E.power_norm(M, J, which)
                ok = nrm <= 1e-18 * (1 + 1e-9) and J <= Jstar + 4
                print("%-28s it%d replicate %d %-8s J %4d  J* %4d  ||M^J|| %.3e%s" % (name, it, n, what, J, Jstar, nrm, "" if ok else "  <-- violated"))
                if not ok:
                    bad.append((it, n, what, J, Jstar, nrm))
    assert not bad, "%s: (iteration, replicate, sweep, J, J*, ||M^J||) %r" % (name, bad)


@pytest.mark.parametrize("N,d,q,sweep", [(300, 20, 4, None), (77, 33, 17, None), (17, 250, 31, None),
                                         (600, 250, 16, "columns"), (600, 250, 16, "pairs")])
def test_pca_envelope(N, d, q, sweep):
    """Stage by stage as tests/test_pca_gpu.py: test_stagewise_vs_oracle; where the sweep kernel is chosen, also with reads at the
    end of each iteration only, which is what lets the fused sweep over the rows run (extended_ref.pca_trace)."""
    from pyvb_amd.pca import PCABatch
    n, ext, e64, _ = E.pca_reference(N, d, q)
    assert max(e64.values()) <= E.CAP
    init, pri = E.pca_problem(N, d, q)
    over = []
    for stage_reads in ([True] if sweep is None else [True, False]):
        b = PCABatch.from_problem(init, pri)
        if sweep is not None:
            b.set_sweep(sweep)
        rows = []
        for key, arr in E.pca_trace(b, N, stage_reads=stage_reads):
            assert np.all(np.isfinite(arr)), key
            e_gpu = E.rel(arr, ext[key])
            rows.append((None, key, e64[key], e_gpu, e_gpu / E.yardstick(e64[key], n)))
        b.close()
        tag = "pca_%d_%d_%d%s%s" % (N, d, q, "" if sweep is None else "_" + sweep, "" if stage_reads else "_fused")
        over += _report(tag, rows)
    assert not over, "PCA (%d, %d, %d): %d quantities beyond %g x yardstick, worst %r" % (N, d, q, len(over), E.FACTOR, max(over, key=lambda r: r[4]))


def _report_bound(tag, names, rows):
    """rows: [(key, replicate, part index, e64, e_gpu, ratio, error relative to the part itself)] -> prints them, returns
    (offenders of the yardstick -- a non-finite part among them, its ratio is NaN --, offenders of the cap)"""
    for key, rep, p, e64, e_gpu, ratio, own in rows:
        print("%-28s r%-3d it%d %-9s %-6s e64 %.2e  e_gpu %.2e  e_gpu/y %6.2f  (of the part itself %.2e)%s"
              % (tag, rep, key[0], key[2], names[p], e64, e_gpu, ratio, own, "  <-- over" if ratio > E.FACTOR else ""))
    print("%-28s SUMMARY  max e64 %.2e  max e_gpu %.2e  max e_gpu/y %.2f"
          % (tag, max(r[3] for r in rows), max(r[4] for r in rows), max(r[5] for r in rows)))
    return [r for r in rows if not r[5] <= E.FACTOR], [r for r in rows if not r[3] <= E.CAP]


@pytest.mark.parametrize("name,mode", [(n, "reference") for n in E.LDS_CASES] + [(n, "exact") for n in E.EXACT_BOUND_CASES])
def test_lds_bound_envelope(name, mode):
    """The six parts of the lower bound after each iteration, per replicate: |part - extended| / s_r <= 16 max(e64, n 2^-52).
    Reference mode is read on the handle test_lds_envelope runs; the exact mode has a handle of its own."""
    trace, _ = _run_handle(name, mode)
    rows = E.compare_bound_with_reference(name, trace)
    over, capped = _report_bound("%s %s" % (name, mode), E.LDS_PARTS, rows)
    assert len(rows) == 6 * E.lds_case(name)["iters"] * E.lds_case(name)["Y"].shape[0]
    assert not capped, "%s: the float64 oracle is beyond the cap on %r" % (name, capped)
    assert not over, "%s %s: %d parts beyond %g x yardstick, worst %r" % (name, mode, len(over), E.FACTOR, max(over, key=lambda r: r[5]))


@pytest.mark.parametrize("mode", E.BOUND_MODES)
@pytest.mark.parametrize("N,d,q,sweep", [(300, 20, 4, None), (77, 33, 17, None), (17, 250, 31, None),
                                         (600, 250, 16, "columns"), (600, 250, 16, "pairs"), E.PCA_SMALL + (None,)])
def test_pca_bound_envelope(N, d, q, sweep, mode):
    """The five parts of the VB-PCA bound after each iteration.  Where the sweep kernel is chosen the handle is read at the end of
    an iteration only, so that the chosen sweep runs (test_pca_envelope); the 1 x 1 x 1 handle has beta_a = 0.501, which takes
    the host's digamma through its recurrence."""
    from pyvb_amd.pca import PCABatch
    n = E.pca_reference(N, d, q)[0]
    ref = E.pca_bound_reference(N, d, q)
    init, pri = E.pca_problem(N, d, q)
    b = PCABatch.from_problem(init, pri)
    if sweep is not None:
        b.set_sweep(sweep)
    if mode != "reference":
        b.set_bound_mode(mode)
    rows = []
    for key, arr in E.pca_trace(b, N, stage_reads=sweep is None, bounds=(mode,), parts=E.pca_handle_parts(b)):
        if E.is_bound(key):
            ext, e64, _ = ref[key]
            rows += [(key,) + row for row in E.compare_bound(arr, ext, e64, n)]
    b.close()
    tag = "pca_%d_%d_%d%s %s" % (N, d, q, "" if sweep is None else "_" + sweep + "_fused", mode)
    over, capped = _report_bound(tag, E.PCA_PARTS, rows)
    assert len(rows) == 5 * 2
    assert not capped, "%s: the float64 oracle is beyond the cap on %r" % (tag, capped)
    assert not over, "%s: %d parts beyond %g x yardstick, worst %r" % (tag, len(over), E.FACTOR, max(over, key=lambda r: r[5]))


def test_device_special_functions():
    """The device's digamma (pyvb_amd/csrc/digamma.h: the one k_elbo, k_wishart's psi_multi and the tape interpreter call) and
    lgamma on the arguments the bounds give them (extended_ref.special_grid), one T_UNARY record each, against the long-double
    values in units of max(1, |f|): within 16 max(scipy's largest distance on the same grid, 2^-52)."""
    import scipy.special as sp
    from oracle import _xspecial as XS
    from pyvb_amd import generic as G
    E.require_extended()
    x = E.special_grid()
    n = x.size
    ex = G.DeviceExecutor(3 * 256)
    ex.write(0, x)
    ex.run(ex.tape([[G.T_UNARY, 256, 0, 0, n, 1, 0, G.U_DIGAMMA], [G.T_UNARY, 512, 0, 0, n, 1, 0, G.U_LGAMMA]]))
    got = {"digamma": ex.read(256, n), "lgamma": ex.read(512, n)}
    ex.close()
    bad = []
    for name, ref, f64 in (("digamma", XS.digamma(x.astype(E.LD)), sp.digamma(x)), ("lgamma", XS.gammaln(x.astype(E.LD)), sp.gammaln(x))):
        ok = np.isfinite(ref)           # (every point of the grid today)
        unit = np.maximum(1.0, np.abs(ref[ok]))
        e64 = (np.abs(f64[ok].astype(E.LD) - ref[ok]) / unit).astype(float)
        assert np.all(np.isfinite(got[name][ok])), "%s: not finite at %r" % (name, x[ok][~np.isfinite(got[name][ok])])
        e_gpu = (np.abs(got[name][ok].astype(E.LD) - ref[ok]) / unit).astype(float)
        y = max(float(e64.max()), E.U64)
        worst = int(e_gpu.argmax())
        print("device %-8s %d points  scipy: largest e64 %.2e at %r   device: largest e_gpu %.2e at %r   e_gpu/y %.2f"
              % (name, ok.sum(), e64.max(), float(x[ok][int(e64.argmax())]), e_gpu[worst], float(x[ok][worst]), e_gpu[worst] / y))
        for xi, e in zip(x[ok], e_gpu):
            if not e <= E.FACTOR * y:
                print("device %-8s x = %r  e_gpu %.2e  e_gpu/y %.2f  <-- over" % (name, float(xi), e, e / y))
                bad.append((name, float(xi), float(e / y)))
    assert not bad, "(function, x, e_gpu / y) beyond %g: %r" % (E.FACTOR, bad)
