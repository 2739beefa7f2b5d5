"""GPU: the HIP paths at their real accuracy.  Every kernel instantiation is driven stage by stage through the example's
loop and compared, after every stage, with the oracles run in extended precision (tests/extended_ref.py) -- not at the
suite's RTOL = 1e-8 but at 16 times what the float64 oracle itself loses on the same problem:

    e_gpu <= 16 max(e64, n 2^-52),   n = max(D, K, T)  (PCA: max(d, q, N)),

with e64 <= 1e-11 enforced on every case by tests/test_extended_ref_cpu.py.  The bound is set by the reference side only;
the factor covers Gauss-Jordan without pivoting against LAPACK, the MFMA accumulation order, v_rcp_f64 + Newton against
IEEE division and the carry-over across two iterations (which also has the measured table).  The lower
bound is not compared here (digamma / gammaln are float64 only; it keeps its 1e-8 tests).

The warm-up contract: the lengths get_warmup() reports are sufficient (||M^J|| <= 1e-18 for the recurrence matrices of the
extended run) and not wasteful (at most one step of the rule's granularity above what the documented rule gives in NumPy).

Every test prints what it measured before it asserts (-s shows it; profiles/accuracy_envelope.txt is such an output).
"""
import functools

import numpy as np
import pytest

import extended_ref as E

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _run_handle(name):
    """The case on a handle: ([(key, array)] as E.lds_trace gives it, [get_warmup() after each iteration's sweeps])."""
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
    trace, warm = [], []
    for key, arr in E.lds_trace(E.HandleLDS(b), c["iters"], bool(np.isnan(Y).any())):
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
def test_pca_envelope(N, d, q, sweep, monkeypatch):
    """Stage by stage as tests/test_pca_gpu.py: test_stagewise_vs_oracle; where the sweep kernel is chosen, also with reads at the
    end of each iteration only, which is what lets the fused sweep over the rows run (extended_ref.pca_trace)."""
    from pyvb_amd.pca import PCABatch
    if sweep is not None:
        monkeypatch.setenv("PYVB_PCA_SWEEP", sweep)
    n, ext, e64, _ = E.pca_reference(N, d, q)
    assert max(e64.values()) <= E.CAP
    init, pri = E.pca_problem(N, d, q)
    over = []
    for stage_reads in ([True] if sweep is None else [True, False]):
        b = PCABatch.from_problem(init, pri)
        rows = []
        for key, arr in E.pca_trace(b, N, stage_reads=stage_reads):
            assert np.all(np.isfinite(arr)), key
            e_gpu = E.rel(arr, ext[key])
            rows.append((None, key, e64[key], e_gpu, e_gpu / E.yardstick(e64[key], n)))
        b.close()
        tag = "pca_%d_%d_%d%s%s" % (N, d, q, "" if sweep is None else "_" + sweep, "" if stage_reads else "_fused")
        over += _report(tag, rows)
    assert not over, "PCA (%d, %d, %d): %d quantities beyond %g x yardstick, worst %r" % (N, d, q, len(over), E.FACTOR, max(over, key=lambda r: r[4]))
