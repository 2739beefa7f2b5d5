"""GPU: outputs that hold NaN, row by row against the long-double run (pyvb_amd/csrc/k_missing.hip; gj_wave_subset in gj.h).

The envelope's norm is max-abs over a whole array: a known entry that is no longer pinned, or the one missing entry of an
otherwise observed row being off by 1e-10 of itself, disappears under a fully missing row.  Here the cases of
extended_ref._missing_rows -- every row a named pattern: one known entry, one missing entry in lane 0 or lane K - 1, one 8-wide
tile, every second entry, the halves and the seam of the 128-wide class, both ends of the chain unobserved -- are read after
every update_Y, and per row

    known entries:    Yq bitwise the observation, Yvar exactly 0.0 (a fully observed row: all of it)
    missing entries:  max |handle - extended| / max |extended| over the row's missing entries  <=  16 max(e64_row, n 2^-52)

for Yq and Yvar separately, n = max(D, K, T), e64_row the float64 oracle's distance in the same unit (at most 1e-11:
tests/test_missing_rows_cpu.py, which also shows that the comparison catches five mutants of update_Y).

Then the default order -- iterate() does not update the outputs, under Wishart noise the rows keep their diagonal initial
covariances (k_missing_ent_dense with diag_cov = 1) -- followed by an iteration that does; and the initial outputs a handle
gives itself when it is told none (k_missing_init with null pointers).

Every test prints what it measured before it asserts (-s shows it; profiles/accuracy_envelope.txt is such an output).
"""
import numpy as np
import pytest

import extended_ref as E
from test_envelope_gpu import _report, _report_bound

pytestmark = pytest.mark.gpu

ROW_CASES = E.ROWS_ENVELOPE + ["t7_d65_k128_rows_big", "t11_d9_k128_rows_big"]
ORDER = (False, True)           # outputs never updated in the first iteration, updated in the second
ORDER_CASES = ["t11_d5_k9_wishart_rows", "t11_d6_k64_wishart_rows", "t11_d12_k100_rows_big"]
DEFAULT_CASES = ["t11_d5_k9_wishart_rows", "t11_d12_k100_rows_big"]


def _handle(c, mode="reference"):
    from pyvb_amd.lds import LDSBatch
    b = LDSBatch.from_problem(c["Y"], c["st0"], c["pri"])
    if mode != "reference":
        b.set_bound_mode(mode)          # before the first update
    return b


def _trace(name, updates=None, mode="reference"):
    """[(key, array)] of extended_ref.lds_trace_order on a handle of the case"""
    c = E.lds_case(name)
    b = _handle(c, mode)
    trace = list(E.lds_trace_order(E.HandleLDS(b), updates or (True,) * c["iters"], () if c.get("outputs_only") else (mode,)))
    b.close()
    return trace


def _assert_rows(name, rows, updates=None):
    c = E.lds_case(name)
    N, T, _ = c["Y"].shape
    its = E.row_iterations(updates or (True,) * c["iters"])
    assert its and len(rows) == 2 * len(its) * N * T, (name, its, len(rows))
    assert max(r[4] for r in rows) <= E.CAP         # (tests/test_missing_rows_cpu.py reports it row by row)
    over = E.offending_rows(rows)
    by_pattern = sorted({(r[0][2], r[3]) for r in over})
    assert not over, "%s: %d rows out of order, (quantity, pattern) %r; worst (key, replicate, row, pattern, e64, e_row, ratio, pinned) %r" \
        % (name, len(over), by_pattern, max(over, key=lambda r: (not r[7], r[6] if r[6] == r[6] else np.inf)))


@pytest.mark.parametrize("name", ROW_CASES)
def test_outputs_row_by_row(name):
    rows = E.compare_rows(name, _trace(name))
    _assert_rows(name, rows)


@pytest.mark.parametrize("mode", E.BOUND_MODES)
@pytest.mark.parametrize("name", ORDER_CASES)
def test_outputs_never_updated_then_updated(name, mode):
    """The first iteration without update_Y (sweeps, A, C, Q, R, bound: what iterate() does), the second with it.  Every
    quantity of the trace after both iterations, the outputs among them; the rows after the update_Y; the six parts of the bound
    after the second iteration only -- before the first update_Y the reference's bound is NaN in both oracles
    (tests/test_missing_rows_cpu.py), and the handle's value there is not compared."""
    tag = "%s kept, updated %s" % (name, mode)
    trace = _trace(name, ORDER, mode)
    assert [k for k, _ in trace if E.is_bound(k)] == [(0, "bound", mode), (1, "bound", mode)]
    whole, bnd = E.compare_with_rows_reference(name, trace, ORDER, skip_bound=(0,))
    rows = E.compare_rows(name, trace, ORDER, tag=tag)
    over = _report(tag, whole)
    over_b, capped = _report_bound(tag, E.LDS_PARTS, bnd)
    assert len(whole) == len(trace) - 2 and len(bnd) == 6 * E.lds_case(name)["Y"].shape[0]
    assert max(r[2] for r in whole) <= E.CAP and not capped
    assert not over, "%s: %d quantities beyond %g x yardstick, worst %r" % (tag, len(over), E.FACTOR, max(over, key=lambda r: r[4]))
    _assert_rows(name, rows, ORDER)
    assert not over_b, "%s: %d parts beyond %g x yardstick, worst %r" % (tag, len(over_b), E.FACTOR, max(over_b, key=lambda r: r[5]))


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))


@pytest.mark.parametrize("name", DEFAULT_CASES)
def test_default_initial_outputs(name):
    """A handle that is told no initial outputs (k_missing_init with null pointers) and one that is told Yq = 0 on the rows that
    hold NaN and Yrowvar = 1: bitwise equal before the first update and in every array after one full iteration; the second
    is held to the extended run, whole arrays, rows and bound."""
    explicit = name + "_explicit"
    cd, ce = E.lds_case(name + "_default"), E.lds_case(explicit)
    bd, be = _handle(cd), _handle(ce)
    for a, b in zip(bd.get_outputs(with_qld=True), be.get_outputs(with_qld=True)):
        assert _same_bits(a, b)
    td = list(E.lds_trace_order(E.HandleLDS(bd), (True,), ("reference",)))
    te = list(E.lds_trace_order(E.HandleLDS(be), (True,), ("reference",)))
    assert [k for k, _ in td] == [k for k, _ in te]
    differ = [k for (k, a), (_, b) in zip(td, te) if not _same_bits(a, b)]
    for a, b in zip(bd.get_outputs(with_qld=True) + tuple(bd.get_logdets().values()), be.get_outputs(with_qld=True) + tuple(be.get_logdets().values())):
        assert _same_bits(a, b)
    bd.close(); be.close()
    assert not differ, "%s: default and explicit initial outputs differ in %r" % (name, differ)
    whole, bnd = E.compare_with_rows_reference(explicit, te)
    rows = E.compare_rows(explicit, te)
    over = _report(explicit, whole)
    over_b, capped = _report_bound(explicit, E.LDS_PARTS, bnd)
    assert len(whole) == len(te) - 1 and len(bnd) == 6 * ce["Y"].shape[0]
    assert max(r[2] for r in whole) <= E.CAP and not capped
    assert not over, "%s: %d quantities beyond %g x yardstick, worst %r" % (explicit, len(over), E.FACTOR, max(over, key=lambda r: r[4]))
    _assert_rows(explicit, rows)
    assert not over_b, "%s: %d parts beyond %g x yardstick, worst %r" % (explicit, len(over_b), E.FACTOR, max(over_b, key=lambda r: r[5]))
