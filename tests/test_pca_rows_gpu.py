"""GPU: the VB-PCA sweeps (pyvb_amd/csrc/k_pca.hip) row by row against the long-double run, at the edges of their tiles.

The envelope's norm is max-abs over the whole [N, d] array: an observed entry overwritten by its prediction, or the one missing
entry of an otherwise observed row being off by 1e-10 of itself, disappears in it.  Here every row of a case is a named pattern
(extended_ref.PCA_ROW_PATTERNS: one byte of a mask word, one word, one tile, one block, the seam at column 128, the last partly
padded tile, ... under a column no row observes and a column one row observes), the shapes are the smallest that reach each
template form and each edge of the kernels (extended_ref.PCA_ROW_CASES says which), and per row, wherever the trace reads it,

    observed entries of X:  bitwise the data given to set_data (a fully observed row: all of it)
    missing entries of X:   max |handle - extended| / max |extended| over the row's missing entries  <=  16 max(e64_row, n 2^-52)
    Z:                      max |z - z_ext| / max |z_ext| of the row                                  <=  the same
    X_rowvar:               |v - v_ext| / |v_ext| of a row with a missing entry                       <=  the same

n = max(d, q, N), e64_row the float64 oracle's distance in the same unit (at most 1e-11: tests/test_pca_rows_cpu.py, which also
shows that the comparison catches five mutants of update_X).  Every quantity of the trace is held to the envelope as
tests/test_envelope_gpu.py: test_pca_envelope holds it, and the five parts of the bound in both modes.

Each case runs under every sweep kind listed for it (PCABatch.set_sweep) and in two read schedules: a read after every stage
(pass 1 and pass 2 apart), and a read at the end of each iteration only -- which lets the fused sweeps run, lazily where the kind
is "columns" or "pairs", so that the read goes through k_pca_materialize.

Every test prints what it measured before it asserts (-s shows it; profiles/accuracy_envelope.txt ends with such an output).
"""
import functools

import numpy as np
import pytest

import extended_ref as E

pytestmark = pytest.mark.gpu

RUNS = [(name, sweep, reads) for name, c in E.PCA_ROW_CASES.items() for sweep in c["sweeps"] for reads in c["schedules"]]
EXACT_RUNS = [(name, sweep) for name, c in E.PCA_ROW_CASES.items() if c["bounds"] for sweep in c["sweeps"]]


@functools.lru_cache(maxsize=None)
def _ncu():
    """the device's CU count, which sizes the long cases (256 on MI355X)"""
    import torch
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


def _handle(c, sweep, mode="reference"):
    from pyvb_amd.pca import PCABatch
    b = PCABatch.from_problem(c["init"], c["pri"])
    b.set_sweep(sweep)
    assert b.sweep == sweep
    if mode != "reference":
        b.set_bound_mode(mode)
    return b


def _trace(c, sweep, reads, mode="reference"):
    b = _handle(c, sweep, mode)
    trace = list(E.pca_trace(b, c["N"], iters=c["iters"], stage_reads=reads, bounds=(mode,) if c["bounds"] else (), parts=E.pca_handle_parts(b), rowvar=True))
    assert b.sweep == sweep
    b.close()
    return trace


def _tag(name, sweep, reads, mode=None):
    return "pca_rows %s %s%s%s" % (name, sweep, "" if reads else " fused", "" if mode is None else " " + mode)


def _brief(tag, what, rows, at):
    """rows of compare_pca_with_rows_reference (at: the index of e64; e_gpu and the ratio follow it): prints those beyond the
    yardstick or the cap and one line for the rest (every quantity and part of every run would be 3 000 lines), returns
    (offenders of the yardstick -- a non-finite value among them, its ratio is NaN --, offenders of the cap)"""
    over, capped = [r for r in rows if not r[at + 2] <= E.FACTOR], [r for r in rows if not r[at] <= E.CAP]
    for r in over + [r for r in capped if r not in over]:
        print("%-44s %-10s %r  e64 %.2e  e_gpu %.2e  e_gpu/y %6.2f  <-- over" % (tag, what, r[:at], r[at], r[at + 1], r[at + 2]))
    if rows:
        print("%-44s %-10s %2d values  max e64 %.2e  max e_gpu %.2e  max e_gpu/y %.2f"
              % (tag, what.upper(), len(rows), max(r[at] for r in rows), max(r[at + 1] for r in rows), max(r[at + 2] for r in rows)))
    return over, capped


def _assert_rows(tag, c, rows, reads):
    keys = c["iters"] * (6 if reads else 3)
    assert len(rows) == keys * c["N"], (tag, len(rows))
    assert max(r[4] for r in rows) <= E.CAP         # (tests/test_pca_rows_cpu.py reports it row by row)
    over = E.offending_rows(rows)
    by_pattern = sorted({(r[0][2], r[3]) for r in over})
    assert not over, "%s: %d rows out of order, (quantity, pattern) %r; worst (key, 0, row, pattern, e64, e_row, ratio, pinned) %r" \
        % (tag, len(over), by_pattern, max(over, key=lambda r: (not r[7], r[6] if r[6] == r[6] else np.inf)))


@pytest.mark.parametrize("name,sweep,reads", RUNS)
def test_pca_row_by_row(name, sweep, reads):
    """Rows, whole quantities and the reference bound of one handle."""
    ncu = _ncu()
    c = E.pca_rows_case(name, ncu)
    tag = _tag(name, sweep, reads)
    trace = _trace(c, sweep, reads)
    whole, bnd = E.compare_pca_with_rows_reference(name, trace, ncu)
    rows = E.compare_pca_rows(name, trace, tag=tag, ncu=ncu)
    over, capped_w = _brief(tag, "quantities", whole, 2)
    over_b, capped = _brief(tag, "bound", bnd, 3)
    assert len(whole) == c["iters"] * ((15 if reads else 10)) and len(bnd) == (5 * c["iters"] if c["bounds"] else 0)
    assert not capped_w and not capped
    _assert_rows(tag, c, rows, reads)
    assert not over, "%s: %d quantities beyond %g x yardstick, worst %r" % (tag, len(over), E.FACTOR, max(over, key=lambda r: r[4]))
    assert not over_b, "%s: %d parts beyond %g x yardstick, worst %r" % (tag, len(over_b), E.FACTOR, max(over_b, key=lambda r: r[5]))


@pytest.mark.parametrize("name,sweep", EXACT_RUNS)
def test_pca_rows_exact_bound(name, sweep):
    """The exact bound needs a handle of its own (the mode is set before the first update): the five parts after each iteration,
    read at the end of the iteration only, and the rows of that handle once more."""
    ncu = _ncu()
    c = E.pca_rows_case(name, ncu)
    tag = _tag(name, sweep, False, "exact")
    trace = _trace(c, sweep, False, "exact")
    _, bnd = E.compare_pca_with_rows_reference(name, trace, ncu)
    rows = E.compare_pca_rows(name, trace, tag=tag, ncu=ncu)
    over_b, capped = _brief(tag, "bound", bnd, 3)
    assert len(bnd) == 5 * c["iters"] and not capped
    _assert_rows(tag, c, rows, False)
    assert not over_b, "%s: %d parts beyond %g x yardstick, worst %r" % (tag, len(over_b), E.FACTOR, max(over_b, key=lambda r: r[5]))


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))


STATE = ("X", "X_rowvar", "W_mean", "W_var", "Z", "Z_cov", "Mu_mean", "Mu_var", "beta_ab")


@pytest.mark.parametrize("sweep", ["columns", "pairs"])
def test_a_second_handle_ends_bitwise_where_the_first_does(sweep):
    """The lazy sweeps carry state between iterations on the device (the flags and the ring of k_pca_pairs, <W>_x and <Mu>_x of the
    sweep before): two fresh handles of the same kind, read at the end of each iteration, agree in every bit of every array and
    of the bound."""
    c = E.pca_rows_case("n70_d256_q16")
    ends = []
    for _ in range(2):
        b = _handle(c, sweep)
        for _ in E.pca_trace(b, c["N"], iters=c["iters"], stage_reads=False):
            pass
        ends.append((b.get_state(), b.elbo()))
        b.close()
    differ = [k for k in STATE if not _same_bits(ends[0][0][k], ends[1][0][k])]
    print("%-44s arrays that differ between two fresh handles: %r; bounds the same bits: %s" % (_tag("n70_d256_q16", sweep, False), differ, _same_bits(ends[0][1], ends[1][1])))
    assert not differ and _same_bits(ends[0][1], ends[1][1])


@pytest.mark.parametrize("sweep", ["columns", "pairs"])
def test_materialising_is_idempotent(sweep):
    """After a lazy sweep the imputed entries exist only once a reader asks for them (k_pca_materialize): two consecutive
    get_state() return bitwise the same X -- the second reads nothing the first wrote -- with every observed entry the data."""
    c = E.pca_rows_case("n70_d256_q16")
    b = _handle(c, sweep)
    b.update_W(); b.update_Z(); b.update_X(0, 1); b.update_Mu(); b.update_X(1, c["N"])
    first = b.get_state()
    second = b.get_state()
    b.update_Beta()
    third = b.get_state()
    b.close()
    differ = [k for k in STATE if not _same_bits(first[k], second[k])]
    print("%-44s arrays that differ between two consecutive reads: %r" % (_tag("n70_d256_q16", sweep, False), differ))
    assert not differ
    assert _same_bits(first["X"], third["X"]) and _same_bits(first["Z"], third["Z"])
    obs = c["init"]["obs"]
    assert _same_bits(first["X"][obs], c["init"]["X"][obs])
