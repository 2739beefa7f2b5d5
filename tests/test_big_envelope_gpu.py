"""GPU: the 128-wide LDS class, 64 < max(D, K) <= 128 (pyvb_amd/csrc/k_big.hip, k_wishart_big.hip and the two-wavefront forms of
the small kernels), at its real accuracy and at every tile count -- extended_ref.BIG_CASES, driven stage by stage through the
example's loop as tests/test_envelope_gpu.py drives its cases, and held to the long-double run

  * quantity by quantity after every stage, e_gpu <= 16 max(e64, n 2^-52) (extended_ref.compare_with_reference);
  * tile by tile: the last two axes of Sigma, A_mean, C_mean, A_colvar, C_colvar (Q_w, R_w, A_cov, C_cov under Wishart noise) cut
    into 16 x 16 tiles, the states into the 16-entry tile of each node, each tile in units of its own largest entry of the
    extended run, e_tile <= 16 max(e64_tile, n 2^-52) -- the unit the kernels deal their work out in: a tile that belongs to one
    wavefront, or one mirrored store of k_stats_big, cannot hide beside the diagonal (extended_ref.compare_tiles);
  * part by part of the lower bound, reference mode on every case, exact mode on a handle of its own for the two full-width
    cases (the others reach no further instantiation of k_elbo<2>);
  * the warm-up contract on the plain cases, and on the 600-node case the from-zero path itself: 0 < J < Lseg;
  * the known entries of A and C bitwise, their variances exactly 0.0, after every update_A / update_C.

tests/test_big_envelope_cpu.py holds the reference side: e64 <= 1e-11 whole, by tile and by part, so no bound exceeds 1.6e-10.
Every test prints what it measured before it asserts (-s shows it; profiles/accuracy_envelope.txt has such an output).
"""
import functools

import numpy as np
import pytest

import extended_ref as E
from test_envelope_gpu import _report, _report_bound

pytestmark = pytest.mark.gpu


def _runs():
    """[(case, forced time split or None)]: the warm-up case at W = 1 and at W = 2, each against the one extended run"""
    return [(name, W) for name in E.BIG_CASES for W in E.BIG_SPLITS.get(name, (None,))]


def _tag(name, W):
    return name if W is None else "%s_w%d" % (name, W)


@functools.lru_cache(maxsize=None)
def _run_handle(name, W=None, mode="reference"):
    """The case on a handle: (trace [(key, array)] as E.lds_trace gives it with the parts of the bound of `mode`, [get_warmup() after
    each iteration's sweeps], offenders among the known entries, known entries looked at)."""
    from pyvb_amd.lds import LDSBatch
    c = E.lds_case(name)
    assert (W is None) == ("splits" not in c) and (W is None or W in c["splits"])
    b = LDSBatch.from_problem(c["Y"], c["st0"], c["pri"])
    if W is not None:
        b.set_time_split(W)
        assert b.get_time_split() == W
    if mode != "reference":
        b.set_bound_mode(mode)
    m = E.PinnedHandleLDS(b, c["pri"])
    trace, warm = [], []
    for key, arr in E.lds_trace(m, c["iters"], False, (mode,)):
        trace.append((key, arr))
        if key[1:] == ("backward sweep", "X"):
            warm.append(b.get_warmup())
    b.close()
    return trace, warm, m.pins, m.pin_checks


@pytest.mark.parametrize("name,W", _runs(), ids=[_tag(*r) for r in _runs()])
def test_big_envelope(name, W):
    """Every whole quantity after every stage, as tests/test_envelope_gpu.py: test_lds_envelope."""
    trace, _, _, _ = _run_handle(name, W)
    rows = E.compare_with_reference(name, trace)
    assert all(max(r[4].values()) <= E.CAP for r in E.lds_reference(name))
    over = _report(_tag(name, W), rows)
    assert not over, "%s: %d quantities beyond %g x yardstick, worst %r" % (_tag(name, W), len(over), E.FACTOR, max(over, key=lambda r: r[4]))


@pytest.mark.parametrize("name,W", _runs(), ids=[_tag(*r) for r in _runs()])
def test_big_envelope_by_tile(name, W):
    """Every 16 x 16 tile of the matrix quantities and every 16-entry node tile of the states after every stage, in the tile's own
    unit: e_tile <= 16 max(e64_tile, n 2^-52); a tile that is exactly zero in the extended run is exactly zero here."""
    trace, _, _, _ = _run_handle(name, W)
    assert all(float(e.max()) <= E.CAP for til in E.lds_tile_reference(name) for e in til.values())
    rows = E.compare_tiles(name, trace, tag=_tag(name, W))
    want = {k for k, _ in trace if not E.is_bound(k) and k[2] in E.TILE_QUANTITIES}
    assert {r[1] for r in rows} == want and any(k[2] == "X" for k in want) and any(k[2] == "Sigma" for k in want)
    print("%-28s SUMMARY tiles %d  max e64 %.2e  max e_tile %.2e  max e_tile/y %.2f"
          % (_tag(name, W), sum(r[3].size for r in rows), max(r[2].max() for r in rows), max(r[3].max() for r in rows), max(r[4].max() for r in rows)))
    over = E.offending_tiles(rows)
    for o in over[:40]:
        print("%-28s it%d %-15s %-9s tile %r  e64 %.2e  e_tile %.2e  e_tile/y %.2f  <-- over" % ((_tag(name, W), o[1][0], o[1][1], o[1][2]) + o[2:]))
    assert not over, "%s: %d tiles beyond %g x yardstick, worst %r" % (_tag(name, W), len(over), E.FACTOR, max(over, key=lambda o: o[5]))


@pytest.mark.parametrize("name,W,mode", [(n, W, "reference") for n, W in _runs()] + [(n, None, "exact") for n in E.BIG_EXACT_BOUND_CASES],
                         ids=[_tag(*r) + "-reference" for r in _runs()] + [n + "-exact" for n in E.BIG_EXACT_BOUND_CASES])
def test_big_bound_envelope(name, W, mode):
    """The six parts of the lower bound after each iteration: |part - extended| / s_r <= 16 max(e64, n 2^-52).  Reference mode is
    read on the handle test_big_envelope runs; the exact mode has a handle of its own."""
    trace, _, _, _ = _run_handle(name, W, mode)
    rows = E.compare_bound_with_reference(name, trace)
    over, capped = _report_bound("%s %s" % (_tag(name, W), mode), E.LDS_PARTS, rows)
    assert len(rows) == 6 * E.lds_case(name)["iters"] * E.lds_case(name)["Y"].shape[0]
    assert not capped, "%s: the float64 oracle is beyond the cap on %r" % (name, capped)
    assert not over, "%s %s: %d parts beyond %g x yardstick, worst %r" % (_tag(name, W), mode, len(over), E.FACTOR, max(over, key=lambda r: r[5]))


@pytest.mark.parametrize("name,W", [r for r in _runs() if r[0] in E.BIG_WARMUP_CASES], ids=[_tag(*r) for r in _runs() if r[0] in E.BIG_WARMUP_CASES])
def test_big_warmup_lengths_are_sufficient_and_not_wasteful(name, W):
    """tests/test_envelope_gpu.py: test_warmup_lengths_are_sufficient_and_not_wasteful on the plain cases of the class: the lengths
    get_warmup() reports leave ||M^J|| <= 1e-18 (1 + 1e-9) for the recurrence matrices of the extended run, and J <= J* + 4."""
    _, warm, _, _ = _run_handle(name, W)
    (_, T, _, _, _, rec, _), = E.lds_reference(name)
    assert len(warm) == len(rec) == E.lds_case(name)["iters"]
    bad = []
    for it, w in enumerate(warm):
        assert np.all(w < (1 << 30)), "%s: no contraction found, J = %r" % (name, w)
        for n in range(w.shape[0]):
            F, B = (m[n] for m in rec[it])
            for M, which, J, what in ((F, "inf", int(w[n, 0]), "forward"), (B, "1", int(w[n, 1]), "backward")):
                Jstar = E.warmup_rule(M, which)
                nrm = E.power_norm(M, J, which)
                ok = nrm <= 1e-18 * (1 + 1e-9) and J <= Jstar + 4
                print("%-28s it%d replicate %d %-8s J %4d  J* %4d  ||M^J|| %.3e%s" % (_tag(name, W), it, n, what, J, Jstar, nrm, "" if ok else "  <-- violated"))
                if not ok:
                    bad.append((it, n, what, J, Jstar, nrm))
    assert not bad, "%s: (iteration, replicate, sweep, J, J*, ||M^J||) %r" % (_tag(name, W), bad)


@pytest.mark.parametrize("W", [1, 2])
def test_columns_warm_up_from_zero_at_full_width(W):
    """What t600_d128_k128_warm is there for: 0 < J < Lseg for every replicate in both directions, so k_sweep_big has segment columns
    that start from zero -- at W = 2 across the border of the two parts of 304 and 294 nodes, where Lseg = 19."""
    name = "t600_d128_k128_warm"
    _, warm, _, _ = _run_handle(name, W)
    T = E.lds_case(name)["Y"].shape[1]
    Lw = T - 2 if W == 1 else (((T - 2 + W - 1) // W) + 15) & ~15      # pyvb_amd/csrc/geometry.h: part_len
    Lseg = (Lw + 15) >> 4
    assert (Lw, Lseg) == ((598, 38) if W == 1 else (304, 19))
    for w in warm:
        print("%-28s J forward %r  backward %r  Lseg %d" % (_tag(name, W), w[:, 0].tolist(), w[:, 1].tolist(), Lseg))
        assert np.all(w > 0) and np.all(w < Lseg) and np.all(w < 19), "warm-up from zero not exercised: J = %r, Lseg = %d" % (w, Lseg)


def test_known_entries_are_bitwise():
    """Every known entry of A_mean / C_mean is bitwise the given value and its variance exactly 0.0, after every update_A /
    update_C of t27_d97_k113_known (extended_ref.PinnedHandleLDS looks after each call)."""
    name = "t27_d97_k113_known"
    c = E.lds_case(name)
    _, _, pins, looked = _run_handle(name)
    known = sum(int((~np.isnan(c["pri"][w + "_obs"])).sum()) for w in ("A", "C"))
    print("%-28s known entries %d, looked at %d times in all, not held: %d %r" % (name, known, looked, len(pins), pins[:10]))
    assert looked == known * c["iters"] and known >= 2 * 97 + 30
    assert not pins, "(matrix, replicate, row, column, what) %r" % pins[:40]
    for other in ("t35_d128_k128",):        # a case without known entries looks at none
        assert _run_handle(other)[3] == 0
