"""GPU: the forward sweep's seam starts (pyvb_amd/csrc/sweep_plan.h, k_sweep.hip MODE 1 without time split).  A column whose
left neighbour and itself own at least J nodes starts from zero at its own first node and is made good afterwards by J steps
of delta <- F delta added to the stored c_t (and X) rows; every other column warms up, or starts at the boundary, as before.

The shapes are small but long enough for seam starts: J is read from the handle after k_prep (it does not depend on T; the
replicates of a problem share their initial parameters, so they share J in the first sweep), the lengths are built around it,
and the plan -- tests/c/sweep_plan_driver.cpp, built here with the host compiler, the one definition the kernel reads too -- is
asked which columns start how.  A shape meant to have seam starts fails if it has none.

Checks, with the comparators the suite already has and no tolerance of their own:
* X after one forward sweep and after a forward + backward pair against the oracle in extended precision, by the envelope's
  rule (tests/extended_ref.py: rel, yardstick, FACTOR, CAP): e_gpu <= 16 max(e64, n 2^-52), e64 <= 1e-11 -- over all nodes, and
  again over the seam nodes alone (the first J of every seam column and the node before each), both reported on failure;
* the six parts of the bound after iterate(3) against oracle/lds_closed_form.py at tests/test_gpu_parity.py's 1e-8 of sum |part|;
* stage-wise forward and backward sweeps plus the parameter updates equal iterate(1) bit for bit, as
  tests/test_gpu_parity.py::test_iterate_equals_individual_calls_and_is_deterministic compares that pair.
"""
import functools
import os
import subprocess

import numpy as np
import pytest

import extended_ref as E
from oracle import lds_closed_form as O
from pyvb_amd import synth

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
RTOL = 1e-8                 # tests/test_gpu_parity.py
BOUNDARY, SEAM, WARM = 0, 1, 2
N = 3
J_MAX = 64                  # the problems are drawn once at the length a warm-up of 64 steps would need, and cut
T_GEN = 16 * (J_MAX + 8) + 2
SHAPES = [(16, 16), (17, 33), (64, 64)]
SMALL = [(16, 16), (17, 33)]


@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    """kinds(TL, T, J, forward=1) -> the 16 columns' (before, count, jc, kind) from sweep_plan.h (W = 1)."""
    tmp = tmp_path_factory.mktemp("sweep_plan_gpu")
    exe = tmp / "sweep_plan_driver"
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(REPO, "pyvb_amd", "csrc"),
                    os.path.join(HERE, "c", "sweep_plan_driver.cpp"), "-o", str(exe)], check=True, capture_output=True)

    def kinds(TL, T, J, forward=1):
        (tmp / "in.txt").write_text("plan %d %d 1 0 %d %d\n" % (TL, T, J, forward))
        subprocess.run([str(exe), str(tmp / "in.txt"), str(tmp / "out.txt")], check=True)
        fields = (tmp / "out.txt").read_text().strip().split("|")
        return [tuple(int(x) for x in f.split()) for f in fields[1:]]
    return kinds


@functools.lru_cache(maxsize=None)
def _base(D, K):
    """One draw per shape at T_GEN; the replicates keep their own data and initial states and share replicate 0's parameters."""
    Y, st0, pri = synth.make_problem(T_GEN, D, K, N, seed=900 + D + K)
    for k in ("A_mean", "C_mean", "A_colvar", "C_colvar", "Q_b", "R_b"):
        st0[k] = np.repeat(st0[k][:1], N, axis=0)
    return Y, st0, pri


def _cut(D, K, T, lengths=None):
    Y, st0, pri = _base(D, K)
    Y = Y[:, :T].copy()
    st0 = {k: (v[:, :T] if k == "X" else v).copy() for k, v in st0.items()}
    if lengths is not None:
        live = np.arange(T)[None, :] < np.asarray(lengths)[:, None]
        Y = np.where(live[:, :, None], Y, 0.0)
        st0["X"] = np.where(live[:, :, None], st0["X"], 0.0)
    return Y, st0, pri


def _batch(Y, st0, pri, lengths=None):
    from pyvb_amd.lds import LDSBatch
    b = LDSBatch.from_problem(Y, st0, pri, lengths=lengths)
    b.set_time_split(1)
    assert b.get_time_split() == 1
    return b


@functools.lru_cache(maxsize=None)
def _J(D, K):
    """The forward warm-up length of the first sweep of this shape's problem, from the handle after k_prep."""
    b = _batch(*_cut(D, K, 100))
    b.sweep("forward")
    w = b.get_warmup()
    b.close()
    J = int(w[0, 0])
    assert np.all(w[:, 0] == J) and 4 <= J <= J_MAX, "forward warm-up lengths %r: the problems are drawn for one J <= %d" % (w[:, 0], J_MAX)
    return J


def _seam_nodes(cols, J):
    """Time indices of the first J nodes of every seam column and of the node before each (interior node i is t = i + 1)."""
    t = set()
    for before, count, jc, kind in cols:
        if kind == SEAM:
            t |= set(range(before, before + J + 1))
    return sorted(t)


@functools.lru_cache(maxsize=None)
def _reference(D, K, T, lengths):
    """[(replicate or None, T_n, X after the forward sweep, X after the pair)] in float64 and in extended precision, each
    replicate of a handle with lengths run alone (tests/extended_ref.py: _problems).  Computed once, never modified."""
    Y, st0, pri = _cut(D, K, T, lengths)
    if lengths is None:
        problems = [(None, T, Y, st0)]
    else:
        problems = [(n, Tn, Y[n:n + 1, :Tn].copy(), {k: (v[n:n + 1, :Tn] if k == "X" else v[n:n + 1]).copy() for k, v in st0.items()})
                    for n, Tn in enumerate(lengths)]
    out = []
    for rows, Tn, Yp, sp in problems:
        res = {}
        for tag, m in (("f64", E.OracleLDS(Yp.copy(), {k: v.copy() for k, v in sp.items()}, pri)),
                       ("ext", E.OracleLDS(E.to_long(Yp), E.to_long(sp), E.to_long(pri)))):
            m.sweep("forward")
            res[tag, "forward"] = np.array(m.read("X"))
            m.sweep("backward")
            res[tag, "pair"] = np.array(m.read("X"))
            for a in res.values():
                a.setflags(write=False)
        out.append((rows, Tn, res))
    return out


def _check_sweeps(plan, D, K, T, lengths, want_seams):
    """want_seams: per replicate True (at least one seam column), False (none), or None (not asserted)."""
    J = _J(D, K)
    Y, st0, pri = _cut(D, K, T, lengths)
    b = _batch(Y, st0, pri, lengths)
    b.sweep("forward")
    got = {"forward": b.get_state(("X",))["X"]}
    assert np.all(b.get_warmup()[:, 0] == J)
    b.sweep("backward")
    got["pair"] = b.get_state(("X",))["X"]
    b.close()
    lens = lengths if lengths is not None else (T,) * N
    plans = [plan(Tn, T, J) for Tn in lens]
    for n, (cols, want) in enumerate(zip(plans, want_seams)):
        nseam = sum(1 for s in cols if s[3] == SEAM)
        if want is True:
            assert nseam >= 1, "replicate %d (T_n = %d, J = %d): no column starts at a seam, the case proves nothing" % (n, lens[n], J)
        elif want is False:
            assert nseam == 0, "replicate %d (T_n = %d, J = %d): %d seam columns where every column must warm up" % (n, lens[n], J, nseam)
    report, bad = [], []
    for rows, Tn, ref in _reference(D, K, T, lengths):
        reps = range(N) if rows is None else [rows]
        nn = max(D, K, Tn)
        for stage in ("forward", "pair"):
            g = got[stage] if rows is None else got[stage][rows:rows + 1, :Tn]
            assert np.all(np.isfinite(g)), "non-finite states after the %s" % stage
            ext, f64 = ref["ext", stage], ref["f64", stage]
            e64, e_gpu = E.rel(f64, ext), E.rel(g, ext)
            bound = E.FACTOR * E.yardstick(e64, nn)
            line = "rows %s T_n %d %-7s all nodes : e64 %.2e e_gpu %.2e bound %.2e" % (rows, Tn, stage, e64, e_gpu, bound)
            report.append(line)
            if not (e64 <= E.CAP and e_gpu <= bound):
                bad.append(line)
            for i, n in enumerate(reps):
                ts = _seam_nodes(plans[n], J)
                if not ts:
                    continue
                e64s, e_gpus = E.rel(f64[i, ts], ext[i, ts]), E.rel(g[i, ts], ext[i, ts])
                bounds = E.FACTOR * E.yardstick(e64s, nn)
                line = "replicate %d T_n %d %-7s seam nodes: e64 %.2e e_gpu %.2e bound %.2e (%d nodes)" % (n, Tn, stage, e64s, e_gpus, bounds, len(ts))
                report.append(line)
                if not (e64s <= E.CAP and e_gpus <= bounds):
                    bad.append(line)
    print("\n".join(report))
    assert not bad, "D %d K %d T %d J %d lengths %r\noutside the envelope:\n%s\nall figures:\n%s" % (D, K, T, J, lengths, "\n".join(bad), "\n".join(report))


@pytest.mark.parametrize("D,K", SHAPES)
def test_seam_columns_against_the_extended_run(plan, D, K):
    """T = 16 (J + 8) + 2: sixteen columns of J + 8 nodes, fifteen of them seam starts."""
    T = 16 * (_J(D, K) + 8) + 2
    _check_sweeps(plan, D, K, T, None, (True,) * N)


@pytest.mark.parametrize("D,K", SMALL)
def test_column_length_exactly_J(plan, D, K):
    """T = 16 J + 2: the edge of the condition.  Column 1 reaches the boundary, columns 2 .. 15 start at seams and every one of
    their nodes is corrected."""
    T = 16 * _J(D, K) + 2
    _check_sweeps(plan, D, K, T, None, (True,) * N)


@pytest.mark.parametrize("D,K", SMALL)
def test_one_node_under_the_edge_warms_up(plan, D, K):
    """T = 16 J - 14: columns of J - 1 nodes, so every column falls back to the warm-up (or the boundary)."""
    T = 16 * _J(D, K) - 14
    _check_sweeps(plan, D, K, T, None, (False,) * N)


@pytest.mark.parametrize("D,K", SMALL)
def test_ragged_lengths_on_either_side_of_the_edge(plan, D, K):
    J = _J(D, K)
    lengths = (16 * J + 2, 16 * J - 14, 16 * (J + 8) + 2)
    _check_sweeps(plan, D, K, max(lengths), lengths, (True, False, True))


@pytest.mark.parametrize("short", [20, "J + 2"])
def test_short_chain_has_no_seam(plan, short):
    """T = 20: columns of two nodes, none of them a seam start (with J >= 30 all of them start at the boundary; this problem's J
    is smaller, so the later ones warm up).  T = J + 2: one node a column and every column that owns one starts at the boundary,
    which reproduces the sequential chain."""
    D, K = 16, 16
    J = _J(D, K)
    T = 20 if short == 20 else min(J, 16) + 2
    cols = plan(T, T, J)
    assert all(s[3] != SEAM for s in cols)
    if short != 20:
        assert all(s[3] == BOUNDARY for s in cols if s[1] > 0) and sum(s[1] for s in cols) == T - 2
    _check_sweeps(plan, D, K, T, None, (False,) * N)


def _any_seam(plan, T, w):
    return [sum(1 for s in plan(T, T, int(J)) if s[3] == SEAM) for J in w[:, 0]]


@pytest.mark.parametrize("D,K", SHAPES)
def test_bound_after_three_iterations_against_the_oracle(plan, D, K):
    T = 16 * (_J(D, K) + 8) + 2
    Y, st0, pri = _cut(D, K, T)
    b = _batch(Y, st0, pri)
    st = O.expand_state(st0, pri, T)
    seams = []
    for it in range(3):
        parts = O.iterate(st, pri, Y)
        b.iterate(1)
        got = b.elbo()
        seams.append(_any_seam(plan, T, b.get_warmup()))
        err = np.abs(got - parts) / np.abs(parts).sum(axis=1, keepdims=True)
        print("iteration %d: seam columns per replicate %r, largest part error %.2e of sum |part|" % (it, seams[-1], err.max()))
        assert np.all(np.isfinite(got)) and np.all(err <= RTOL), "iteration %d: bound parts\n%r\n%r" % (it, got, parts)
    Xg = b.get_state(("X",))["X"]
    b.close()
    assert max(seams[0]) >= 1, "no column started at a seam in the first iteration: the case proves nothing (%r)" % (seams,)
    assert np.abs(Xg - st["X"]).max() <= RTOL * np.abs(st["X"]).max()


@pytest.mark.parametrize("D,K,extra", [(16, 16, 8), (17, 33, 8), (64, 64, 8), (16, 16, 0)])
def test_stagewise_sweeps_equal_iterate(plan, D, K, extra):
    """The stage-wise forward sweep keeps its X rows and corrects them too; iterate's does not write them.  The backward sweep
    that follows reads c_t and the row next to the far boundary in both, and must give the same states bit for bit -- also
    where the columns are exactly J long (extra = 0) and the row next to the far boundary is a seam column's J-th node."""
    J = _J(D, K)
    T = 16 * (J + extra) + 2
    assert sum(1 for s in plan(T, T, J) if s[3] == SEAM) >= 1
    Y, st0, pri = _cut(D, K, T)
    a, b = _batch(Y, st0, pri), _batch(Y, st0, pri)
    a.iterate(1)
    b.sweep("forward"); b.sweep("backward"); b.update_A(); b.update_C(); b.update_Q(); b.update_R()
    Xa, Xb, ea, eb = a.get_state(("X",))["X"], b.get_state(("X",))["X"], a.elbo(), b.elbo()
    a.close(); b.close()
    assert np.array_equal(Xa, Xb), "states differ: largest difference %.3e" % np.abs(Xa - Xb).max()
    assert np.array_equal(ea, eb)
