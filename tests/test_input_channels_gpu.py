"""GPU: known inputs (k_inputs.hip) and known regressors (k_regressors.hip) channel by channel, at the tile edges of the two files.

The cases are inputs_ref.CHANNEL_CASES and regressors_ref.CHANNEL_CASES: synth's problems with the channels replaced by named
patterns (x big, x small, impulses at either end, a dead channel, a constant) and with finite random values in row 0 of U and in the
padding rows of U, V and Y.  tests/test_input_channels_cpu.py holds the reference side: the cap, what each case reaches, and that
the comparison flags planted defects where they live.

  * Envelope.  Every case against the comparator's long-double run in the units of extended_ref.compare_channels -- chain by
    chain, channel by channel, end node by end node -- after every stage, the parts of both bounds replicate by replicate:
    e_unit <= 16 max(e64_unit, n 2^-52), n = max(T_n, D, K) of the chain's own length, e64_unit <= 1e-11; a unit that is exactly zero
    in the extended run (the mean column of a dead channel) is exactly zero.  The whole-array comparison of
    tests/test_inputs_gpu.py runs beside it.
  * Bitwise invariances.  Row 0 of U redrawn; the padding rows of U, of V, of Y redrawn, each alone: the whole trace of a second
    handle is bitwise the first's.
  * Setters on a handle that has run.  set_inputs, set_regressors or set_observations after an iteration, then another: bitwise a
    fresh handle given the new data and the state of the first, and inside the envelope of the comparator started from that state.
"""
import numpy as np
import pytest

import extended_ref as ER
import inputs_ref as IR
import regressors_ref as RR
from test_inputs_gpu import _bound, _close, _compare_parts, _do
from test_inputs_gpu import _snapshot as _snapshot_inputs
from test_regressors_gpu import _snapshot as _snapshot_regressors

pytestmark = pytest.mark.gpu

CASES = [(IR, k) for k in IR.CHANNEL_CASES] + [(RR, k) for k in RR.CHANNEL_CASES]
IDS = [("inputs-" if R is IR else "regressors-") + k for R, k in CASES]
_traces = {}


def _parts(R, prob):
    """(Y, U, V or None, st0, pri, lengths) of a problem of either module"""
    return prob[:2] + (None,) + prob[2:5] if R is IR else prob[:6]


def _handle(R, prob, split=None):
    from pyvb_amd.lds import LDSBatch
    Y, U, V, st0, pri, ln = _parts(R, prob)
    b = LDSBatch.from_problem(Y, st0, pri, lengths=ln, U=U, V=V)
    if split:
        b.set_time_split(split)
        assert b.get_time_split() == split
    return b


def _snapshot(R, b):
    return _snapshot_inputs(b) if R is IR else _snapshot_regressors(b)


def _trace(R, b, iters):
    """run_stages on a handle: every quantity after the stage that produces it, the parts of both bounds after each iteration"""
    args = (lambda stage: _do(b, stage), lambda: _snapshot(R, b), lambda mode: _bound(b, mode), iters)
    return IR.run_stages(*args) if R is IR else RR.run_stages(*(args + (b.P,)))


def _case_trace(R, name):
    """the trace of a case's handle, ITERS iterations; run once, shared between the tests: do not write to the arrays"""
    if (R, name) not in _traces:
        b = _handle(R, R.channel_problem(name), R.CHANNEL_CASES[name][-3])
        _traces[R, name] = _trace(R, b, R.ITERS)
        b.close()
    return _traces[R, name]


def _bitwise(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))


# ---- 1. the envelope, unit by unit ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R,name", CASES, ids=IDS)
def test_envelope_by_chain_channel_and_end_node(R, name):
    """Largest e_unit / y measured on an MI355X (profiles/accuracy_envelope.txt; the bound is 16): see DESIGN.md sections 26 and 27."""
    c = R.CHANNEL_CASES[name]
    T, D, K = c[:3]
    n = max(T, D, K)
    ref = ER.channel_reference(R, name)
    got = _case_trace(R, name)
    assert [k for k, _ in got] == ref["keys"]
    # the whole-array comparison of tests/test_inputs_gpu.py: parity with the float64 comparator, and the envelope with the replicates stacked
    failures = []
    for i, ((key, g), v64) in enumerate(zip(got, ref["f64"])):
        it, stage, q = key
        what = "%s iteration %d %s %s" % (name, it + 1, stage, q)
        if stage == "bound":
            for r in range(g.shape[0]):
                _compare_parts(g[r], v64[r], "%s replicate %d" % (what, r), q == "exact")
        else:
            _close(g, v64, what)
        if i >= len(ref["ext"]):        # D = 64: the long-double run has one iteration; the second is held to parity above
            assert D == 64 and it == 1
            continue
        vx = ref["ext"][i]
        if stage == "bound":
            e64 = ER.bound_errors(v64, vx)[0]
            assert e64.max() <= ER.CAP
            cond = ref["cond"][i] if "cond" in ref else {}          # (regressors_ref.KAPPA_CASES: the clause on the residual of R)
            for r, p, e6, eg, ratio, own in ER.compare_bound(g, vx, e64, n):
                if not eg <= ER.FACTOR * max(ER.yardstick(e6, n), cond.get(("chain", r, ER.LDS_PARTS[p]), 0.0)):
                    failures.append((what, r, ER.LDS_PARTS[p], e6, eg, ratio))
        else:
            e64, e_gpu = ER.rel(v64, vx), ER.rel(g, vx)
            y = ER.yardstick(e64, n)
            print("%-52s WHOLE e64 %.2e  e_gpu %.2e  (%.2f y)" % (what, e64, e_gpu, e_gpu / y))
            assert e64 <= ER.CAP
            if not e_gpu <= ER.FACTOR * y:
                failures.append((what, e64, e_gpu, e_gpu / y))
    # the units
    rows = ER.compare_channels(ref, got, "CHANNELS " + name)
    assert rows and {r[1] for r in rows} == set(ER.CHANNEL_KINDS)
    assert max(r[4] for r in rows) <= ER.CAP
    off = ER.offending_units(rows)
    assert not failures and not off, (failures, off[:20])


def test_a_dead_channel_stays_on_its_prior():
    """the mean column of a channel that is nonzero in row 0 alone is exactly zero and its variances are the prior's, after every
    update of B, on every case that has such a channel (prior mean 0, prior precision 1e-3)"""
    seen = 0
    for R, name in CASES:
        P = R.CHANNEL_CASES[name][3]
        dead = [p for p in range(P) if p % 8 == 5]
        if not dead:
            continue
        pp = R.channel_problem(name)[3 if R is IR else 4]["B_prior_prec"]
        for key, g in _case_trace(R, name):
            if key[2] == "B_mean":
                assert np.all(g[:, :, dead] == 0.0), (name, key)
                seen += len(dead)
            if key[2] == "B_colvar":
                want = np.broadcast_to(1.0 / pp[dead], g[:, dead].shape)
                assert np.all(np.abs(g[:, dead] - want) <= np.spacing(want)), (name, key)
    assert seen >= 4


# ---- 2. what is never read changes nothing, bitwise ----------------------------------------------------------------------------
def _redrawn(R, name, what):
    """the case's problem with one thing drawn anew, as finite values: row 0 of U, or the padding rows of U, of V, of Y"""
    prob = list(R.channel_problem(name))
    lengths = R.channel_lengths(name)
    rng = np.random.default_rng(9000 + len(what))
    i = {"U row 0": 1, "U padding": 1, "V padding": 2, "Y padding": 0}[what]
    a = prob[i].copy()
    if what == "U row 0":
        a[:, 0] = 7.0 * rng.standard_normal(a[:, 0].shape)
    else:
        pad = np.arange(a.shape[1])[None, :] >= lengths[:, None]
        assert pad.any()
        a[pad] = 1e3 * rng.standard_normal((int(pad.sum()), a.shape[2]))
    assert not np.array_equal(a, prob[i]) and np.all(np.isfinite(a))
    prob[i] = a
    return tuple(prob)


INVARIANCES = [(IR, "lengths_d16k10p9", w) for w in ("U row 0", "U padding", "Y padding")] \
    + [(RR, "lengths_d16k10p5v9", w) for w in ("U row 0", "U padding", "V padding", "Y padding")] \
    + [(RR, "t48_d17k2p17v16", "U row 0")]


@pytest.mark.parametrize("R,name,what", INVARIANCES, ids=["%s-%s" % (n, w.replace(" ", "_")) for _, n, w in INVARIANCES])
def test_rows_that_are_never_read_change_nothing(R, name, what):
    want = _case_trace(R, name)
    b = _handle(R, _redrawn(R, name, what), R.CHANNEL_CASES[name][-3])
    got = _trace(R, b, R.ITERS)
    b.close()
    assert [k for k, _ in got] == [k for k, _ in want]
    bad = [k for (k, g), (_, w) in zip(got, want) if not _bitwise(g, w)]
    assert not bad, "%s redrawn: not bitwise the same in %r" % (what, bad)


# ---- 3. setters on a handle that has run ---------------------------------------------------------------------------------------
STATE_KEYS = ("X", "A_mean", "A_colvar", "C_mean", "C_colvar", "Q_b", "R_b", "B_mean", "B_colvar", "E_mean", "E_colvar")
SETTERS = [(IR, "t27_d17k3p17", "set_inputs"), (IR, "t27_d17k3p17", "set_observations"), (RR, "t48_d17k2p17v16", "set_inputs"),
           (RR, "t48_d17k2p17v16", "set_regressors"), (RR, "t48_d17k2p17v16", "set_observations")]


def _new_data(R, name, setter):
    """(the argument of the setter, the problem's data with it in place): the old data times 1 + 0.1 N(0, 1) plus 0.05 N(0, 1), the
    constant regressor kept"""
    Y, U, V = _parts(R, R.channel_problem(name))[:3]
    rng = np.random.default_rng(R.CHANNEL_SEEDS[name] + 2)
    old = {"set_inputs": U, "set_regressors": V, "set_observations": Y}[setter]
    new = old * (1.0 + 0.1 * rng.standard_normal(old.shape)) + 0.05 * rng.standard_normal(old.shape)
    if setter == "set_regressors":
        new[:, :, 0] = 1.0
    return new, {"set_inputs": (Y, new, V), "set_regressors": (Y, U, new), "set_observations": (new, U, V)}[setter]


def _everything(R, b):
    """everything in get_state, get_input_state and get_regressor_state, the posterior classes, and the six parts in both modes"""
    out = dict(b.get_state())
    out.update(b.get_input_state())
    if b.Pv:
        out.update(b.get_regressor_state())
    out["Sigma"], out["qld_x"] = b.get_posterior_classes()
    for mode in ER.BOUND_MODES:
        out["bound " + mode] = _bound(b, mode)
    return out


def _end_trace(R, g):
    """what a handle holds after an iteration under the keys of run_stages: every quantity is the one its stage left (X the backward
    sweep's), so this is the trace without the forward sweep's X"""
    stages = IR.STAGES if R is IR else RR.stages(1)
    return [((0, stage, q), g[q]) for stage, keys in stages[1:] for q in keys] + [((0, "bound", m), g["bound " + m]) for m in ER.BOUND_MODES]


@pytest.mark.parametrize("R,name,setter", SETTERS, ids=["%s-%s" % (n, s) for _, n, s in SETTERS])
def test_a_setter_on_a_handle_that_has_run(R, name, setter):
    prob = R.channel_problem(name)
    Y, U, V, st0, pri, ln = _parts(R, prob)
    T, D, K = R.CHANNEL_CASES[name][:3]
    new, (Y2, U2, V2) = _new_data(R, name, setter)
    h1 = _handle(R, prob)
    h1.iterate(1)
    st1 = {k: v for k, v in h1.get_state().items() if k in STATE_KEYS}
    getattr(h1, setter)(new)
    h1.iterate(1)
    g1 = _everything(R, h1)
    h1.close()
    prob2 = (Y2, U2, st1, pri, ln) if R is IR else (Y2, U2, V2, st1, pri, ln)
    h2 = _handle(R, prob2)
    h2.iterate(1)
    g2 = _everything(R, h2)
    h2.close()
    assert set(g1) == set(g2) and {"X", "B_mean", "qld_B", "lnd_B", "Q_a", "R_a", "bound exact"} <= set(g1) and (R is IR or "lnd_E" in g1)
    bad = [k for k in g1 if not _bitwise(g1[k], g2[k])]
    assert not bad, "%s on a handle that has run is not a fresh handle with that data: %r differ" % (setter, bad)
    # the comparator started from that same state, in float64 and cast up
    ref = ER.channel_reference_of(R, prob2, 1)
    cap = max(e for units in ref["e64"] for e in units.values())
    print("SETTER %s %s: largest e64_unit of the comparator from the handle's state %.2e" % (name, setter, cap))
    assert cap <= ER.CAP
    rows = ER.compare_channels(ref, _end_trace(R, g1), "SETTER %s %s" % (name, setter))
    assert len(rows) > 100 and not ER.offending_units(rows), ER.offending_units(rows)[:20]
    for (key, v64), vx in zip(zip(ref["keys"], ref["f64"]), ref["ext"]):        # and the whole arrays, as everywhere
        if key == (0, "forward", "X"):
            continue
        g = g1[key[2] if key[1] != "bound" else "bound " + key[2]]
        if key[1] == "bound":
            over = [r for r in ER.compare_bound(g, vx, ER.bound_errors(v64, vx)[0], max(T, D, K)) if not r[4] <= ER.FACTOR]
            assert not over, (key, over)
        else:
            _close(g, v64, "%s %s after %s" % (name, key[2], setter))
            assert ER.rel(g, vx) <= ER.FACTOR * ER.yardstick(ER.rel(v64, vx), max(T, D, K)), key
