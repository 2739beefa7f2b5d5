"""CPU: the reference side of tests/test_input_channels_gpu.py, alone -- known inputs (k_inputs.hip) and known regressors
(k_regressors.hip) channel by channel, at the tile edges of the two files (inputs_ref.CHANNEL_CASES, regressors_ref.CHANNEL_CASES).

  * Cap.  For every case the float64 comparator is within CAP = 1e-11 of its long-double run in every unit of
    extended_ref.channel_errors -- chain by chain, channel by channel, end node by end node, part by part of both bounds -- after
    every stage, so 16 max(e64_unit, n 2^-52) never exceeds 1.6e-10 for a unit either.
  * Reach.  The cases reach what their table says, from D, K, P and Pv alone, through pyvb_amd/csrc/geometry.h
    (tests/c/geometry_driver.cpp) where a layout value is named, and through the constants of the two kernel files.
  * Planted defects.  extended_ref.compare_channels, fed a float64 comparator run with one defect planted, flags it where it
    lives -- and two of the defects pass the whole-array comparison of tests/test_inputs_gpu.py on the same trace.
"""
import os
import re
import subprocess

import numpy as np
import pytest

import extended_ref as ER
import inputs_ref as IR
import regressors_ref as RR

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
CASES = [(IR, k) for k in IR.CHANNEL_CASES] + [(RR, k) for k in RR.CHANNEL_CASES]
IDS = [("inputs-" if R is IR else "regressors-") + k for R, k in CASES]


def _shape(R, name):
    """(T, D, K, P, Pv) of a case of either table"""
    c = R.CHANNEL_CASES[name]
    return c[:4] + ((0,) if R is IR else (c[4],))


# ---- the table ---------------------------------------------------------------------------------------------------------------
def test_the_table_of_cases():
    assert {k: v[:4] for k, v in IR.CHANNEL_CASES.items()} == {
        "t48_d5k2p31": (48, 5, 2, 31), "t27_d17k3p17": (27, 17, 3, 17), "t27_d33k32p16": (27, 33, 32, 16), "t48_d64k2p31": (48, 64, 2, 31),
        "t700_d8k8p5_w4": (700, 8, 8, 5), "lengths_d16k10p9": (77, 16, 10, 9)}
    assert {k: v[:5] for k, v in RR.CHANNEL_CASES.items()} == {
        "t48_d17k2p17v16": (48, 17, 2, 17, 16), "t48_d33k1p16v31": (48, 33, 1, 16, 31), "t40_d5k3v33": (40, 5, 3, 0, 33),
        "t40_d5k31v33": (40, 5, 31, 0, 33), "t48_d64k2p24v14": (48, 64, 2, 24, 14), "lengths_d16k10p5v9": (77, 16, 10, 5, 9)}
    for R, name in CASES:
        c = R.CHANNEL_CASES[name]
        ln, split, iters, big = c[-4:]
        assert ln == ((2, 3, 19, 60, 77) if name.startswith("lengths") else None) and split == (4 if name.endswith("_w4") else None)
        assert iters == (1 if c[1] == 64 else 2)            # one long-double iteration at full state width
        # big / small: 1e3 / 1e-3 on the inputs-only cases of full length, 30 and 1 / 30 on every regressors and chain-lengths case
        assert big == (1e3 if R is IR and ln is None else 30.0)
        assert len(R.channel_lengths(name)) == (5 if ln else 2)
        assert 700 * 64 >= c[0] * c[1]
    # the earlier tables and their seeds are untouched
    assert list(IR.CASES) == ["t19_d6k4p2", "t33_d5k15p1", "t77_d16k16p8", "t40_d64k40p12", "t700_d8k8p3_w4", "lengths_d16k10p3"]
    assert list(RR.CASES) == ["t19_d6k4v2", "t19_d6k4p2v1", "t33_d5k14v3", "t77_d16k16p4v8", "t40_d64k40p6v12", "t12_d3k1v63", "t700_d8k8p2v3_w4",
                              "lengths_d16k10p2v3"]
    assert not set(IR.CHANNEL_SEEDS.values()) & set(IR.SEEDS.values()) and not set(RR.CHANNEL_SEEDS.values()) & set(RR.SEEDS.values())


@pytest.mark.parametrize("R,name", CASES, ids=IDS)
def test_the_channels_are_the_named_patterns(R, name):
    T, D, K, P, Pv = _shape(R, name)
    prob = R.channel_problem(name)
    Y, U = prob[0], prob[1]
    V, ulab, vlab = (None, prob[5], None) if R is IR else (prob[2], prob[6], prob[7])
    lengths, big = R.channel_lengths(name), R.CHANNEL_CASES[name][-1]
    from pyvb_amd import synth
    drawn = synth.make_input_problem(T, D, K, P, len(lengths), seed=R.CHANNEL_SEEDS[name])[1] if P else None
    for n, Tn in enumerate(int(t) for t in lengths):
        for a in (Y, U, V):
            if a is not None:       # live padding: finite, and no zero among it
                assert np.all(np.isfinite(a[n])) and np.all(a[n, Tn:] != 0.0)
        assert np.all(prob[2 if R is IR else 3]["X"][n, Tn:] == 0.0)         # X's padding stays zero
        for p in range(P):
            u, k = U[n, 1:Tn, p], p % 8
            assert U[n, 0, p] != 0.0 and ulab[n][p].startswith(IR.U_PATTERNS[k][:7])
            want = {0: drawn[n, 1:Tn, p], 7: drawn[n, 1:Tn, p], 1: drawn[n, 1:Tn, p] * big, 2: drawn[n, 1:Tn, p] / big,
                    3: np.arange(1, Tn) == 1, 4: np.arange(1, Tn) == Tn - 1, 5: np.zeros(Tn - 1), 6: np.ones(Tn - 1)}[k]
            assert np.array_equal(u, np.asarray(want, dtype=float)), (n, p)
            if k in (3, 4):         # where two patterns coincide the label says so
                assert (ulab[n][p] == "impulse at t = 1 = T_n - 1") == (Tn == 2)
        for p in range(Pv):
            v, k = V[n, :Tn, p], p % 8
            assert vlab[n][p] == ("constant 1" if p == 0 else RR.V_PATTERNS[k])
            if p == 0:
                assert np.all(v == 1.0)
            elif k in (3, 4):
                assert np.array_equal(v, (np.arange(Tn) == (0 if k == 3 else Tn - 1)).astype(float))
            else:
                assert np.abs(v).max() > 0 and len(set(v)) == Tn       # drawn: no constant among them
    if P:       # the scales are in the data: a x big channel is big / small times a x small one
        rms = np.sqrt((U[0, 1:int(lengths[-1])] ** 2).mean(0)) if lengths[0] == lengths[-1] else np.sqrt((U[-1, 1:] ** 2).mean(0))
        if P > 2:
            assert 0.2 * big ** 2 < rms[1] / rms[2] < 5 * big ** 2


# ---- 1. the cap ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R,name", CASES, ids=IDS)
def test_float64_comparator_is_within_the_cap_in_every_unit(R, name):
    T, D, K, P, Pv = _shape(R, name)
    ref = ER.channel_reference(R, name)
    iters = R.CHANNEL_CASES[name][-2]
    stages = IR.STAGES if R is IR else RR.stages(P)
    per_iter = sum(len(q) for _, q in stages) + len(ER.BOUND_MODES)
    assert len(ref["keys"]) == per_iter * R.ITERS and len(ref["ext"]) == per_iter * iters == len(ref["e64"])
    assert all(a.dtype == ER.LD for a in ref["ext"])
    worst = {}
    for key, units in zip(ref["keys"], ref["e64"]):
        for (kind, r, idx), e in units.items():
            assert e <= ER.CAP, "%s %r %s replicate %d %r: float64 comparator %.3e from the extended run, cap %.0e" % (name, key, kind, r, idx, e, ER.CAP)
            k = (kind, key[1] == "bound")
            if e >= worst.get(k, (-1.0,))[0]:
                worst[k] = (e, key, r, idx)
    for (kind, bound), (e, key, r, idx) in sorted(worst.items()):
        print("%-22s largest e64 by %-7s%s %.2e at %r replicate %d %r" % (name, kind, " of the bound" if bound else "", e, key, r, idx))
    # every kind of unit is there: a chain unit of every quantity and part, a channel unit of every column, the end nodes
    lengths = ref["lengths"]
    for key, units in zip(ref["keys"], ref["e64"]):
        kinds = {}
        for kind, r, idx in units:
            kinds.setdefault((kind, r), []).append(idx)
        for r, Tn in enumerate(int(t) for t in lengths):
            if key[1] == "bound":
                assert kinds["chain", r] == list(ER.LDS_PARTS)
                continue
            assert kinds["chain", r] == [""]
            if key[2] == "X":
                assert kinds["node", r] == ER.end_nodes(Tn) + (["rest"] if Tn > 4 else []) + (["padding"] if Tn < T else [])
            if key[2] in ER.CHANNEL_QUANTITIES:
                assert kinds["channel", r] == list(range(P if key[2][0] == "B" else Pv))
    # a dead channel with prior mean 0: its mean column is exactly zero in the extended run, after every update of B
    dead = [p for p in range(P) if p % 8 == 5]
    assert len(dead) == {31: 4, 24: 3, 17: 2, 16: 2, 9: 1, 5: 0, 0: 0}[P]
    for key, x in zip(ref["keys"], ref["ext"]):
        if key[2] == "B_mean":
            assert np.all(x[:, :, dead] == 0) and np.all(np.abs(x).max(axis=1)[:, [p for p in range(P) if p not in dead]] > 0)


# ---- 2. reach ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def geometry(tmp_path_factory):
    """pyvb_amd/csrc/geometry.h through tests/c/geometry_driver.cpp: a list of command lines -> the output lines"""
    tmp = tmp_path_factory.mktemp("channel_geometry")
    exe = tmp / "geometry_driver"
    subprocess.run(["g++", "-std=c++17", "-O1", "-I", os.path.join(REPO, "pyvb_amd", "csrc"), os.path.join(HERE, "c", "geometry_driver.cpp"),
                    "-o", str(exe)], check=True, capture_output=True)

    def run(lines):
        (tmp / "in.txt").write_text("".join(ln + "\n" for ln in lines))
        p = subprocess.run([str(exe), str(tmp / "in.txt"), str(tmp / "out.txt")], capture_output=True, text=True)
        assert p.returncode == 0, p.stderr[-2000:]
        return (tmp / "out.txt").read_text().splitlines()
    return run


def _constant(fname, pattern):
    src = open(os.path.join(REPO, "pyvb_amd", "csrc", fname)).read()
    m = re.search(pattern, src)
    assert m, "%s: %s not found" % (fname, pattern)
    return int(m.group(1))


def _reach(D, K, P, Pv, lay):
    """what the kernels of k_inputs.hip and k_regressors.hip loop over at a shape: from D, K, P and Pv, and the layout's DT and KS"""
    K0 = K + 2 * P
    return dict(Kt=K0 + Pv, DT=lay["DT"], KS=lay["KS"], d_last=D - 16 * (lay["DT"] - 1) if lay["DT"] < 4 or D > 48 else None,
                WT=(P + 15) >> 4, w_last=P - 16 * ((P - 1) >> 4) if P else 0, CT=(2 * P + 15) >> 4,
                PT=(Pv + 15) >> 4, v_last=Pv - 16 * ((Pv - 1) >> 4) if Pv else 0, K0=K0, K0_in_tile=K0 % 16, K_in_tile=K % 16)


REACH = {
    # P = IN_PMAX, Kt = 64 at one state tile; two W tiles, CT = 4
    "t48_d5k2p31": dict(Kt=64, DT=1, KS=16, d_last=5, WT=2, w_last=15, CT=4, PT=0, v_last=0, K0=64, K0_in_tile=0, K_in_tile=2),
    # one real column in W's second tile; DT = 2 with one real row
    "t27_d17k3p17": dict(Kt=37, DT=2, KS=16, d_last=1, WT=2, w_last=1, CT=3, PT=0, v_last=0, K0=37, K0_in_tile=5, K_in_tile=3),
    # P a full tile, Kt = 64, the inputs' gain columns (from K on) start on an operand-tile edge
    "t27_d33k32p16": dict(Kt=64, DT=4, KS=16, d_last=None, WT=1, w_last=16, CT=2, PT=0, v_last=0, K0=64, K0_in_tile=0, K_in_tile=0),
    "t48_d64k2p31": dict(Kt=64, DT=4, KS=16, d_last=16, WT=2, w_last=15, CT=4, PT=0, v_last=0, K0=64, K0_in_tile=0, K_in_tile=2),
    "t700_d8k8p5_w4": dict(Kt=18, DT=1, KS=8, d_last=8, WT=1, w_last=5, CT=1, PT=0, v_last=0, K0=18, K0_in_tile=2, K_in_tile=8),
    "lengths_d16k10p9": dict(Kt=28, DT=1, KS=8, d_last=16, WT=1, w_last=9, CT=2, PT=0, v_last=0, K0=28, K0_in_tile=12, K_in_tile=10),
    # all three groups, K0 = 36 inside a tile, Pv a full tile
    "t48_d17k2p17v16": dict(Kt=52, DT=2, KS=16, d_last=1, WT=2, w_last=1, CT=3, PT=1, v_last=16, K0=36, K0_in_tile=4, K_in_tile=2),
    # Kt = 64 with all three groups; PT = 2 with 15 real columns; K0 = 33
    "t48_d33k1p16v31": dict(Kt=64, DT=4, KS=16, d_last=None, WT=1, w_last=16, CT=2, PT=2, v_last=15, K0=33, K0_in_tile=1, K_in_tile=1),
    # PT = 3 with one real column, P = 0
    "t40_d5k3v33": dict(Kt=36, DT=1, KS=16, d_last=5, WT=0, w_last=0, CT=0, PT=3, v_last=1, K0=3, K0_in_tile=3, K_in_tile=3),
    # K + Pv = 64: RE at 1023 of 1024; K = 31 in the clamped loads of the 4-row k-steps
    "t40_d5k31v33": dict(Kt=64, DT=1, KS=16, d_last=5, WT=0, w_last=0, CT=0, PT=3, v_last=1, K0=31, K0_in_tile=15, K_in_tile=15),
    # Kt = 64 at D = 64
    "t48_d64k2p24v14": dict(Kt=64, DT=4, KS=16, d_last=16, WT=2, w_last=8, CT=3, PT=1, v_last=14, K0=50, K0_in_tile=2, K_in_tile=2),
    "lengths_d16k10p5v9": dict(Kt=29, DT=1, KS=8, d_last=16, WT=1, w_last=5, CT=1, PT=1, v_last=9, K0=20, K0_in_tile=4, K_in_tile=10),
}


@pytest.mark.parametrize("R,name", CASES, ids=IDS)
def test_cases_reach_what_the_table_says(R, name, geometry):
    T, D, K, P, Pv = _shape(R, name)
    Kt = K + 2 * P + Pv
    IN_PMAX, RE = _constant("k_known.hip", r"#define IN_PMAX (\d+)"), _constant("k_known.hip", r"__shared__ double RE\[(\d+)\]")
    assert (IN_PMAX, RE) == (31, 1024) and _constant("k_known.hip", r"__shared__ double WV\[64 \* (\d+)\]") == 65
    assert max(D, Kt) <= 64 and P <= IN_PMAX and K * Pv <= RE            # what a handle accepts (include/pyvb_hip.h)
    # the layout is that of D states and Kt = K + 2 P + Pv output channels (api.hip: lds_geometry(N, T, D, K + 2 P + Pv, noise))
    v = [int(x) for x in geometry(["layout %d %d" % (D, Kt)])[0].split("|")[0].split()]
    lay = dict(zip(("D", "K", "DT", "KT", "DP", "KP", "DS", "KS", "QR"), v))
    assert lay["D"] == D and lay["K"] == Kt and lay["QR"] == 64 and lay["DS"] == 4 * lay["DT"]
    got = _reach(D, K, P, Pv, lay)
    print("%-22s %r" % (name, got))
    assert got == REACH[name]
    if name == "t48_d5k2p31":
        assert P == IN_PMAX and (P + 15) >> 4 == 2
    if name == "t27_d17k3p17":          # V's first tile (columns P .. P + 15 of WV) lies over the padding of W's second tile (16 .. 31)
        assert P < 32 and P + 15 >= 17 and 16 < P
    if name == "t40_d5k31v33":
        assert K * Pv == RE - 1 and K + Pv == 64 and (K + 3) >> 2 == 8 and K % 4 == 3      # the last k-step has three real rows
    if name == "t48_d33k1p16v31":
        assert K and P and Pv and Kt == 64
    split = R.CHANNEL_CASES[name][-3]
    if split:       # the impulses at t = 1 and T - 1 land in the first and in the last wavefront's part
        out = geometry(["check %d %d" % (T, split), "parts %d %d %d" % (T, split, T)])
        assert out[0].startswith("0|")
        Lw, live = int(out[1].split("|")[0].split()[0]), int(out[1].split("|")[1])
        assert live == split == 4 and Lw == 176 and (1 - 1) // Lw == 0 and (T - 2 - 1) // Lw == split - 1
        assert 4 % 8 < P        # both impulse channels are there
    if name.startswith("lengths"):      # every pattern in every chain
        assert P >= (8 if R is IR else 5) and (R is IR or Pv >= 5)
        assert [int(t) for t in R.channel_lengths(name)] == [2, 3, 19, 60, 77]


# ---- 3. planted defects --------------------------------------------------------------------------------------------------------
class _NoInputTermAtNode0(IR.Model):
    """-<A>^T <Q> e_1 dropped from the message of X_1 to X_0"""
    _at = None

    def _e(self, t):
        e = IR.Model._e(self, t)
        return 0 * e if self._at == 0 and t == 1 else e

    def _x_step(self, post, t):
        self._at = t
        IR.Model._x_step(self, post, t)


class _SuuFromRow0(IR.Model):
    """Suu summed from t = 0"""

    def __init__(self, Y, U, st0, pri):
        IR.Model.__init__(self, Y, U, st0, pri)
        self.Suu = np.einsum("ntp,ntq->npq", U, U)


class _LiveUNext(IR.Model):
    """the u_{t+1} channel live in the chain's last row: X_{T_n - 1} takes -<A>^T <Q> <B> u_{T_n} from the first padding row"""
    u_next = None

    def _x_step(self, post, t):
        IR.Model._x_step(self, post, t)
        if t == self.T - 1 and self.u_next is not None:
            st = self.st
            e = np.einsum("nkp,np->nk", st["B_mean"], self.u_next)
            w = -np.einsum("nki,nk->ni", st["A_mean"], np.einsum("nkl,nl->nk", post["Qbar"], e))
            st["X"][:, t] += np.einsum("nij,nj->ni", post["Sigma"][:, 2], w)


class _Channel16TakesTheGainOfChannel0(RR.Model):
    """in the sweeps regressor channel 16 enters through column 0 of <E>"""

    def _on_residual(self, fn, *args):
        E = self.st["E_mean"]
        self.st["E_mean"] = E.copy()
        self.st["E_mean"][:, :, 16] = E[:, :, 0]
        try:
            RR.Model._on_residual(self, fn, *args)
        finally:
            self.st["E_mean"] = E


def _offenders(R, name, trace, tag):
    off = ER.offending_units(ER.compare_channels(ER.channel_reference(R, name), trace, tag))
    return off, [o for o in off if o[0] == off[0][0]] if off else []


def _whole_array(R, name, trace):
    """the largest e / (16 y) of the whole-array comparison of tests/test_inputs_gpu.py: test_parity_and_envelope on a trace"""
    ref = ER.channel_reference(R, name)
    T, D, K = _shape(R, name)[:3]
    n, worst = max(T, D, K), 0.0
    for (key, arr), v64, vx in zip(trace, ref["f64"], ref["ext"]):
        if key[1] == "bound":
            e64 = ER.bound_errors(v64, vx)[0]
            worst = max([worst] + [r[4] / ER.FACTOR for r in ER.compare_bound(arr, vx, e64, n)])
        else:
            worst = max(worst, ER.rel(arr, vx) / (ER.FACTOR * ER.yardstick(ER.rel(v64, vx), n)))
    return worst


def test_the_sound_comparator_has_no_unit_out_of_order():
    for R, name in ((IR, "t27_d17k3p17"), (IR, "lengths_d16k10p9"), (RR, "t40_d5k3v33")):
        rows = ER.compare_channels(ER.channel_reference(R, name), R.channel_trace(name), "float64 comparator " + name)
        assert rows and not ER.offending_units(rows) and max(r[6] for r in rows) <= 1.0
        assert _whole_array(R, name, R.channel_trace(name)) <= 1.0 / ER.FACTOR


def test_the_input_term_dropped_at_node_0_is_first_flagged_there():
    name = "t27_d17k3p17"
    off, first = _offenders(IR, name, IR.channel_run(IR.channel_problem(name), iters=1, cls=_NoInputTermAtNode0), "defect: no -A'Q e_1 at node 0")
    assert first and first[0][0] == (0, "forward", "X")
    nodes = {(o[2], o[3]): o[6] for o in first if o[1] == "node"}
    assert (0, 0) in nodes and (1, 0) in nodes
    for r in (0, 1):        # node 0 is where it is largest; the forward sweep carries it on, fading
        assert nodes[r, 0] == max(v for (rr, _), v in nodes.items() if rr == r)


def test_a_live_u_next_channel_in_a_chain_s_last_row_is_flagged_in_the_shorter_chains_alone():
    name = "lengths_d16k10p9"
    prob = IR.channel_problem(name)
    Y, U, st0, pri, ln = prob[:5]
    T = Y.shape[1]
    ms = IR.models(Y, U, st0, pri, ln, _LiveUNext)
    for (n,), m in ms:
        if m.T < T:
            m.u_next = U[n:n + 1, m.T]
    trace = IR.run_stages(lambda stage: [IR.do_stage(m, stage) for _, m in ms], lambda: IR.snapshot(ms, T),
                          lambda mode: np.concatenate([m.elbo_parts(mode) for _, m in ms]), 1)
    off, first = _offenders(IR, name, trace, "defect: u_{t+1} live in the last row")
    assert {o[2] for o in off} == {0, 1, 2, 3}          # the chains of 2, 3, 19 and 60 nodes; not the one of 77
    assert first[0][0] == (0, "forward", "X") and {o[3] for o in first if o[1] == "node" and o[2] == 3} == {59}


def test_suu_summed_from_row_0_takes_the_dead_channel_off_its_prior():
    name = "t27_d17k3p17"
    off, first = _offenders(IR, name, IR.channel_run(IR.channel_problem(name), iters=1, cls=_SuuFromRow0), "defect: Suu from t = 0")
    assert first[0][0] == (0, "B", "B_mean")
    dead = {(o[2], o[3]): o[6] for o in off if o[0] == (0, "B", "B_mean") and o[1] == "channel" and o[3] in (5, 13)}
    assert set(dead) == {(0, 5), (0, 13), (1, 5), (1, 13)} and all(v == np.inf for v in dead.values())      # zero in the extended run
    var = {(o[2], o[3]) for o in off if o[0] == (0, "B", "B_colvar") and o[1] == "channel"}
    assert {(0, 5), (0, 13), (1, 5), (1, 13)} <= var            # and the variance is no longer the prior's


def test_regressor_channel_16_with_the_gain_of_channel_0_is_flagged():
    name = "t40_d5k3v33"
    off, first = _offenders(RR, name, RR.channel_run(RR.channel_problem(name), iters=1, cls=_Channel16TakesTheGainOfChannel0),
                            "defect: channel 16 <- gain of channel 0")
    assert first and first[0][0] == (0, "forward", "X")
    assert {o[1] for o in first} == {"chain", "node"} and {o[2] for o in first} == {0, 1}
    assert [o for o in off if o[0][2] == "E_mean" and o[1] == "channel" and o[3] == 16]


def _scaled(R, name, key, cut):
    """(the float64 trace of one iteration with the part `cut` of the array of `key` times 1 + eps, eps): eps is half of what the
    whole-array bound 16 max(e64, n 2^-52) admits on that array, in units of the part's own largest entry"""
    ref = ER.channel_reference(R, name)
    T, D, K = _shape(R, name)[:3]
    i = ref["keys"].index(key)
    v64, vx = ref["f64"][i], ref["ext"][i]
    eps = 0.5 * ER.FACTOR * ER.yardstick(ER.rel(v64, vx), max(T, D, K)) * float(np.abs(vx).max()) / float(np.abs(vx[cut]).max())
    trace = [(k, a.copy()) for k, a in zip(ref["keys"], ref["f64"])][:len(ref["keys"]) // R.ITERS]
    trace[i][1][cut] *= 1.0 + eps
    return trace, eps


def test_a_column_of_B_under_a_big_input_passes_the_whole_array_and_not_its_channel():
    name, key = "t27_d17k3p17", (0, "B", "B_mean")
    assert IR.channel_problem(name)[5][0][1] == "x big"
    trace, eps = _scaled(IR, name, key, (0, slice(None), 1))
    print("defect: column 1 of B (x big) of replicate 0 times 1 + %.2e" % eps)
    assert 1e-11 < eps < 1e-8           # the suite's RTOL cannot see it either
    assert _whole_array(IR, name, trace) <= 1.0, "the whole-array comparison was to pass"
    off = ER.offending_units(ER.compare_channels(ER.channel_reference(IR, name), trace, "defect: one column of B"))
    assert [o[:4] for o in off] == [(key, "channel", 0, 1)], off


def test_q_b_of_the_two_node_chain_passes_the_stacked_comparison_and_not_its_chain():
    name, key = "lengths_d16k10p9", (0, "Q", "Q_b")
    trace, eps = _scaled(IR, name, key, (0,))
    print("defect: Q_b of the chain of 2 nodes times 1 + %.2e" % eps)
    assert eps < 1e-8
    assert _whole_array(IR, name, trace) <= 1.0, "the stacked comparison was to pass"
    off = ER.offending_units(ER.compare_channels(ER.channel_reference(IR, name), trace, "defect: Q_b of chain 0"))
    assert [o[:4] for o in off] == [(key, "chain", 0, "")], off


def test_unit_errors_on_arrays_whose_answer_is_known():
    LD = ER.LD
    lengths = np.array([2, 5, 7], dtype=np.int32)
    x = np.arange(1.0, 3 * 7 * 4 + 1).reshape(3, 7, 4).astype(LD)
    for r, Tn in enumerate(lengths):
        x[r, Tn:] = 0
    g = x.copy()
    g[1, 3, 2] *= 1 + LD(1e-12)         # T_n - 2 of the chain of 5
    g[2, 3, 0] += LD(1e-9)              # the rest of the chain of 7
    e = ER.channel_errors(g, x, (0, "forward", "X"), lengths)
    assert {k for k in e if k[1] == 0} == {("chain", 0, ""), ("node", 0, 0), ("node", 0, 1), ("node", 0, "padding")}
    assert ("node", 1, "rest") in e and ("node", 2, "padding") not in e
    assert np.isclose(e["node", 1, 3], x[1, 3, 2] * 1e-12 / x[1, 3, 3]) and e["node", 1, "rest"] == 0.0 and e["node", 1, 4] == 0.0
    assert np.isclose(e["node", 2, "rest"], 1e-9 / float(x[2, 4, 3])) and e["chain", 0, ""] == 0.0
    g[0, 4, 1] = 1e-300                 # padding that is not zero
    assert ER.channel_errors(g, x, (0, "forward", "X"), lengths)["node", 0, "padding"] == np.inf
    # a channel: column p of a mean [N, rows, P], row p of the variances [N, P, rows]; a dead column is zero or nothing
    m = np.ones((3, 4, 6), dtype=LD); m[:, :, 5] = 0; m[:, :, 2] = LD(1e-3)
    g = m.copy(); g[1, 3, 2] += LD(1e-15)
    e = ER.channel_errors(g, m, (0, "B", "B_mean"), lengths)
    assert np.isclose(e["channel", 1, 2], 1e-12) and np.isclose(e["chain", 1, ""], 1e-15) and e["channel", 1, 5] == 0.0
    g[2, 0, 5] = -1e-200
    assert ER.channel_errors(g, m, (0, "B", "B_mean"), lengths)["channel", 2, 5] == np.inf
    v = np.ones((3, 6, 4), dtype=LD); g = v.copy(); g[0, 4, 1] *= 1 + LD(1e-13)
    e = ER.channel_errors(g, v, (0, "E", "E_colvar"), lengths)
    assert np.isclose(e["channel", 0, 4], 1e-13) and e["channel", 0, 1] == 0.0


# ---- 4. the kappa-clause on the residual of R ------------------------------------------------------------------------------------
def test_the_kappa_clause_is_one_rounding_of_a_cancelling_sum_and_nothing_else():
    """regressors_ref.KAPPA_CASES: one output, 31 regressors and 33 states on 48 rows.  R_b of replicate 1 is a sum that cancels to a
    five-thousandth of its terms; the allowance that the yardstick takes from it is zero before the first update_R, one rounding
    (kappa 2^-52) on R_b itself, and reaches only what is formed from R_b."""
    assert RR.KAPPA_CASES == ("t48_d33k1p16v31",)
    name = RR.KAPPA_CASES[0]
    ref = ER.channel_reference(RR, name)
    # (kappa once more, from the extended run itself)
    Y, U, V, st0, pri, ln = RR.channel_problem(name)[:6]
    (_, m), = RR.models(ER.to_long(Y), ER.to_long(U), ER.to_long(V), ER.to_long(st0), ER.to_long(pri), ln)
    for stage, _ in RR.stages(16)[:-1]:
        RR.do_stage(m, stage)
    k = RR.residual_condition(m, m.statistics()).astype(float)
    print("kappa of the residual of R, iteration 1: replicate 0 %.0f, replicate 1 %.0f" % (k[0, 0], k[1, 0]))
    assert k.shape == (2, 1) and 1000 < k[0, 0] < k[1, 0] < 10000
    first_R = ref["keys"].index((0, "R", "R_b"))
    for i, (key, cond) in enumerate(zip(ref["keys"], ref["cond"])):
        assert all(0.0 <= v <= ER.CAP for v in cond.values())
        if i < first_R:
            assert not any(cond.values()), key
    assert np.isclose(ref["cond"][first_R]["chain", 1, ""], k[1, 0] * ER.U64, rtol=1e-3)
    # the float64 comparator's own error there says nothing about the sum: it is a hundredth of one rounding of it
    assert ref["e64"][first_R]["chain", 1, ""] < 0.1 * k[1, 0] * ER.U64
    # what the allowance reaches in the second iteration: the columns of C and E, R_b, and L_C -- not the states, A, B or Q
    reached = {key[2] for key, cond in zip(ref["keys"], ref["cond"]) if max(cond.values()) > 48 * ER.U64}
    assert reached == {"R_b", "C_colvar", "E_mean", "E_colvar", "reference"}, reached
    # the comparison still sees a defect in that very unit: R_b of replicate 1 off by a hundred roundings of the sum
    rows = ER.compare_channels(ref, RR.channel_trace(name), "float64 comparator " + name)
    assert not ER.offending_units(rows)
    trace = [(kk, a.copy()) for kk, a in zip(ref["keys"], ref["f64"])]
    trace[first_R][1][1] *= 1.0 + 100 * k[1, 0] * ER.U64
    off = ER.offending_units(ER.compare_channels(ref, trace, "defect: R_b of replicate 1"))
    assert [o[:4] for o in off] == [((0, "R", "R_b"), "chain", 1, "")]
    for R, nm in CASES:
        assert ("cond" in ER.channel_reference(R, nm)) == (nm == name)
