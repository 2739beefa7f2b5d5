"""CPU-only: the update flow of an LDS handle with regressors in the output equation (pyvb_lds_create_regressors) -- the steps of
k_known.hip that pyvb_amd/csrc/lds_flow.h takes for side 1, the output equation.  tests/c/lds_flow_driver.cpp is the one driver of
both flow tests: its recorder prints the steps of the known channels as in_* (side 0) and rg_* (side 1), and `init` takes Pv as a
seventh number; it is a stand-alone program, built
here with the address and undefined-behaviour sanitizers (runtimes linked statically), and nothing is loaded into Python.  The model
is that of tests/test_lds_flow_cpu.py, a version counter per primary quantity, with E among the parameters:

    gains, U     also from E                     rg_gains right behind prep (and in_gains)
    stats        formed by rg_moments, the last step of the statistics
    H_C          from the sums and E             rg_HC before every update of the columns of C and every residual of R
    resR         also from E                     resid 1 then rg_resR; C and R share no launch

It pins the steps of an iteration for P = 0, Pv > 0 and for P > 0, Pv > 0, that update_E drops the gains and the residual of R, the
errors of a handle that does not have its regressors yet, and holds seeded random call sequences to the model.
"""
import os
import subprocess

import numpy as np
import pytest

import test_lds_flow_cpu as FL
from test_lds_flow_cpu import BWD, CSRC, E_ARG, E_STALE, FWD, HERE, NO_CLASSES, SAN, SUMS_STEPS, SWEEPS, Flagged

PARAMETERS = FL.PARAMETERS + ("E",)
SOURCES = dict(FL.SOURCES)
SOURCES.update({"gains": PARAMETERS, "U": PARAMETERS + ("Y", "X"), "resR": FL.SOURCES["resR"] + ("E",), "HC": FL.SUMS + ("E", "given")})
RG_STEPS = ("rg_gains", "rg_moments", "rg_HC", "rg_colsE", "rg_resR", "rg_elbo")


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("lds_flow_regressors")
    probe = tmp / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    if subprocess.run(SAN + [str(probe), "-o", str(tmp / "probe")], capture_output=True).returncode != 0:
        pytest.skip("this compiler cannot link the static sanitizer runtimes")
    exe = tmp / "lds_flow_regressors_driver"
    subprocess.run(SAN + ["-Wall", "-I", CSRC, os.path.join(HERE, "c", "lds_flow_driver.cpp"), "-o", str(exe)], check=True, capture_output=True)

    def run(commands):
        """commands: lists of a word and integers.  Returns, per command, [the command, its steps, the error or None, the state after it]."""
        (tmp / "in.txt").write_text("".join(" ".join(str(x) for x in c) + "\n" for c in commands))
        p = subprocess.run([str(exe), str(tmp / "in.txt"), str(tmp / "out.txt")], capture_output=True, text=True)
        assert p.returncode == 0, "the sanitized driver failed:\n" + p.stderr[-4000:]
        calls = []
        for line in (tmp / "out.txt").read_text().split("\n")[:-1]:
            if line.startswith("> "):
                calls.append([line[2:].split(), [], None, None])
            elif line.startswith("= "):
                calls[-1][3] = [int(x) for x in line[2:].split()]
            elif line.startswith("! "):
                calls[-1][2] = (int(line.split()[1]), line.split(" ", 2)[2])
            else:
                calls[-1][1].append(line.split())
        assert len(calls) == len(commands) and all(c[3] is not None for c in calls)
        return calls
    return run


class Model(FL.Model):
    """test_lds_flow_cpu.Model with the regressors: the steps of k_regressors.hip, and what the others must do beside them."""

    def __init__(self, T, N, D, P, dense, big, Pv):
        FL.Model.__init__(self, T, N, D, P, dense, big)
        self.Pv = Pv
        self.v["E"] = 0
        self.regressors_set = self.regressor_priors_set = False

    def now(self, buf):
        return tuple(self.v[s] for s in SOURCES[buf])

    def ready(self):
        return self.regressors_set and self.regressor_priors_set

    def step(self, s, fail):
        kind = s[0]
        a = [int(x) for x in s[1:] if x.lstrip("-").isdigit()]
        if kind in RG_STEPS:
            if not self.Pv:
                fail("%s on a handle without regressors" % kind)
            if self.expect_next:
                want = self.expect_next.pop(0)
                if s[:len(want)] != want:
                    fail("%s must follow here, not %s" % (" ".join(want), " ".join(s)))
            elif kind in ("rg_gains", "rg_moments", "rg_resR", "rg_elbo"):
                fail("%s where nothing asks for it" % " ".join(s))
            if self.lost_x:
                fail("%s after a forward sweep that did not write its states out" % kind)
            if kind in ("rg_moments", "rg_gains") and not self.ready():
                fail("%s on a handle with regressors before it has them" % kind)
            if kind == "rg_moments":
                self.form("stats")
            elif kind in ("rg_HC", "rg_colsE"):
                if not self.current("stats"):
                    fail("%s reads the statistics, which are not current" % kind)
                if kind == "rg_HC":
                    self.form("HC")
                else:
                    self.bump("E")
            elif kind == "rg_resR":
                self.form("resR")
            return
        if not self.Pv:
            return FL.Model.step(self, s, fail)
        # the steps a handle without regressors has too: what they read of the regressors before, what must follow behind
        if kind == "prep" and not self.ready():
            fail("prep on a handle with regressors before it has them")
        if kind == "cols":
            which, c0, c1, fuse = a
            if which == 2:
                fail("A and C share no launch on a handle with regressors")
            if which == 1:
                if fuse:
                    fail("C and R share no launch on a handle with regressors: E sits between them")
                if not self.current("HC"):
                    fail("cols 1 reads H_C, which is not of the current sums and E")
            elif fuse:          # A and Q in one launch where no input stands between them: the model of the fused launch, for A
                if self.expect_next:
                    fail("%s must follow here, not %s" % (" ".join(self.expect_next[0]), " ".join(s)))
                if self.P or (fuse, c0, c1) != (3, 0, self.D):
                    fail("fuse")
                if not self.current("stats"):
                    fail("cols reads the statistics, which are not current")
                self.bump("A"); self.form("resQ"); self.bump("Q")
                return
        if kind == "resid" and a[0] == 1 and not self.current("HC"):
            fail("resid 1 reads H_C, which is not of the current sums and E")
        FL.Model.step(self, s, fail)
        if kind == "prep":
            self.expect_next = self.expect_next + [["rg_gains"]]
        elif kind == "stats":
            self.expect_next = self.expect_next + [["rg_moments"]]
        elif (kind == "tie" and s[1] == "moments") or kind == "in_moments":
            self.formed.pop("stats", None)              # not before rg_moments
        elif kind == "resid" and a[0] == 1:
            self.formed.pop("resR", None)               # not before rg_resR
            self.expect_next = self.expect_next + [["rg_resR"]]
        elif kind == "elbo":
            self.expect_next = self.expect_next + [["rg_elbo", s[1]]]

    def after(self, cmd, err):
        if err is None and cmd[0] == "regressors":
            self.bump("Y"); self.regressors_set = True
        elif err is None and cmd[0] == "regressor_priors":
            self.bump("given"); self.regressor_priors_set = True
        elif err is None and cmd[0] == "regressor_state":
            self.bump("given")
        else:
            FL.Model.after(self, cmd, err)


UPDATES = FL.UPDATES + ("E",)


def replay(calls):
    """test_lds_flow_cpu.replay over the model above; PYVB_E_ARG exactly where inputs or regressors are missing."""
    m, steps = None, 0
    for i, (cmd, trace, err, st) in enumerate(calls):
        if cmd[0] == "init":
            m = Model(*(int(x) for x in cmd[1:8]))
        for j, s in enumerate(trace):
            def fail(why, j=j):
                raise Flagged(i, j, why + "  (%s)" % " ".join(cmd))
            m.step(s, fail)
            steps += 1

        def fail(why):
            raise Flagged(i, len(trace), why + "  (%s)" % " ".join(cmd))
        if m.expect_next:
            fail("%s must follow" % " ".join(m.expect_next[0]))
        if m.lost_x:
            fail("the call ends after a forward sweep that did not write its states out")
        if cmd[0] in UPDATES and m.running() == 0 and [s for s in trace if s != ["join_elbo"]]:
            fail("steps with no replicate running")
        if err is not None:
            code, text = err
            if code == E_STALE:
                if m.current("stats"): fail("PYVB_E_STALE though the statistics are current")
                if not m.has_classes:
                    if not text.startswith(NO_CLASSES): fail("the model has no classes: " + text)
                else:
                    k = "%d of %d X_t were updated since the parameters changed" % (m.fresh(), m.T)
                    if len(set(m.xgen)) < 2 or not text.startswith(k): fail("the model's X_t belong to %d gains, k = %d: %s" % (len(set(m.xgen)), m.fresh(), text))
            elif code == E_ARG:
                no_inputs = m.P and not (m.inputs_set and m.input_priors_set)
                if not (no_inputs or (m.Pv and not m.ready())): fail("PYVB_E_ARG: " + text)
                if not no_inputs and "regressor" not in text: fail("the regressors are missing: " + text)
            else:
                fail("status %d" % code)
        m.after(cmd, err)
        m.check_state(st, fail)
    return steps


# ---- the classes of handle: name -> (P, Pv), and the commands that make one ready for its first update
CLASSES = {"regressors": (0, 2), "both": (2, 3)}


def _start(name, T, N, D):
    P, Pv = CLASSES[name]
    cmds = [["init", T, N, D, P, 0, 0, Pv], ["priors"], ["observations", 0]]
    if P:
        cmds += [["inputs"], ["input_priors"], ["input_state"]]
    return cmds + [["regressors"], ["regressor_priors"], ["regressor_state"], ["state", 1, 0, 1]]


# ---- the step list of one pyvb_lds_iterate from a handle that has iterated before (D = 3); the bound goes to the side stream (1).
# DESIGN.md section 27 has a copy.
ITERATION = {
    "regressors": ["prep", "rg_gains"] + SWEEPS[1:] + SUMS_STEPS + ["rg_moments", "cols 0 0 3 3", "rg_HC", "cols 1 0 3 0", "rg_colsE", "rg_HC",
                                                                    "resid 1", "rg_resR", "noise 1", "elbo 1", "rg_elbo 1"],
    "both": ["prep", "in_gains", "rg_gains"] + SWEEPS[1:] + SUMS_STEPS + ["in_moments", "rg_moments", "in_HA", "cols 0 0 3 0", "in_colsB", "rg_HC",
                                                                          "cols 1 0 3 0", "rg_colsE", "in_HA", "resid 0", "in_resQ", "noise 0", "rg_HC",
                                                                          "resid 1", "rg_resR", "noise 1", "elbo 1", "in_elbo 1", "rg_elbo 1"],
}


@pytest.mark.parametrize("name", sorted(ITERATION))
def test_the_steps_of_an_iteration(driver, name):
    calls = driver(_start(name, 5, 2, 3) + [["iterate", 1], ["iterate", 1], ["iterate", 2]])
    replay(calls)
    text = [[" ".join(s) for s in trace] for _, trace, _, _ in calls]
    assert text[-3] == ITERATION[name]          # the first iteration too: nothing was current, and nothing is formed twice
    assert text[-2] == ITERATION[name]
    assert text[-1] == ITERATION[name] * 2


def test_the_order_is_forward_backward_As_Bs_Cs_Es_Q_R_bound():
    for name, steps in ITERATION.items():
        pos = [steps.index(s) for s in ["sweep 0 0 0 0", "sweep 1 1 1 1"] + (["cols 0 0 3 0", "in_colsB"] if CLASSES[name][0] else ["cols 0 0 3 3"])
               + ["cols 1 0 3 0", "rg_colsE"] + (["noise 0"] if CLASSES[name][0] else []) + ["noise 1", "elbo 1"]]
        assert pos == sorted(pos), (name, pos)


@pytest.mark.parametrize("name", sorted(CLASSES))
def test_update_E_drops_the_gains_and_the_residual_of_R(driver, name):
    cmds = _start(name, 5, 2, 3) + [["iterate", 1], ["elbo"], ["E"], ["elbo"], ["sweep", FWD]]
    calls = driver(cmds)
    replay(calls)
    text = [[" ".join(s) for s in trace] for _, trace, _, _ in calls]
    rg = ["rg_elbo 0"]
    both = ["in_elbo 0"] if CLASSES[name][0] else []
    assert text[-4] == ["elbo 0"] + both + rg                                       # everything is current after an iteration
    gains, resQ, resR = (lambda st: (st[1], st[4], st[5]))(calls[-4][3])
    assert (gains, resQ, resR) == (0, 1, 1)                                         # (R's update dropped the gains)
    assert text[-3] == ["rg_colsE"]
    assert (calls[-3][3][1], calls[-3][3][3], calls[-3][3][4], calls[-3][3][5]) == (0, 1, 1, 0)     # gains, stats, resQ, resR
    assert text[-2] == ["rg_HC", "resid 1", "rg_resR", "elbo 0"] + both + rg          # the residual of R again, that of Q not
    assert text[-1][:2 + len(both)] == ["prep"] + (["in_gains"] if both else []) + ["rg_gains"]
    # E after a forward sweep: the gains are current until E changes
    calls = driver(_start(name, 5, 2, 3) + [["iterate", 1], ["sweep", FWD], ["sweep", BWD], ["E"], ["x", 2]])
    replay(calls)
    assert calls[-3][3][1] == 1 and calls[-2][3][1] == 0 and calls[-1][1][0] == ["prep"]


def test_a_handle_with_regressors_before_it_has_them(driver):
    calls = driver([["init", 4, 1, 2, 0, 0, 0, 2], ["priors"], ["observations", 0], ["sweep", FWD], ["regressors"], ["sweep", FWD], ["regressor_priors"],
                    ["sweep", FWD]])
    replay(calls)
    assert [c[2][0] if c[2] else 0 for c in calls[3:]] == [E_ARG, 0, E_ARG, 0, 0]
    assert "pyvb_lds_set_regressors" in calls[3][2][1] and "pyvb_lds_set_regressor_priors" in calls[5][2][1]
    assert [" ".join(s) for s in calls[7][1]] == ["prep", "rg_gains", "sweep 0 0 0 1", "swap_classes"]
    assert calls[3][1] == [] and calls[5][1] == []          # refused before any step
    # with inputs too: theirs are asked for first, and the statistics ask as the gains do
    calls = driver([["init", 4, 1, 2, 2, 0, 0, 2], ["priors"], ["observations", 0], ["regressors"], ["regressor_priors"], ["sweep", FWD], ["inputs"],
                    ["input_priors"], ["classes"], ["E"]])
    replay(calls)
    assert calls[5][2][0] == E_ARG and "pyvb_lds_set_inputs" in calls[5][2][1]
    assert [" ".join(s) for s in calls[9][1]] == ["stats 1", "moments 0", "tie moments", "in_moments", "rg_moments", "rg_colsE"]
    calls = driver([["init", 4, 1, 2, 0, 0, 0, 2], ["priors"], ["observations", 0], ["classes"], ["E"], ["cols", 1, 0, 2], ["R"], ["elbo"]])
    replay(calls)
    assert all(c[2] and c[2][0] == E_ARG and "pyvb_lds_set_regressors" in c[2][1] for c in calls[4:])


def _random_call(rng, name, T, N, D, st):
    """test_lds_flow_cpu's generator for a handle with inputs (no missing outputs, no known entries, no parents), with the
    regressors' entries in the place of the inputs' throughout where there are none, and half of the time otherwise"""
    P, Pv = CLASSES[name]
    c = FL._random_call(rng, "inputs", T, N, D, st)
    swap = {"B": "E", "inputs": "regressors", "input_state": "regressor_state"}
    if c[0] in swap and (not P or rng.random() < 0.5):
        return [swap[c[0]]] + c[1:]
    if c[0] == "Q" and rng.random() < 0.3:
        return ["E"]
    return c


def test_random_call_sequences_against_the_model(driver):
    rng = np.random.default_rng(2027)
    cmds = []
    for name in CLASSES:
        for _ in range(60):
            T, N, D = int(rng.integers(2, 6)), int(rng.integers(1, 5)), int(rng.integers(1, 4))
            st = dict(on=[1] * N, conv=[0] * N, missing=0, parents=None)
            cmds += _start(name, T, N, D)
            cmds += [_random_call(rng, name, T, N, D, st) for _ in range(int(rng.integers(5, 40)))]
            cmds.append(["get_state"])
    assert 2000 < len(cmds) < 8000
    calls = driver(cmds)
    steps = replay(calls)
    assert steps > len(cmds)
    seen = {s[0] for _, trace, _, _ in calls for s in trace}
    assert seen >= set(RG_STEPS) | {"prep", "in_gains", "sweep", "step", "swap_classes", "stats", "moments", "tie", "in_moments", "in_HA", "in_colsB",
                                    "in_resQ", "resid", "cols", "noise", "elbo", "in_elbo", "carry", "form_lnd_x", "join_elbo", "converge", "copy",
                                    "stage", "mask"}, seen
    errors = [e[1] for _, _, e, _ in calls if e is not None]
    assert any(t.startswith(NO_CLASSES) for t in errors) and any("X_t were updated since the parameters changed" in t for t in errors)


# ---- planted defects: a passing transcript, mutated; the model flags each at its step
@pytest.mark.parametrize("defect", ["drop rg_gains", "drop rg_HC before the residual of R", "fuse C with R", "drop rg_resR"])
def test_planted_defects_are_flagged_at_their_step(driver, defect):
    calls = driver(_start("regressors", 4, 2, 3) + [["iterate", 1], ["E"], ["R"]])
    replay(calls)
    i = len(calls) - 3
    if defect == "drop rg_gains":
        j = FL._find(calls, ["iterate", 1], ["rg_gains"])[1]
        bad = FL._mutated(calls, i, j)
    elif defect == "drop rg_HC before the residual of R":
        i = len(calls) - 1
        assert [" ".join(s) for s in calls[i][1]] == ["rg_HC", "resid 1", "rg_resR", "noise 1"]
        j, bad = 0, FL._mutated(calls, i, 0)
    elif defect == "fuse C with R":
        j = FL._find(calls, ["iterate", 1], ["cols", "1"])[1]
        bad = FL._mutated(calls, i, j, ["cols", "1", "0", "3", "3"])
    else:
        j = FL._find(calls, ["iterate", 1], ["rg_resR"])[1]
        bad = FL._mutated(calls, i, j)
        j += 0          # flagged where noise 1 stands in the place of rg_resR
    with pytest.raises(Flagged) as e:
        replay(bad)
    assert (e.value.call, e.value.step) == (i, j), str(e.value)
