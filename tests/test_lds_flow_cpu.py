"""CPU-only: the update flow of an LDS handle -- which kernels a call launches, decided from the host-side state -- needs no device
(pyvb_amd/csrc/lds_flow.h over LdsState of lds_state.h).  tests/c/lds_flow_driver.cpp instantiates LdsFlow itself, the header that is
compiled into the library, over a device that writes one line per step, and is built here with the address and undefined-behaviour
sanitizers (runtimes linked statically, as tests/test_pca_plan_cpu.py builds its driver); nothing is loaded into Python.  This file
keeps a model beside it that does not use the flags: a version counter per primary quantity (the states, the outputs, the columns of
A / B / C, the noise posteriors, what the caller gave of priors and posteriors, column covariances the caller gave, the covariance
classes), for every derived buffer the versions it was formed from (SOURCES below is the table of DESIGN.md section 14), per X_t the
gains it was last updated under, and where the states and the rows of replicates out of the run are.  It holds every step of scripted
and seeded random call sequences to:

* currency: a step that reads a derived buffer reads one formed from the current versions of its sources;
* minimality: prep, wexpect, stats / moments and the residual steps run only when their output is stale (EXCEPTIONS names what the
  flow launches although its output may be current);
* classes: swap_classes exactly when every X_t has come to be updated under the current gains; the two PYVB_E_STALE refusals exactly
  when the model has no classes / when its X_t belong to different gains, with the model's k;
* buffers: every sweep reads the buffer that holds the states; no copy, staging or change of mask while rows sit on the other side of a
  ping-pong; carry steps exactly then and never with every replicate running; with none running the update entries emit nothing;
* the step list of one iteration per class of handle (ITERATION, copied into DESIGN.md section 14);
* state: the state after every call is what the model derives.

Five defects planted into a passing transcript (not into the header) are each flagged at their step.
"""
import os
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
CSRC = os.path.join(REPO, "pyvb_amd", "csrc")
SAN = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan"]
FWD, BWD = 0, 1
GAMMA, DIAGONAL_GAMMA = 1, 2
E_ARG, E_STALE = 1, 4
NO_CLASSES = "the posterior covariances of the X_t are undefined before the first complete sweep"

# what every derived buffer is computed from
PARAMETERS = ("A", "B", "C", "Q", "R", "given")
SUMS = ("X", "Y", "cls")
SOURCES = {
    "gains": PARAMETERS,                        # with Sigma_new / qld_x_new / lnd_x_new; Wishart: QA, RC, trA, trC; inputs: in_gains
    "expect": ("Q", "R"),                       # Wishart: Qbar, Rbar, lnd
    "stats": SUMS,                              # stats, mom (tie; inputs: in_moments)
    "resQ": SUMS + ("A", "B", "given"),         # Wishart: RQ
    "resR": SUMS + ("C", "given"),              # Wishart: RR
    "sg0": SUMS + ("A", "cov"),                 # Wishart: SG of A / of C
    "sg1": SUMS + ("C", "cov"),
    "U": PARAMETERS + ("Y", "X"),               # the c_t of the forward sweep right before
    "sxx": ("X",),                              # of the backward sweep that read U
    "HA": SUMS + ("B", "given"),                # inputs: H_A = Sx1x - <B> Su1x
}

# What the flow launches although the model says its output is current.  Behaviour is unchanged, so the launches stay.
EXCEPTIONS = {
    "in_HA": "H_A has no field in LdsState: it is formed before every update of the columns of A and every residual of Q",
    "carry": "one record serves rows switched off and rows frozen: after a freeze the rows out of the run are carried from where the "
             "ping-pong stood at the last settle or change of mask, although the frozen ones are in both buffers",
}


class Flagged(AssertionError):
    def __init__(self, call, step, why):
        AssertionError.__init__(self, "call %d, step %s: %s" % (call, step, why))
        self.call, self.step = call, step


def test_the_headers_need_no_device():
    for name in ("lds_state.h", "lds_flow.h"):
        src = open(os.path.join(CSRC, name)).read()
        assert "#include <hip" not in src and "#include \"common.h\"" not in src and "#include \"host.h\"" not in src, name
    assert "#include \"lds_state.h\"" in open(os.path.join(CSRC, "host.h")).read()
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert " lds_state.h " in mk and " lds_flow.h " in mk


def test_the_flow_is_in_one_place():
    api = open(os.path.join(CSRC, "api.hip")).read()
    for gone in ("static int ensure_expect(", "static int ensure_gains(", "static int ensure_stats(", "static int ensure_resid(", "static int sweep(",
                 "static void adopt_classes(", "static int update_noise(", "static int lds_bound(", "static int iterate_updates(",
                 "static int ensure_lnd_x(", "static int inputs_ready(", "h->st.mixed_cov", "h->st.stats_valid", "sweep all states first"):
        assert gone not in api, gone
    assert "flow(h).iterate_updates()" in api or "f.iterate_updates()" in api


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("lds_flow")
    probe = tmp / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    if subprocess.run(SAN + [str(probe), "-o", str(tmp / "probe")], capture_output=True).returncode != 0:
        pytest.skip("this compiler cannot link the static sanitizer runtimes")
    exe = tmp / "lds_flow_driver"
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


UPDATES = ("sweep", "x", "cols", "B", "parents", "Q", "R", "Y", "elbo", "iterate", "until")


class Model:
    def __init__(self, T, N, D, P, dense, big):
        self.T, self.N, self.D, self.P, self.dense, self.big = T, N, D, P, bool(dense), bool(big)
        self.v = dict.fromkeys(("X", "Y", "A", "B", "C", "Q", "R", "given", "cov", "cls"), 0)
        self.formed = {}                    # derived buffer -> the versions of its sources it was formed from
        self.xgen = [None] * T              # the gains X_t was last updated under
        self.gains_id = None                # the gains as last formed (counts the preps)
        self.preps = 0
        self.has_classes = self.lnd_pending = False
        self.xloc = 0                       # the X buffer that holds the states
        self.park_x, self.park_cls_other = 0, False     # where the rows out of the run are taken to sit
        self.on, self.conv = [1] * N, [0] * N
        self.has_missing = self.inputs_set = self.input_priors_set = False
        self.exact = False
        self.expect_next = []               # steps that must follow at once
        self.lost_x = False                 # a forward sweep did not write its states out
        self.flagged_carry = 0

    # ---- versions
    def now(self, buf):
        return tuple(self.v[s] for s in SOURCES[buf])

    def current(self, buf):
        return self.formed.get(buf) == self.now(buf)

    def form(self, buf):
        self.formed[buf] = self.now(buf)

    def bump(self, *names):
        for n in names:
            self.v[n] += 1

    def running(self):
        return sum(1 for o, c in zip(self.on, self.conv) if o and not c)

    def settled(self):
        return self.running() == self.N or (self.park_x == self.xloc and not self.park_cls_other)

    def fresh(self):
        return sum(1 for g in self.xgen if g is not None and g == self.gains_id)

    def x_updated(self, ts):
        full_before = self.fresh() == self.T
        for t in ts:
            self.xgen[t] = self.gains_id
        self.bump("X")
        if not full_before and self.fresh() == self.T:
            self.expect_next = [["swap_classes"]]

    # ---- one step of a call
    def step(self, s, fail):
        kind = s[0]
        a = [int(x) for x in s[1:] if x.lstrip("-").isdigit()]
        if self.expect_next:
            want = self.expect_next.pop(0)
            if s[:len(want)] != want:
                fail("%s must follow here, not %s" % (" ".join(want), " ".join(s)))
        elif kind in ("swap_classes", "in_gains", "tie", "in_moments", "in_resQ", "in_elbo", "moments", "syy_missing", "syy_full", "missing_ent_dense"):
            fail("%s where nothing asks for it" % " ".join(s))
        if self.lost_x and not (kind in ("swap_classes", "join_elbo") or (kind == "sweep" and a[0] == BWD and a[2] == 1)):
            fail("%s after a forward sweep that did not write its states out" % " ".join(s))

        def need(buf, what=None):
            if not self.current(buf):
                fail("%s reads %s, which is not of the current %s" % (what or kind, buf, ", ".join(SOURCES[buf])))

        def stale(buf):
            if self.current(buf):
                fail("%s forms %s, which is current" % (kind, buf))

        if kind == "wexpect":
            stale("expect"); self.form("expect")
        elif kind == "dense_pre":
            need("expect"); stale("gains")
            self.expect_next = [["prep"]]
        elif kind == "prep":
            stale("gains")
            if self.dense:
                need("expect")
            if self.P and not (self.inputs_set and self.input_priors_set):
                fail("prep on a handle with inputs before it has them")
            self.form("gains")
            self.preps += 1
            self.gains_id = self.preps
            if self.P:
                self.expect_next = [["in_gains"]]
        elif kind == "in_gains":
            pass
        elif kind == "sweep":
            direction, src, read_cache, keep_x = a
            need("gains")
            if src != self.xloc:
                fail("the sweep reads X[%d], the states are in X[%d]" % (src, self.xloc))
            if bool(read_cache) != (direction == BWD and self.current("U")):
                fail("read_cache = %d: U is %s" % (read_cache, "current" if self.current("U") else "not of the forward sweep right before, or gains, outputs or states changed since"))
            self.lost_x = not keep_x
            if not keep_x and direction != FWD:
                fail("a backward sweep that keeps no states")
            self.xloc = 1 - self.xloc
            self.x_updated(range(self.T))
            if direction == FWD:
                self.form("U")
            if read_cache and not self.big:
                self.form("sxx")
        elif kind == "step":
            need("gains")
            self.x_updated([a[0]])
        elif kind == "swap_classes":
            self.bump("cls")
            self.has_classes, self.lnd_pending = True, False
            if self.running() < self.N:
                self.park_cls_other = not self.park_cls_other
        elif kind == "stats":
            stale("stats")
            if not self.has_classes:
                fail("statistics while the X_t have no covariance classes")
            if len(set(self.xgen)) > 1:
                fail("statistics while the X_t belong to different gains")
            if bool(a[0]) != (not self.current("sxx")):
                fail("with_sxx = %d: sxx is %scurrent" % (a[0], "" if self.current("sxx") else "not "))
            if self.big and not a[0]:
                fail("the 128-wide class takes sxx from the sweep")
            self.expect_next = [["moments", str(1 - a[0])], ["tie", "moments"]] + ([["in_moments"]] if self.P else [])
        elif kind == "moments":
            pass
        elif kind == "tie" and s[1] == "moments":
            if not self.P:
                self.form("stats")
        elif kind == "in_moments":
            if not (self.inputs_set and self.input_priors_set):
                fail("in_moments on a handle with inputs before it has them")
            self.form("stats")
        elif kind == "in_HA":
            need("stats"); self.form("HA")
        elif kind == "cols":
            which, c0, c1, fuse = a
            need("stats")
            if self.dense:
                fail("cols with Wishart noise")
            if self.P and which != 1:
                need("HA")
            if which == 2 and self.P:
                fail("A and C share no launch on a handle with inputs")
            self.bump(*{0: "A", 1: "C", 2: "AC"}[which])
            if fuse:
                if (fuse, c0, c1) != (3, 0, self.D) or which == 0:
                    fail("fuse")
                for w in ((1,) if which == 1 else (0, 1)):
                    self.form("resQ" if w == 0 else "resR")
                self.bump(*("R" if which == 1 else "QR"))
        elif kind == "in_colsB":
            need("stats"); self.bump("B")
        elif kind == "cols_dense":
            which, c0, c1 = a
            need("stats"); need("expect")
            self.bump(*{0: "A", 1: "C", 2: "AC"}[which])
            if (c0, c1) == (0, self.D):
                for w in ((0, 1) if which == 2 else (which,)):
                    self.form("sg%d" % w)
        elif kind == "resid":
            res = "resQ" if a[0] == 0 else "resR"
            stale(res); need("stats")
            if self.dense:
                fail("resid with Wishart noise")
            if self.P and a[0] == 0:
                need("HA")
                self.expect_next = [["in_resQ"]]
            else:
                self.form(res)
        elif kind == "in_resQ":
            self.form("resQ")
        elif kind == "wresid":
            which, update, use_sg = a
            need("stats")
            ws = (0, 1) if which == 2 else (which,)
            if bool(use_sg) != all(self.current("sg%d" % w) for w in ws):
                fail("use_sg = %d: SG is %s" % (use_sg, "current" if all(self.current("sg%d" % w) for w in ws) else "not of every column as it is now"))
            for w in ws:
                if not update:
                    stale("resQ" if w == 0 else "resR")
                self.form("resQ" if w == 0 else "resR")
            if update:
                self.bump(*[("Q", "R")[w] for w in ws])
        elif kind == "noise":
            need("resQ" if a[0] == 0 else "resR")
            self.bump("QR"[a[0]])
        elif kind in ("elbo", "elbo_dense"):
            need("stats"); need("resQ"); need("resR")
            if self.dense != (kind == "elbo_dense"):
                fail("the bound of the other noise family")
            if self.dense:
                need("expect")
            if self.exact and self.lnd_pending:
                fail("the exact bound reads lnd_x, which is not formed from the classes the caller gave")
            if self.P:
                self.expect_next = [["in_elbo", s[1]]]
        elif kind == "in_elbo":
            pass
        elif kind == "impute":
            self.expect_next = [["syy_missing"], ["tie", "syy"]]
        elif kind == "impute_dense":
            need("expect")
            self.expect_next = [["syy_full"], ["missing_ent_dense", "0"]]
        elif kind in ("syy_missing", "syy_full", "missing_ent_dense", "tie", "parents", "join_elbo", "converge"):
            pass
        elif kind == "carry":
            if self.running() == self.N:
                fail("a carry with every replicate running")
            if s[1] == "x":
                if a[0] != self.park_x or self.park_x == self.xloc:
                    fail("carry from X[%d]: the rows out of the run are in X[%d], the states in X[%d]" % (a[0], self.park_x, self.xloc))
                if not any(not o for o in self.on):
                    self.flagged_carry += 1         # EXCEPTIONS["carry"]: frozen rows only
                self.park_x = self.xloc
            else:
                if not self.park_cls_other:
                    fail("carry of the classes: they are in the current set")
                self.park_cls_other = False
        elif kind in ("copy", "stage", "mask", "form_lnd_x"):
            if not self.settled():
                fail("%s while rows of replicates out of the run sit on the other side of a ping-pong" % kind)
            if kind == "form_lnd_x":
                if not self.lnd_pending:
                    fail("lnd_x is formed though nobody gave classes")
                self.lnd_pending = False
        else:
            fail("unknown step %r" % (s,))

    # ---- what a call changes beside its steps
    def after(self, cmd, err):
        c, a = cmd[0], [int(x) for x in cmd[1:]]
        if err is not None:
            return
        if c == "priors": self.bump("given")
        elif c == "wishart_priors": self.bump("Q", "R", "given")
        elif c == "wishart_state": self.bump("Q", "R")
        elif c in ("column_cov", "column_obs"): self.bump("given", "cov")
        elif c == "observations":
            self.bump("Y"); self.has_missing = bool(a[0])
        elif c == "output_state": self.bump("Y")
        elif c == "inputs":
            self.bump("Y"); self.inputs_set = True
        elif c == "input_priors":
            self.bump("given"); self.input_priors_set = True
        elif c == "input_state": self.bump("given")
        elif c == "state":
            if a[0]: self.bump("X")
            if a[1]: self.bump("given", "cov")
            elif a[2]: self.bump("given")
        elif c == "classes":
            self.bump("cls"); self.has_classes = self.lnd_pending = True
        elif c == "time_split": self.bump("X")
        elif c == "Y" and self.has_missing and self.running(): self.bump("Y")
        elif c == "until": self.conv = a[1:]
        elif c == "active":
            if a != self.on:
                self.on = a
                self.park_x, self.park_cls_other = self.xloc, False
        elif c == "bound": self.exact = bool(a[0])

    def check_state(self, st, fail):
        cur, gains, expect, stats, resQ, resR, sg0, sg1, u, sxx, fresh, mixed, classes, lnd_pending, x_park, cls_other = st
        got = dict(gains=gains, expect=expect, stats=stats, resQ=resQ, resR=resR, sg0=sg0, sg1=sg1, U=u, sxx=sxx)
        for buf, flag in got.items():
            if bool(flag) != self.current(buf):
                fail("the state says %s is %s, the model %s" % (buf, "current" if flag else "stale", "current" if self.current(buf) else "stale"))
        if cur != self.xloc: fail("cur")
        if fresh != self.fresh(): fail("fresh_count %d, the model %d" % (fresh, self.fresh()))
        if bool(mixed or (gains and 0 < fresh < self.T)) != (len(set(self.xgen)) > 1):
            fail("the X_t belong to %d gains, the state says mixed_cov %d, fresh_count %d" % (len(set(self.xgen)), mixed, fresh))
        if bool(classes) != self.has_classes: fail("classes_valid")
        if bool(lnd_pending) != self.lnd_pending: fail("lnd_x_pending")
        if x_park != self.park_x: fail("x_park %d, the model %d" % (x_park, self.park_x))
        if bool(cls_other) != self.park_cls_other: fail("cls_parked_other")


def replay(calls):
    """Holds a transcript to the model; raises Flagged(call, step).  Returns (steps, the model's EXCEPTIONS["carry"] count)."""
    m, steps, carries = None, 0, 0
    for i, (cmd, trace, err, st) in enumerate(calls):
        if cmd[0] == "init":
            if m is not None:
                carries += m.flagged_carry
            m = Model(*(int(x) for x in cmd[1:7]))
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
                if not (m.P and not (m.inputs_set and m.input_priors_set)): fail("PYVB_E_ARG: " + text)
            else:
                fail("status %d" % code)
        m.after(cmd, err)
        m.check_state(st, fail)
    return steps, carries + (m.flagged_carry if m else 0)


# ---- the classes of handle: name -> (dense, big, P), and the commands that make one ready for its first update
CLASSES = {"gamma": (0, 0, 0), "big": (0, 1, 0), "wishart": (1, 0, 0), "wishart_big": (1, 1, 0), "inputs": (0, 0, 2)}


def _start(name, T, N, D):
    dense, big, P = CLASSES[name]
    cmds = [["init", T, N, D, P, dense, big], ["priors"], ["observations", 0]]
    if dense:
        cmds.append(["wishart_priors"])
    if P:
        cmds += [["inputs"], ["input_priors"], ["input_state"]]
    return cmds + [["state", 1, dense, 1]] + ([["wishart_state"]] if dense else [])


def _random_call(rng, name, T, N, D, st):
    """st: what the generator keeps of the handle: the mask, the converged bytes, missing outputs, the parents"""
    dense, big, P = CLASSES[name]
    k = int(rng.integers(0, 34))
    if k < 4: return ["sweep", k % 2]
    if k < 7: return ["x", int(rng.integers(0, T))]
    if k < 10:
        c0 = int(rng.integers(0, D)); full = rng.random() < 0.5
        return ["cols", int(rng.integers(0, 2)), 0 if full else c0, D if full else int(rng.integers(c0 + 1, D + 1))]
    if k == 10: return ["B"] if P else ["Q"]
    if k == 11: return ["Q"]
    if k == 12: return ["R"]
    if k < 15: return ["elbo"]
    if k < 18: return ["iterate", int(rng.integers(0, 3))]
    if k == 18:
        run = [n for n in range(N) if st["on"][n] and not st["conv"][n]]
        for n in run:
            if rng.random() < 0.4: st["conv"][n] = 1
        return ["until", int(rng.integers(1, 3))] + st["conv"]
    if k == 19:
        on = [n for n in range(N) if st["on"][n]]
        if on and rng.random() < 0.7: st["on"][on[int(rng.integers(0, len(on)))]] = 0
        return ["active"] + st["on"]
    if k == 20: return ["get_state"]
    if k == 21: return ["get_classes"]
    if k == 22: return ["get_logdets"]
    if k == 23: return ["classes"]
    if k == 24: return ["state", int(rng.integers(0, 2)), int(dense and rng.random() < 0.5), int(rng.integers(0, 2))]
    if k == 25: return ["priors"] if not st["parents"] else ["elbo"]
    if k == 26: return [["wishart_state"], ["wishart_priors"], ["column_cov"]][int(rng.integers(0, 3))] if dense else ["time_split"]
    if k == 27: return ["column_obs"] if not P and not (dense and big) else ["input_state"] if P else ["elbo"]
    if k == 28:
        if P or (dense and big): return ["observations", 0]
        st["missing"] = int(rng.integers(0, 2))
        return ["observations", st["missing"]]
    if k == 29: return ["output_state"] if st["missing"] else ["inputs"] if P else ["sweep", FWD]
    if k == 30: return ["Y"]
    if k == 31: return ["bound", int(rng.integers(0, 2))]
    if k == 32 and st["parents"]:
        w = int(rng.integers(0, 2))
        return ["parents", w, st["parents"][w]] if st["parents"][w] else ["elbo"]
    return ["sweep", BWD]


def _sequences(seed, per_class, parents=None):
    rng = np.random.default_rng(seed)
    cmds = []
    for name in CLASSES:
        if parents and name != "gamma":
            continue
        for _ in range(per_class):
            T, N, D = int(rng.integers(2, 6)), int(rng.integers(1, 5)), int(rng.integers(1, 4))
            st = dict(on=[1] * N, conv=[0] * N, missing=0, parents=parents)
            cmds += _start(name, T, N, D)
            for w in (0, 1):
                if parents and parents[w]:
                    cmds.append(["set_parents", w, parents[w]])
            cmds += [_random_call(rng, name, T, N, D, st) for _ in range(int(rng.integers(5, 40)))]
            cmds.append(["get_state"])
    return cmds


def test_random_call_sequences_against_the_model(driver):
    cmds = _sequences(2026, 40) + _sequences(7, 20, (GAMMA, DIAGONAL_GAMMA)) + _sequences(8, 20, (DIAGONAL_GAMMA, 0))
    assert 3000 < len(cmds) < 12000
    calls = driver(cmds)
    steps, carries = replay(calls)
    assert steps > len(cmds)
    seen = {s[0] for _, trace, _, _ in calls for s in trace}
    assert seen >= {"prep", "in_gains", "wexpect", "dense_pre", "sweep", "step", "swap_classes", "stats", "moments", "tie", "in_moments", "in_HA",
                    "in_colsB", "in_resQ", "resid", "wresid", "cols", "cols_dense", "noise", "parents", "impute", "impute_dense", "elbo", "in_elbo",
                    "elbo_dense", "carry", "form_lnd_x", "join_elbo", "converge", "copy", "stage", "mask"}, seen
    errors = [e[1] for _, _, e, _ in calls if e is not None]
    assert any(t.startswith(NO_CLASSES) for t in errors) and any("X_t were updated since the parameters changed" in t for t in errors)
    assert carries > 0          # EXCEPTIONS["carry"] is met, and named


# ---- the step list of one pyvb_lds_iterate, per class of handle, from a handle that has iterated before (D = 3).  The bound goes to
# the side stream (1).  DESIGN.md section 14 has a copy.
SWEEPS = ["prep", "sweep 0 0 0 0", "swap_classes", "join_elbo", "sweep 1 1 1 1"]
SUMS_STEPS = ["stats 0", "moments 1", "tie moments"]
ITERATION = {
    "gamma": SWEEPS + SUMS_STEPS + ["cols 2 0 3 3", "elbo 1"],
    "gamma_parents_A": SWEEPS + SUMS_STEPS + ["cols 2 0 3 3", "parents 1 0 0", "elbo 1"],
    "gamma_parents_A_entry_parents_C": SWEEPS + SUMS_STEPS + ["cols 2 0 3 3", "parents 1 0 0", "parents 2 1 0", "elbo 1"],
    "entry_parents_both": SWEEPS + SUMS_STEPS + ["cols 2 0 3 3", "parents 2 2 0", "elbo 1"],
    "big": SWEEPS + ["stats 1", "moments 0", "tie moments", "cols 2 0 3 3", "elbo 1"],
    "wishart": ["dense_pre"] + SWEEPS + SUMS_STEPS + ["cols_dense 2 0 3", "wresid 2 1 1", "wexpect", "elbo_dense 1"],
    "wishart_big": ["dense_pre"] + SWEEPS + ["stats 1", "moments 0", "tie moments", "cols_dense 2 0 3", "wresid 2 1 1", "wexpect", "elbo_dense 1"],
    "inputs": ["prep", "in_gains"] + SWEEPS[1:] + SUMS_STEPS + ["in_moments", "in_HA", "cols 0 0 3 0", "in_colsB", "cols 1 0 3 3", "in_HA", "resid 0",
                                                                 "in_resQ", "noise 0", "elbo 1", "in_elbo 1"],
}
# the first iteration of a handle: nothing is current.  Wishart: the expectations first
FIRST = {"gamma": ITERATION["gamma"], "wishart": ["wexpect"] + ITERATION["wishart"]}
# the exact bound on classes the caller gave: lnd_x is formed when the iteration's own sweeps did not replace the classes --
# they do unless every X_t was already updated under the current gains, so only a call sequence like this one meets it
EXACT_ON_GIVEN_CLASSES = ["sweep 0 1 0 0", "join_elbo", "sweep 1 0 1 1"] + SUMS_STEPS + ["cols 2 0 3 3", "form_lnd_x", "elbo 1"]


def _parents_of(name):
    return {"gamma_parents_A": (GAMMA, 0), "gamma_parents_A_entry_parents_C": (GAMMA, DIAGONAL_GAMMA), "entry_parents_both": (DIAGONAL_GAMMA, DIAGONAL_GAMMA)}.get(name, (0, 0))


@pytest.mark.parametrize("name", sorted(ITERATION))
def test_the_steps_of_an_iteration(driver, name):
    cls = name if name in CLASSES else "gamma"
    cmds = _start(cls, 5, 2, 3) + [["set_parents", w, k] for w, k in enumerate(_parents_of(name)) if k] + [["iterate", 1], ["iterate", 1], ["iterate", 2]]
    calls = driver(cmds)
    replay(calls)
    text = [[" ".join(s) for s in trace] for _, trace, _, _ in calls]
    assert text[-2] == ITERATION[name]
    assert text[-1] == ITERATION[name] * 2
    if name in FIRST:
        assert text[-3] == FIRST[name]


def test_the_exact_bound_on_classes_the_caller_gave(driver):
    cmds = _start("gamma", 5, 2, 3) + [["bound", 1], ["classes"], ["elbo"], ["classes"], ["iterate", 1], ["sweep", FWD], ["classes"], ["iterate", 1]]
    calls = driver(cmds)
    replay(calls)
    text = [[" ".join(s) for s in trace] for _, trace, _, _ in calls]
    assert text[-6] == ["stats 1", "moments 0", "tie moments", "resid 0", "resid 1", "form_lnd_x", "elbo 0"]      # before the first sweep
    assert text[-4] == ["prep", "sweep 0 0 0 0", "swap_classes", "join_elbo", "sweep 1 1 1 1"] + SUMS_STEPS + ["cols 2 0 3 3", "elbo 1"]       # no form_lnd_x
    assert text[-1] == EXACT_ON_GIVEN_CLASSES


def test_a_handle_with_inputs_before_it_has_them(driver):
    calls = driver([["init", 4, 1, 2, 2, 0, 0], ["priors"], ["observations", 0], ["sweep", FWD], ["inputs"], ["sweep", FWD], ["input_priors"], ["sweep", FWD]])
    replay(calls)
    assert [c[2][0] if c[2] else 0 for c in calls[3:]] == [E_ARG, 0, E_ARG, 0, 0]
    assert "pyvb_lds_set_inputs" in calls[3][2][1] and "pyvb_lds_set_input_priors" in calls[5][2][1]
    assert [" ".join(s) for s in calls[7][1]] == ["prep", "in_gains", "sweep 0 0 0 1", "swap_classes"]


def test_parked_rows_and_idle_handles(driver):
    start = _start("gamma", 4, 3, 2)
    tail = [["iterate", 1], ["active", 1, 1, 0], ["sweep", FWD], ["get_state"], ["sweep", BWD], ["priors"], ["sweep", FWD], ["classes"], ["get_classes"],
            ["active", 0, 0, 0], ["sweep", FWD], ["x", 1], ["cols", 0, 0, 2], ["Q"], ["elbo"], ["iterate", 2], ["until", 0, 0, 0, 0], ["get_state"]]
    calls = driver(start + tail)
    replay(calls)
    text = [[" ".join(s) for s in c[1]] for c in calls[len(start):]]
    assert text[1] == ["mask"]
    assert text[2] == ["prep", "sweep 0 0 0 1", "swap_classes"]
    assert text[3] == ["carry x 0", "carry classes", "copy"]    # the sweep moved the states to X[1] and swapped the classes; the parked row stayed
    assert text[4] == ["sweep 1 1 1 1"]                         # (the getter staged through X[0]; U is a buffer of its own and still the forward sweep's)
    assert text[7] == ["carry classes", "stage"]                # X: back and forth since, the row is where the states are; the classes were swapped once
    assert text[8] == ["copy"]
    assert text[9] == ["mask"]
    for i in range(10, 15):
        assert text[i] == [], (tail[i], text[i])                # nothing runs: the update entries emit nothing
    assert text[15] == ["join_elbo", "join_elbo"] and text[16] == [] and text[17] == ["copy"]


# ---- planted defects: a passing transcript, mutated; the model flags each at its step
def _transcript(driver):
    cmds = (_start("gamma", 4, 3, 2) + [["iterate", 1], ["sweep", FWD], ["active", 1, 1, 0], ["sweep", BWD], ["get_state"], ["priors"], ["sweep", FWD], ["observations", 0], ["sweep", BWD]]
            + _start("wishart", 4, 2, 3) + [["iterate", 1], ["sweep", FWD], ["sweep", BWD], ["cols", 0, 1, 2], ["Q"]])
    calls = driver(cmds)
    replay(calls)
    return calls


def _find(calls, cmd, step):
    for i, c in enumerate(calls):
        if c[0] == [str(x) for x in cmd]:
            for j, s in enumerate(c[1]):
                if s[:len(step)] == step:
                    return i, j
    raise AssertionError("no %s in %s" % (step, cmd))


def _mutated(calls, i, j, new=None):
    out = [[c[0], [list(s) for s in c[1]], c[2], c[3]] for c in calls]
    if new is None:
        del out[i][1][j]
    else:
        out[i][1][j] = new
    return out


@pytest.mark.parametrize("defect", ["drop a prep", "read_cache after an outputs change", "use_sg after a partial column update", "drop a carry", "drop a swap_classes"])
def test_planted_defects_are_flagged_at_their_step(driver, defect):
    calls = _transcript(driver)
    if defect == "drop a prep":
        i = [k for k, c in enumerate(calls) if c[0] == ["sweep", "0"] and c[1] and c[1][0] == ["prep"]][0]
        j, bad = 0, _mutated(calls, i, 0)
    elif defect == "read_cache after an outputs change":
        i = [k for k, c in enumerate(calls) if c[0] == ["sweep", "1"] and calls[k - 1][0][0] == "observations"][0]
        j = [k for k, s in enumerate(calls[i][1]) if s[0] == "sweep"][0]
        assert calls[i][1][j][3] == "0"
        bad = _mutated(calls, i, j, calls[i][1][j][:3] + ["1"] + calls[i][1][j][4:])
    elif defect == "use_sg after a partial column update":
        i, j = _find(calls, ["Q"], ["wresid"])
        assert calls[i - 1][0] == ["cols", "0", "1", "2"] and calls[i][1][j] == ["wresid", "0", "1", "0"]
        bad = _mutated(calls, i, j, ["wresid", "0", "1", "1"])
    elif defect == "drop a carry":
        i, j = _find(calls, ["get_state"], ["carry", "x"])
        bad = _mutated(calls, i, j)
    else:
        i, j = _find(calls, ["iterate", 1], ["swap_classes"])
        bad = _mutated(calls, i, j)
    with pytest.raises(Flagged) as e:
        replay(bad)
    assert (e.value.call, e.value.step) == (i, j), str(e.value)
