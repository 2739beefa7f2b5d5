"""CPU-only: the host-side state of a VB-PCA handle and the planner of its passes over the rows (pyvb_amd/csrc/pca_plan.h) need no
device.  tests/c/pca_plan_driver.cpp strings the state events and the planner together as api_pca.hip does and is built here
with the address and undefined-behaviour sanitizers (runtimes linked statically, as tests/test_replicates_cpu.py builds its
driver); it runs sequences of calls and writes out every step a call takes.  This file keeps a model beside it -- per row
"imputed entries unstored", "rows of Z pending", "z_0 stored by the X_0 step" -- and holds every step to it:

* a step that reads row r outside a sweep never meets unstored entries of r (a store comes first);
* a plan is lazy exactly when the sweep may be (kind, latent tiles, no rows waiting for their first update, the standard range,
  a Z update riding along) and the rows that hold unstored entries lie inside the new range;
* a plan stores first exactly when unstored rows exist and it is not lazy; a pass that is not lazy never meets unstored rows;
* the Z update rides along exactly when one is pending, and nothing reads Z or a statistic of Z while it is pending;
* part_chunks is the partition of the kernel the plan names;
* the state after every call is the model's; after a read nothing is unstored and nothing is pending.
"""
import os
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
SAN = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan"]
STORE, COLUMNS, PAIRS = 0, 1, 2
NCHUNK, NCHUNKB = 7, 3


def test_the_sweep_kinds_are_the_header_s():
    from pyvb_amd import _capi
    assert (STORE, COLUMNS, PAIRS) == (_capi.PCA_SWEEPS["store"], _capi.PCA_SWEEPS["columns"], _capi.PCA_SWEEPS["pairs"])


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("pca_plan")
    probe = tmp / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    if subprocess.run(SAN + [str(probe), "-o", str(tmp / "probe")], capture_output=True).returncode != 0:
        pytest.skip("this compiler cannot link the static sanitizer runtimes")
    exe = tmp / "pca_plan_driver"
    subprocess.run(SAN + ["-Wall", "-I", os.path.join(REPO, "pyvb_amd", "csrc"), os.path.join(HERE, "c", "pca_plan_driver.cpp"), "-o", str(exe)],
                   check=True, capture_output=True)

    def run(commands):
        """commands: lists of a word and integers.  Returns, per command, (the command, its steps, the state after it)."""
        (tmp / "in.txt").write_text("".join(" ".join(str(x) for x in c) + "\n" for c in commands))
        p = subprocess.run([str(exe), str(tmp / "in.txt"), str(tmp / "out.txt")], capture_output=True, text=True)
        assert p.returncode == 0, "the sanitized driver failed:\n" + p.stderr[-4000:]
        calls = []
        for line in (tmp / "out.txt").read_text().split("\n")[:-1]:
            if line.startswith("> "):
                calls.append([line[2:].split(), [], None])
            elif line.startswith("= "):
                calls[-1][2] = [int(x) for x in line[2:].split()]
            else:
                calls[-1][1].append(line.split())
        assert len(calls) == len(commands) and all(c[2] is not None for c in calls)
        return calls
    return run


class Model:
    def __init__(self, N, QT, sweep, xdata, row_offset, comm):
        self.N, self.QT, self.sweep, self.xdata, self.row_offset, self.comm = N, QT, sweep, bool(xdata), row_offset, bool(comm)
        self.unstored = np.zeros(N, dtype=bool)
        self.z_pending = self.z0_stored = False
        self.part_chunks = 0

    def lazy_range(self):
        r = np.flatnonzero(self.unstored)
        return (int(r[0]), int(r[-1]) + 1) if r.size else None

    def step(self, s, where):
        kind = s[0]
        if kind == "store":
            lo, hi = int(s[1]), int(s[2])
            assert self.unstored.any(), where + ": a store with nothing unstored"
            self.unstored[lo:hi] = False
            assert not self.unstored.any(), where + ": the store leaves unstored rows behind"
        elif kind == "pass1":
            assert self.z_pending, where + ": pass 1 with no Z update pending"
            assert not self.unstored.any(), where + ": pass 1 reads X while rows hold unstored entries"
            assert bool(int(s[1])) == self.z0_stored, where + ": keep_z0"
            self.z_pending = self.z0_stored = False
        elif kind == "sweep":
            lo, hi, with_z, keep_z0, lazy, pairs, materialize, vin_lo, vin_hi, part_chunks = (int(x) for x in s[1:])
            assert bool(with_z) == self.z_pending, where + ": the Z update rides along exactly when one is pending"
            assert bool(keep_z0) == (self.z_pending and self.z0_stored), where + ": keep_z0"
            incoming = self.lazy_range()
            inside = incoming is None or (lo <= incoming[0] and incoming[1] <= hi)
            may = bool(with_z) and self.sweep != STORE and self.QT == 1 and not self.xdata and lo <= 1 and hi == self.N and hi > lo
            assert bool(lazy) == (may and inside), where + ": lazy"
            assert bool(pairs) == (bool(lazy) and self.sweep == PAIRS), where + ": pairs"
            assert part_chunks == (NCHUNKB if pairs else NCHUNK), where + ": part_chunks"
            assert bool(materialize) == (incoming is not None and not lazy), where + ": materialize"
            assert (vin_lo, vin_hi) == (incoming if incoming is not None else (0, 0)), where + ": the incoming lazy range"
            if materialize:
                self.unstored[vin_lo:vin_hi] = False
            if lazy:
                self.unstored[:] = False        # (inside: the pass takes the unstored entries in and recomputes them)
                self.unstored[lo:hi] = True
            assert lazy or not self.unstored.any(), where + ": a pass that stores meets unstored rows"
            if with_z:
                self.z_pending = self.z0_stored = False
            self.part_chunks = part_chunks
        elif kind == "small":
            name = s[1]
            if name in ("PREPZ", "RUN_HEAD"):
                self.z_pending, self.z0_stored = True, False
            if name in ("X0", "RUN_MID") and self.row_offset == 0:
                assert not self.unstored[0], where + ": the X_0 step reads row 0 while its entries are unstored"
                if self.z_pending:
                    self.z0_stored = True
            if name in ("W", "BETA", "ELBO", "RUN_TAIL"):
                assert not self.z_pending, where + ": %s reads sums over Z while its rows are pending" % name
        elif kind == "copy":
            assert not self.unstored.any() and not self.z_pending, where + ": rows copied while entries are unstored or Z is pending"
        else:
            raise AssertionError("unknown step %r" % (s,))

    def check_state(self, st, where):
        full, lin, res, z_pending, z0_done, xlazy, vlo, vhi, part_chunks = st
        r = self.lazy_range()
        assert bool(xlazy) == (r is not None), where + ": xlazy"
        if r is not None:
            assert (vlo, vhi) == r, where + ": the lazy range"
        assert bool(z_pending) == self.z_pending and bool(z0_done) == (self.z_pending and self.z0_stored), where + ": the pending Z update"
        assert part_chunks == self.part_chunks, where
        assert not full or lin, where + ": full_valid implies lin_valid"
        assert not (full and z_pending), where + ": every sum cannot be current while the rows of Z are pending"


def _replay(calls):
    m, steps = None, 0
    for i, (cmd, trace, st) in enumerate(calls):
        where = "call %d (%s)" % (i, " ".join(cmd))
        if cmd[0] == "init":
            m = Model(*(int(x) for x in cmd[1:7]))
        elif cmd[0] == "sweep":
            m.sweep = int(cmd[1])
        for s in trace:
            m.step(s, where)
            steps += 1
        m.check_state(st, where)
        if cmd[0] in ("read", "set", "variances"):
            assert not m.unstored.any() and not m.z_pending, where
        if cmd[0] == "set":
            assert st[:3] == [0, 0, 0], where
        if cmd[0] in ("Beta", "iterate") and (cmd[0] == "Beta" or int(cmd[1]) > 0):
            assert st[:3] == [1, 1, 1], where + ": after Beta every sum and the residual are current"
    return steps


def _configs():
    return [(N, QT, sweep, xdata, ro, comm) for N in (1, 2, 9) for QT in (1, 2) for sweep in (STORE, COLUMNS, PAIRS) for xdata in (0, 1)
            for (ro, comm) in ((0, 0), (0, 1), (5, 1), (5, 0))]


def _init(cfg):
    return ["init"] + list(cfg) + [NCHUNK, NCHUNKB]


def _random_call(rng, N):
    k = int(rng.integers(0, 14))
    if k < 3:
        lo = int(rng.integers(0, N + 1)); hi = int(rng.integers(lo, N + 1))
        return [["X", lo, hi], ["X", 0, N], ["X", min(1, N), N]][k] if k else ["X", lo, hi]
    return [["W"], ["Z"], ["X0"], ["Mu"], ["Beta"], ["elbo"], ["iterate", int(rng.integers(0, 3))], ["read"], ["set"], ["variances"],
            ["sweep", int(rng.integers(0, 3))]][k - 3]


def test_random_call_sequences_against_the_model(driver):
    rng = np.random.default_rng(2026)
    cmds, nseq = [], 0
    for cfg in _configs():
        for _ in range(24):
            cmds.append(_init(cfg))
            cmds += [_random_call(rng, cfg[0]) for _ in range(int(rng.integers(3, 25)))]
            cmds.append(["read"])
            nseq += 1
    assert nseq > 3000
    steps = _replay(driver(cmds))
    assert steps > 10 * nseq


ADVISED = {"a": [["Z"], ["X", 0, "N"], ["iterate", 1]],                              # row 0 left lazy before the X_0 step of iterate
           "b": [["iterate", 2], ["Z"], ["X", 3, 7], ["iterate", 1]],                # a partial range while rows are lazy
           "c": [["iterate", 1], ["Z"], ["X", 0, "N"], ["X0"], ["Mu"], ["iterate", 1]]}     # the X_0 step after a lazy range that starts at row 0


@pytest.mark.parametrize("case", sorted(ADVISED))
def test_the_advised_sequences(driver, case):
    cmds = []
    for cfg in _configs():
        cmds.append(_init(cfg))
        cmds += [[cfg[0] if x == "N" else (min(x, cfg[0]) if isinstance(x, int) and c[0] == "X" else x) for x in c] for c in ADVISED[case]]
        cmds.append(["read"])
    calls = driver(cmds)
    _replay(calls)
    # on the handle the advice was about -- lazy sweeps allowed, global row 0 held, no communicator -- the store is really there
    cfg = (9, 1, COLUMNS, 0, 0, 0)
    calls = driver([_init(cfg)] + [[9 if x == "N" else x for x in c] for c in ADVISED[case]] + [["read"]])
    _replay(calls)
    kinds = [[s[0] + (" " + s[1] if s[0] == "small" else "") for s in trace] for _, trace, _ in calls]
    if case == "a":
        assert calls[2][1][0][:3] == ["sweep", "0", "9"] and calls[2][1][0][5] == "1"               # X(0, N): lazy, from row 0
        assert kinds[3].index("store") < kinds[3].index("small RUN_MID")
    if case == "b":
        sweep = calls[3][1][0]
        assert sweep[:3] == ["sweep", "3", "7"] and sweep[5] == "0" and sweep[7:10] == ["1", "1", "9"]     # not lazy; stores rows [1, 9) first
    if case == "c":
        assert kinds[4] == ["store", "small X0"]
        assert [s for s in calls[6][1] if s[0] == "sweep"][-1][5] == "1"                           # and the iteration's sweep is lazy again
