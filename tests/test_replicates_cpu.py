"""CPU-only: the host-side record of a handle's replicates (pyvb_amd/csrc/replicates.h) needs no device.
tests/c/replicates_driver.cpp is built here with the address and undefined-behaviour sanitizers (runtimes linked statically, as
tests/test_tape_plan_cpu.py builds its driver) and run on commands written out below; what it answers is compared with tables
and numpy code in this file:

* validation -- the bad model ids of tests/test_tied_cpu.py and the bad lengths of tests/test_lengths_cpu.py with the status, the
  verbatim message and the replicate it names; valid inputs with what they report as ragged / tied;
* queries -- length, model, first_of, mstart, first and the children of Q and R on 200 random valid draws and on the plain handle;
* masks -- random sequences of shrinking masks, adopted convergence bytes and illegal requests (switching a replicate back on,
  splitting a model): the refusal names the right replicate or model and leaves the state alone; after every step the run mask,
  the caller's mask and n_active() are numpy's.
"""
import os
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
SAN = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan"]
OK, E_ARG = 0, 1

RAGGED_TIED = dict(lengths=(19, 60, 2, 33, 3, 17, 41, 25), models=(0, 1, 1, 1, 2, 2, 3, 3), T=60)


def test_the_status_codes_are_the_header_s():
    from pyvb_amd import _capi
    assert (OK, E_ARG) == (_capi.OK, _capi.E_ARG)


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("replicates")
    probe = tmp / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    if subprocess.run(SAN + [str(probe), "-o", str(tmp / "probe")], capture_output=True).returncode != 0:
        pytest.skip("this compiler cannot link the static sanitizer runtimes")
    exe = tmp / "replicates_driver"
    subprocess.run(SAN + ["-Wall", "-I", os.path.join(REPO, "pyvb_amd", "csrc"), os.path.join(HERE, "c", "replicates_driver.cpp"), "-o", str(exe)],
                   check=True, capture_output=True)

    def run(commands):
        """commands: lists of a word and integers.  Returns the output lines."""
        (tmp / "in.txt").write_text("".join(" ".join(str(x) for x in c) + "\n" for c in commands))
        p = subprocess.run([str(exe), str(tmp / "in.txt"), str(tmp / "out.txt")], capture_output=True, text=True)
        assert p.returncode == 0, "the sanitized driver failed:\n" + p.stderr[-4000:]
        return (tmp / "out.txt").read_text().split("\n")[:-1]
    return run


def _ints(s):
    return [int(x) for x in s.split()]


def _verdict(line):
    head, msg = line.split("|", 1)
    rc, flag = _ints(head)
    return rc, bool(flag), msg


def _state(line):
    n, run, on = line.split("|")
    return int(n), np.array(_ints(run), dtype=bool), np.array(_ints(on))


def _init(N, T, lengths, models):
    return ["init", N, T] + ([0] if lengths is None else [N] + list(lengths)) + ([0] if models is None else [N] + list(models))


MODEL_MSG = ("replicate %d has model %d after %d: model ids start at 0, never decrease and rise in steps of 0 or 1 "
             "(a model is a run of consecutive replicates)")
LENGTH_MSG = "replicate %d has length %d: every chain needs 2 <= T_n <= T = %d"
ON_MSG = ("replicate %d is switched off and cannot be switched on again: the mask can only shrink "
          "(the validity tracking of gains and statistics is per handle)")
SPLIT_MSG = ("the mask switches off part of model %d (replicate %d is %s, replicate %d is %s): the chains of a model "
             "share A, C, Q, R and are switched off together")


# ---- validation ---------------------------------------------------------------------------------------------------------------
# (ids, the replicate refused or None, tied)
MODELS = [([1, 1, 2, 2], 0, None), ([0, 1, 0, 1], 2, None), ([0, 0, 2, 2], 2, None), ([0, 1, 2, 4], 3, None), ([0, 0, 0, -1], 3, None),
          (list(RAGGED_TIED["models"]), None, True), ([0], None, False), ([0, 0, 0, 0, 0], None, True), ([0, 1, 2, 3, 4, 5], None, False),
          ([0, 1, 1], None, True), ([0, 0], None, True)]
# (T, lengths, the replicate refused or None, ragged)
LENGTHS = [(10, [10, 1, 5], 1, None), (10, [10, 5, 11], 2, None), (10, [0, 1, 11], 0, None),
           (60, list(RAGGED_TIED["lengths"]), None, True), (7, [7], None, False), (7, [2], None, True), (9, [9, 9, 9, 9], None, False),
           (9, [9, 9, 8], None, True), (2, [2, 2], None, False)]


def test_validation(driver):
    out = driver([["models", len(ids)] + ids for ids, _, _ in MODELS] + [["lengths", len(ln), T] + ln for T, ln, _, _ in LENGTHS])
    assert len(out) == len(MODELS) + len(LENGTHS)
    for (ids, bad, tied), line in zip(MODELS, out):
        rc, flag, msg = _verdict(line)
        if bad is None:
            assert (rc, flag, msg) == (OK, tied, ""), (ids, line)
        else:
            assert rc == E_ARG and msg == MODEL_MSG % (bad, ids[bad], ids[bad - 1] if bad else -1), (ids, line)
    for (T, ln, bad, ragged), line in zip(LENGTHS, out[len(MODELS):]):
        rc, flag, msg = _verdict(line)
        if bad is None:
            assert (rc, flag, msg) == (OK, ragged, ""), (ln, line)
        else:
            assert rc == E_ARG and msg == LENGTH_MSG % (bad, ln[bad], T), (ln, line)


# ---- queries ------------------------------------------------------------------------------------------------------------------
def _draw(rng):
    """A valid (N, T, lengths or None, models or None): every shape of a handle, singletons and one model for all among them."""
    N, T = int(rng.integers(1, 41)), int(rng.integers(2, 30))
    lengths = None if rng.random() < 0.25 else rng.integers(2, T + 1, N)
    kind = rng.random()
    if kind < 0.2:
        models = None
    else:
        p = 0.0 if kind < 0.3 else (1.0 if kind < 0.4 else rng.random())      # p: how often the next replicate opens a model
        models = np.concatenate([[0], np.cumsum(rng.random(N - 1) < p)]).astype(int)
    return N, T, lengths, models


def _expected(N, T, lengths, models):
    """What the record must answer, in numpy.  A handle is ragged / tied exactly when it was GIVEN lengths / models: the caller
    (api.hip) passes null where check_lengths / check_models report `not ragged` / `not tied`."""
    length = np.full(N, T) if lengths is None else np.asarray(lengths)
    model = np.arange(N) if models is None else np.asarray(models)
    M = int(model.max()) + 1
    mstart = np.array([np.nonzero(model == m)[0][0] for m in range(M)] + [N])
    first = np.zeros(N, dtype=int); first[mstart[:-1]] = 1
    nq = np.array([(length[model == model[n]] - 1).sum() for n in range(N)])
    nr = np.array([length[model == model[n]].sum() for n in range(N)])
    return dict(M=M, length=length, model=model, first_of=mstart[model], nq=nq, nr=nr, mstart=mstart, first=first)


def _check_queries(lines, N, T, lengths, models, what):
    e = _expected(N, T, lengths, models)
    assert _ints(lines[0]) == [e["M"], lengths is not None, models is not None], what
    for line, k in zip(lines[1:6], ("length", "model", "first_of", "nq", "nr")):
        assert _ints(line) == list(e[k]), (what, k)
    # the arrays the tied creation uploads exist with the models, and only then
    assert _ints(lines[6]) == (list(e["mstart"]) if models is not None else []), what
    assert _ints(lines[7]) == (list(e["first"]) if models is not None else []), what
    n, run, on = _state(lines[8])
    assert n == N and run.all() and on.tolist() == [1] * N, what


def test_queries_on_random_handles(driver):
    rng = np.random.default_rng(20260)
    draws = [_draw(rng) for _ in range(200)]
    draws.append((8, RAGGED_TIED["T"], RAGGED_TIED["lengths"], RAGGED_TIED["models"]))
    assert sum(d[2] is not None and d[3] is not None and len(set(d[3])) not in (1, d[0]) for d in draws) > 60
    out = driver([_init(*d) for d in draws])
    assert len(out) == 9 * len(draws)
    for i, d in enumerate(draws):
        _check_queries(out[9 * i:9 * i + 9], *d, what="draw %d: %r" % (i, d))


def test_the_plain_handle_answers_T_n_n_T_minus_1_and_T(driver):
    for N, T in ((1, 2), (5, 12)):
        lines = driver([_init(N, T, None, None)])
        assert _ints(lines[0]) == [N, 0, 0]
        assert [_ints(x) for x in lines[1:6]] == [[T] * N, list(range(N)), list(range(N)), [T - 1] * N, [T] * N]
        assert lines[6] == "" and lines[7] == ""


# ---- masks --------------------------------------------------------------------------------------------------------------------
def _mask_sequence(rng, N, models, steps):
    """(commands, expectations): a random walk through legal and illegal requests, the state kept in numpy."""
    model = np.arange(N) if models is None else np.asarray(models)
    M = int(model.max()) + 1
    on, conv = np.ones(N, dtype=bool), np.zeros(N, dtype=bool)
    cmds, want = [], []

    def state():
        return int((on & ~conv).sum()), (on & ~conv).copy(), on.astype(int).copy()

    def as_bytes(mask):             # any non-zero byte is "on"
        return np.where(mask, rng.choice([1, 1, 2, 255], N), 0)

    for _ in range(steps):
        kind = rng.choice(["shrink", "shrink", "conv", "on", "split", "same"])
        if kind in ("shrink", "same"):
            req = on.copy() if kind == "same" else on & ~np.isin(model, rng.choice(M, int(rng.integers(1, 3))))
            differs = bool((req != on).any())
            on = req
            cmds.append(["mask"] + list(as_bytes(req)))
            want.append(((OK, differs, ""), state()))
        elif kind == "conv":        # the test freezes whole models, and only ones that run
            stop = np.isin(model, rng.choice(M, int(rng.integers(1, 3)))) & on
            conv = conv | stop
            cmds.append(["conv"] + list(conv.astype(int)))
            want.append((None, state()))
        elif kind == "on":
            if on.all():
                continue
            req = on | np.isin(model, model[rng.choice(np.nonzero(~on)[0])])
            if rng.random() < 0.5:      # a request that ALSO splits a model: the switching-on is what is reported
                req[rng.integers(N)] ^= True
                if not (req & ~on).any():
                    continue
            bad = int(np.nonzero(req & ~on)[0][0])
            cmds.append(["mask"] + list(as_bytes(req)))
            want.append(((E_ARG, False, ON_MSG % bad), state()))
        else:                       # one chain of a model of several chains that are all switched on
            whole = [m for m in range(M) if (model == m).sum() > 1 and on[model == m].all()]
            if not whole:
                continue
            req = on.copy()
            req[rng.choice(np.nonzero(model == rng.choice(whole))[0])] = False
            n = next(n for n in range(1, N) if model[n] == model[n - 1] and req[n] != req[n - 1])
            words = ("on" if req[n - 1] else "off", "on" if req[n] else "off")
            cmds.append(["mask"] + list(as_bytes(req)))
            want.append(((E_ARG, False, SPLIT_MSG % (model[n], n - 1, words[0], n, words[1])), state()))
    return cmds, want


def test_random_mask_sequences(driver):
    rng = np.random.default_rng(20261)
    refused = {"on": 0, "split": 0}
    for case in range(60):
        N, T, lengths, models = _draw(rng)
        if case == 0:
            N, T, lengths, models = 8, RAGGED_TIED["T"], RAGGED_TIED["lengths"], np.asarray(RAGGED_TIED["models"])
        cmds, want = _mask_sequence(rng, N, models, 25)
        out = driver([_init(N, T, lengths, models)] + cmds)[9:]
        for cmd, (verdict, st) in zip(cmds, want):
            what = "case %d (models %r): %r" % (case, models, cmd)
            if verdict is not None:
                assert _verdict(out.pop(0)) == verdict, what
                refused["on"] += "switched on again" in verdict[2]
                refused["split"] += "part of model" in verdict[2]
            n, run, on = _state(out.pop(0))
            assert n == st[0] and np.array_equal(run, st[1]) and np.array_equal(on, st[2]), what
        assert not out
    assert refused["on"] > 50 and refused["split"] > 50, refused
