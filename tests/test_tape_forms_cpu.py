"""CPU-only: the cases of tests/tape_forms.py before they reach a device.

* Every case goes through the sanitized planner driver (tests/c/tape_plan_driver.cpp, the fixture of tests/test_tape_plan_cpu.py)
  and its plan must have exactly the form the case declares: the library plans with the same header, so this is the form the
  GPU test runs.
* On every case the float64 interpreter (oracle/tape_ref.py) stays within extended_ref.CAP of the extended run (tests/tape_xref.py)
  and passes the comparison the device has to pass (tape_forms.judge).
* That comparison can fail: six defective interpreters, copies of oracle/tape_ref.run with one planted fault each, are flagged in
  exactly the cases the fault touches.
* tape_divmod of k_tape.hip, simulated in float32 with the reciprocal at float(1 / n) and at both its neighbours, recovers the
  row and column of every element below TAPE_MAX_ELEMS, and first fails beyond it at the indices listed here.
"""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import extended_ref as E  # noqa: E402
import tape_cases as TC  # noqa: E402
import tape_forms as F  # noqa: E402
import tape_xref as X  # noqa: E402
from oracle import tape_ref as R  # noqa: E402
from test_tape_plan_cpu import driver  # noqa: E402,F401  (the fixture)


def assert_form(plan, c):
    W, width = plan["windows"], plan["width"].tolist()
    assert plan["valid"].all()
    if c.form in ("plain", "blocks"):
        assert not plan["in_lds"] and (c.program is None) == (c.form == "plain")
        assert c.form == "plain" or max(n for _, n in c.program[0]) < 3
        return
    assert plan["in_lds"] and width == [4 if c.form in ("window-256", "bundled-4") else 8]
    if c.form == "arena-in-cached-512":
        first, count, _, nseg = W[0][:4]
        assert nseg == 0 and np.array_equal(plan["cops"][first], c.records[0]) and np.any(W[:, 3] > 0)
        return
    assert len(W) == c.outputs.nblocks and np.all(W[:, 3] > 0), "a record of the case stays on the arena"
    assert np.all(W[:, 5] == int(c.form.startswith("bundled")))


def plan_of(driver, c):
    blocks, launches = (None, None) if c.program is None else c.program
    return driver(c.arena.size, c.records, blocks, launches)


@pytest.mark.parametrize("name,form", F.opcode_forms())
def test_cases_have_their_form_and_a_reference_under_the_cap(driver, name, form):
    cases = F.cases(name, form)
    assert cases
    for label, c in cases:
        assert c.form == form
        assert_form(plan_of(driver, c), c)
        ref64, _ = F.reference(c, R.run)
        j = F.judge(c, ref64)
        assert j["e64"] <= E.CAP, (label, j)
        assert not j["problems"], (label, j["problems"])
        o = c.outputs           # the NumPy interpreter itself writes nothing outside what the case lists as written
        touched = np.zeros(c.arena.size, dtype=bool); touched[F.everywhere(c, np.concatenate([o.written, o.scratch]))] = True
        assert np.array_equal(F._bits(ref64[~touched]), F._bits(c.arena[~touched])), label
        sent = c.arena == F.sentinels(0, c.arena.size)      # distinct and not zero by construction, no input has such a value
        last = np.minimum(F.everywhere(c, o.written) + 1, c.arena.size - 1)
        assert name == "scatter_acc" or np.all(sent[last] | touched[last]), "%s: a written extent is not followed by a sentinel" % label


def test_window_cases_have_the_plans_they_are_about(driver):
    for label, (c, want) in F.window_cases().items():
        plan = plan_of(driver, c)
        assert_form(plan, c)
        if not plan["in_lds"]:
            assert want == dict(in_lds=False), label
            continue
        W = plan["windows"]
        assert len(W) == 1, label
        first, count, seg0, nseg, doubles, bundled = W[0][:6]
        if "nseg" in want:
            assert nseg == want["nseg"], label
        if "seglen" in want:
            assert plan["segs"][seg0:seg0 + nseg, 1].tolist() == want["seglen"], label
        if "doubles" in want:
            assert doubles == want["doubles"] == TC.TAPE_LDS_CAP, label
        if "min_count" in want:
            assert bundled and count > 512 and np.sum(plan["cops"][first:first + count, 0] != R.T_NOP) == want["min_count"], label
        ref64, _ = F.reference(c, R.run)
        assert not F.judge(c, ref64)["problems"], label
    strided = F.window_cases()["strided copy in a window"][0]
    span = 300 + np.arange(12 * 9 + 5)
    assert np.setdiff1d(span, strided.outputs.written).size == 12 * 4, "the gaps of the written span are not outputs"


def test_not_positive_definite_cases_are_what_they_say():
    for core in F.not_pd_cores():
        m = core.rec[4]
        M = core.state[core.rec[2]:core.rec[2] + m * m].reshape(m, m)
        k = 1 if "first" in core.name else m
        assert np.all(np.linalg.eigvalsh(M[:k - 1, :k - 1]) > 0) if k > 1 else True
        assert np.linalg.eigvalsh(M[:k, :k]).min() < 0, core.name
        with pytest.raises(R.LinAlgStatus):
            F.reference(F.case(core, "plain"), R.run)


# ---- planted faults
def _gemm(A, o, drop_last=False, ignore_neg=False):
    op, d, a, b, m, n, k, fl = o
    X_ = A[a:a + m * k].reshape((k, m)).T if (fl & 1) else A[a:a + m * k].reshape((m, k))
    Y = A[b:b + k * n].reshape((n, k)).T if (fl & 2) else A[b:b + k * n].reshape((k, n))
    Z = X_[:, :k - 1] @ Y[:k - 1] if drop_last else X_ @ Y
    if fl & 8 and not ignore_neg:
        Z = -Z
    cur = A[d:d + m * n].reshape((m, n))
    A[d:d + m * n] = (cur + Z if (fl & 4) else Z).reshape(-1)


def defective(kind):
    """oracle.tape_ref.run with one fault; DEFECTS[kind][1] says which records it touches."""
    def run(A, ops):
        for o in np.asarray(ops, dtype=np.int64).reshape(-1, 8).tolist():
            op, d, a, b, m, n, p, fl = o
            if DEFECTS[kind][1](o) and kind != "padding":
                if kind == "gemm_last_term":
                    _gemm(A, o, drop_last=True)
                elif kind == "neg_with_acc":
                    _gemm(A, o, ignore_neg=True)
                elif kind == "partial_wavefront":
                    terms = A[a:a + m * m:m + 1] if op == R.T_TRACE else A[a:a + m * n] * A[b:b + m * n]
                    v = terms[:terms.size - terms.size % 64].sum()
                    A[d] = A[d] + v if fl & 4 else v
                elif kind == "ld_src_for_ld_dst":
                    R.run(A, [[op, d, a, p, m, n, p, fl]])
                elif kind == "upper_triangle":
                    M = A[a:a + m * m].reshape(m, m).copy()
                    A[a:a + m * m] = (np.triu(M) + np.triu(M, 1).T).reshape(-1)     # what the upper triangle describes
                    try:
                        R.run(A, [o])
                    except (R.LinAlgStatus, np.linalg.LinAlgError):
                        A[d:d + m * m] = np.nan
                    A[a:a + m * m] = M.reshape(-1)
                continue
            R.run(A, [o])
            if kind == "padding" and DEFECTS[kind][1](o):
                for off, k, wr in TC.extents(o):
                    if wr and k % 2 and off + k < A.size:
                        A[off + k] = 0.0
    return run


def _odd_write(o):
    ext = TC.extents(o)
    return ext is not None and any(wr and k % 2 for _, k, wr in ext)


DEFECTS = {         # kind: (forms it is run in, the records it touches)
    "gemm_last_term": (("plain",), lambda o: o[0] == R.T_GEMM and o[6] % 8 == 1),
    "partial_wavefront": (("plain",), lambda o: (o[0] == R.T_TRACE and o[4] % 64) or (o[0] == R.T_DOT and (o[4] * o[5]) % 64)),
    "ld_src_for_ld_dst": (("plain",), lambda o: o[0] == R.T_COPY2D and o[3] != o[6] and o[4] > 1),
    "neg_with_acc": (("plain",), lambda o: o[0] == R.T_GEMM and o[7] & 12 == 12 and o[6] > 0),
    "upper_triangle": (("plain",), lambda o: o[0] == R.T_CHOLINV and o[4] > 1),
    "padding": (("plain", "window-512"), _odd_write),
}


@pytest.mark.parametrize("kind", sorted(DEFECTS))
def test_a_planted_fault_is_flagged_in_exactly_the_cases_it_touches(kind):
    forms, touches = DEFECTS[kind]
    flagged = wanted = 0
    for name, cs in sorted(F.cores().items()):
        for core in cs:
            for form in forms:
                if form not in F.forms_of(core):
                    continue
                c = F.case(core, form)
                touched = any(touches(o) for o in c.records.tolist())
                if kind == "upper_triangle":        # a symmetric matrix has the same two triangles: the fault shows where they differ
                    touched = touched and "NaN" in core.name
                got, _ = F.reference(c, defective(kind))
                bad = bool(F.judge(c, got)["problems"])
                assert bad == touched, "%s, %s, %s: flagged %s, touched %s" % (kind, core.name, form, bad, touched)
                flagged += bad; wanted += touched
    assert flagged == wanted and flagged >= 3, "the fault %s touches too few cases to mean anything (%d)" % (kind, flagged)


# ---- the element limit
DIVMOD_N = list(range(1, 17)) + [31, 32, 33, 63, 64, 65, 127, 128, 129, 1023, 1024, 2047, 2048]
FIRST_FAILURES = {1: 16777217, 2: 12582911, 3: 18874367, 5: 33554454, 7: 33554478}
EARLIEST = {1: 8388609}


def divmod_wrong(idx, n, rn, x=None):
    """tape_divmod (k_tape.hip) in float32 on the int32 array idx: True where the fix-up does not recover (idx div n, idx mod n).
    j = idx - i n is exact in integers, so one step of fix-up ends with 0 <= j < n -- and then i is the quotient -- exactly when
    -n <= j < 2 n."""
    x = idx.astype(np.float32) + np.float32(0.5) if x is None else x
    j = idx - (x * rn).astype(np.int32) * np.int32(n)
    return (j < -n) | (j >= 2 * n)


def reciprocals(n):
    r = np.float32(1.0) / np.float32(n)
    return [np.nextafter(r, np.float32(0)), r, np.nextafter(r, np.float32(2))]


def test_the_float_division_is_exact_below_the_element_limit_and_not_beyond():
    assert TC.TAPE_MAX_ELEMS == 1 << 22
    with open(os.path.join(os.path.dirname(HERE), "pyvb_amd", "csrc", "tape.h")) as f:
        assert "#define TAPE_MAX_ELEMS (1 << 22)" in f.read()
    idx = np.arange(TC.TAPE_MAX_ELEMS, dtype=np.int32)
    x = idx.astype(np.float32) + np.float32(0.5)
    for n in DIVMOD_N:
        for rn in reciprocals(n):
            assert not divmod_wrong(idx, n, rn, x).any(), "n = %d, rn = %r" % (n, rn)
    step = 1 << 22
    for n, first in sorted(FIRST_FAILURES.items()):
        firsts = []                 # per reciprocal: the first failure up to the listed one
        for rn in reciprocals(n):
            firsts.append(None)
            for lo in range(TC.TAPE_MAX_ELEMS, first + 1, step):
                bad = divmod_wrong(np.arange(lo, min(lo + step, first + 1), dtype=np.int32), n, rn)
                if bad.any():
                    firsts[-1] = lo + int(np.argmax(bad))
                    break
        assert first in firsts, "n = %d: first failures %r, %d not among them" % (n, firsts, first)
        # the listed index is the earliest of the three, except for n = 1: there it is the first failure with the lower neighbour
        # 1 - 2^-24 of the reciprocal; the upper neighbour 1 + 2^-23 (twice as far) already fails at 2^23 + 1.  Both lie beyond the limit.
        assert min(f for f in firsts if f is not None) == EARLIEST.get(n, first), (n, firsts)


def test_records_at_the_element_limit(driver):
    out = driver(TC.VALIDATION_BOUND_ARENA, [rec for rec, _ in TC.VALIDATION_BOUND], plan=False)
    wrong = [(rec, ok) for (rec, ok), got in zip(TC.VALIDATION_BOUND, out["valid"]) if bool(got) != ok]
    assert not wrong, "verdicts that differ from the list (record, expected): %r" % wrong
    # every refusal of the list is the limit's: the same records are accepted once they are small enough ...
    assert [ok for _, ok in TC.VALIDATION_BOUND].count(False) == 7
    # ... and the limit does not depend on the arena
    big = driver((1 << 31) - 1, [rec for rec, _ in TC.VALIDATION_BOUND], plan=False)
    assert big["valid"].tolist() == out["valid"].tolist()
