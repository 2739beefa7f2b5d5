"""CPU-only: the record of the columns' precision parents (pyvb_amd/csrc/column_parents.h) needs no device.
tests/c/column_parents_driver.cpp is built here with the address and undefined-behaviour sanitizers (runtimes linked statically, as
tests/test_geometry_cpu.py builds its driver) and run on commands written out below:

* the kind in force after every sequence of up to four of {clear, set Gamma, set DiagonalGamma, a failed set of either} on either
  matrix of a pair, against a model of three lines in this file;
* every refusal, verbatim;
* the finite-and-positive check at the first and the last index of a0, b0 and qb, with rows != D;
* the staging of what a setter uploads against oracle/_xspecial.py in long double;
* the broadcast of a model's qb to its chains, and the layout of a block.

The bar of the staging.  psi(qa), ln qa, the two ln Gamma and cst are float64 values of pyvb_amd/csrc/digamma.h's series and of
libm, compared with the long-double oracle in units of max(1, |f|).  tests/test_extended_ref_cpu.py::
test_special_functions_against_mpmath holds that ORACLE to 1e-17 of mpmath in these units; half a unit in the last place of a float64
is 1.1e-16, so no float64 value can be asked to meet 1e-17.  What digamma_pos's series itself is held to is the rule of
tests/test_envelope_gpu.py::test_device_special_functions, with the constants of tests/extended_ref.py: within FACTOR = 16 times
max(scipy's largest distance on the same points, 2^-52).  That rule is the bar here; the figures are printed beside 1e-17.
"""
import itertools
import os
import subprocess

import numpy as np
import pytest
import scipy.special as sp

import extended_ref as E
from oracle import _xspecial as XS
from pyvb_amd import _capi

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
SAN = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan"]
OK, E_ARG, E_HIP = 0, 1, 2
CONSTANT, GAMMA, DIAGONAL_GAMMA = 0, 1, 2
AR = dict(A0=0, B0=1, QA=2, QB=3, LGAMMA_A0=4, LGAMMA_QA=5, DIGAMMA_QA=6, LN_QA=7, LN_REF=8, LN_EXACT=9, COUNT=10)
EN = dict(A0=0, B0=1, QA=2, QB=3, CST=4, COUNT=5, ES_OWN=0, ES_EXACT=1, SCALARS=8)
A0 = [1e-3, 0.5, 1.0, 7.25, 1e3]
B0 = [0.7, 2.5, 1.0, 1e-3, 30.0]
QB = [0.3, 1.0, 11.0, 2e-4, 5e2]


def test_the_constants_are_the_header_s():
    assert (OK, E_ARG, E_HIP) == (_capi.OK, _capi.E_ARG, _capi.E_HIP)
    assert (CONSTANT, GAMMA, DIAGONAL_GAMMA) == (_capi.PARENTS_CONSTANT, _capi.PARENTS_GAMMA, _capi.PARENTS_DIAGONAL_GAMMA)
    assert _capi.PARENTS == ("constant", "gamma", "diagonal_gamma")
    header = open(os.path.join(REPO, "include", "pyvb_hip.h")).read()
    for name, v in (("CONSTANT", 0), ("GAMMA", 1), ("DIAGONAL_GAMMA", 2)):
        assert "#define PYVB_PARENTS_%s %d\n" % (name, v) in header
    src = open(os.path.join(REPO, "pyvb_amd", "csrc", "column_parents.h")).read()
    assert "#include <hip" not in src and "#include \"common.h\"" not in src and "#include \"host.h\"" not in src


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("column_parents")
    probe = tmp / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    if subprocess.run(SAN + [str(probe), "-o", str(tmp / "probe")], capture_output=True).returncode != 0:
        pytest.skip("this compiler cannot link the static sanitizer runtimes")
    exe = tmp / "column_parents_driver"
    subprocess.run(SAN + ["-Wall", "-I", os.path.join(REPO, "pyvb_amd", "csrc"), os.path.join(HERE, "c", "column_parents_driver.cpp"), "-o", str(exe)],
                   check=True, capture_output=True)

    def run(commands):
        """commands: lists of words, ints and floats (floats travel as hexadecimal).  Returns the output lines."""
        word = lambda x: float(x).hex() if isinstance(x, (float, np.floating)) else str(x)
        (tmp / "in.txt").write_text("".join(" ".join(word(x) for x in c) + "\n" for c in commands))
        p = subprocess.run([str(exe), str(tmp / "in.txt"), str(tmp / "out.txt")], capture_output=True, text=True)
        assert p.returncode == 0, "the sanitized driver failed:\n" + p.stderr[-4000:]
        lines = (tmp / "out.txt").read_text().split("\n")[:-1]
        assert len(lines) == len(commands)
        return lines
    return run


def _floats(s):
    return np.array([float.fromhex(x) for x in s.split()])


# ---- the kind in force --------------------------------------------------------------------------------------------------------
def test_the_kind_after_every_sequence_of_up_to_four_transitions(driver):
    """A setter whose launch fails leaves the previous kind in force and hands the failure on; the two matrices are independent."""
    ops = [o + w for o in "cgdGD" for w in "01"]
    seqs = [s for n in range(1, 5) for s in itertools.product(ops, repeat=n)]
    assert len(seqs) == 10 + 100 + 1000 + 10000
    which = lambda k, kind: {(False, False): -1, (True, False): 0, (False, True): 1, (True, True): 2}[(k[0] == kind, k[1] == kind)]
    for s, line in zip(seqs, driver([["seq"] + list(s) for s in seqs])):
        k, want = [CONSTANT, CONSTANT], []
        for op in s:
            w = int(op[1])
            k[w] = {"c": CONSTANT, "g": GAMMA, "d": DIAGONAL_GAMMA}.get(op[0], k[w])
            want.append("%d %d %d %d %d" % (k[0], k[1], which(k, GAMMA), which(k, DIAGONAL_GAMMA), E_HIP if op[0] in "GD" else OK))
        assert line == "|".join(want), s


# ---- the refusals -------------------------------------------------------------------------------------------------------------
def test_every_refusal_verbatim(driver):
    lds_dg = "the columns of %s have DiagonalGamma precision parents, one per entry: pyvb_lds_get_entry_precisions / pyvb_lds_update_entry_precisions serve them"
    lds_const = "the columns of %s have Constant precision parents: no hyperpriors were given (pyvb_lds_set_column_precisions)"
    lds_none = "the columns of %s have no DiagonalGamma precision parents: no per-entry hyperpriors were given (pyvb_lds_set_entry_precisions)"
    pca_const = "the columns of W have Constant precision parents: no hyperpriors were given (pyvb_pca_set_column_precisions)"
    pca_none = "the columns of W have no DiagonalGamma precision parents (pyvb_pca_set_entry_precisions)"
    want = {}
    for of in "AC":
        want.update({(CONSTANT, GAMMA, 0, of): lds_const % of, (DIAGONAL_GAMMA, GAMMA, 0, of): lds_dg % of, (GAMMA, GAMMA, 0, of): None,
                     (CONSTANT, DIAGONAL_GAMMA, 0, of): lds_none % of, (GAMMA, DIAGONAL_GAMMA, 0, of): lds_none % of,
                     (DIAGONAL_GAMMA, DIAGONAL_GAMMA, 0, of): None})
    # (a pyvb_pca whose columns have DiagonalGamma parents answers the Gamma entries with the text of Constant ones, as it always did)
    want.update({(CONSTANT, GAMMA, 1, "W"): pca_const, (DIAGONAL_GAMMA, GAMMA, 1, "W"): pca_const, (GAMMA, GAMMA, 1, "W"): None,
                 (CONSTANT, DIAGONAL_GAMMA, 1, "W"): pca_none, (GAMMA, DIAGONAL_GAMMA, 1, "W"): pca_none, (DIAGONAL_GAMMA, DIAGONAL_GAMMA, 1, "W"): None})
    assert len(want) == 18
    for key, line in zip(want, driver([["require"] + list(k) for k in want])):
        assert line == ("%d|" % OK if want[key] is None else "%d|%s" % (E_ARG, want[key])), key


# ---- the check ----------------------------------------------------------------------------------------------------------------
BAD = [("nan", "nan"), ("inf", "inf"), ("-inf", "-inf"), (0.0, "0"), (-1.5, "-1.5")]


def test_finite_and_positive_at_the_first_and_the_last_index(driver):
    """D = q = 3 columns of rows = d = 5 entries: the last entry is column 2, row 4."""
    D, rows = 3, 5
    shapes = [  # (rows per column, extent, pca, of, place of the first index, place of the last index)
        (0, D, 0, "A", "column 0", "column 2"), (rows, D * rows, 0, "C", "column 0, row 0", "column 2, row 4"),
        (0, D, 1, "W", "column 0", "column 2"), (rows, D * rows, 1, "W", "entry 0 of column 0", "entry 4 of column 2")]
    cmds, want = [], []
    for r, n, pca, of, first, last in shapes:
        for what in ("a0", "b0", "qb"):
            for rep in ([-1] if what != "qb" or pca else [0, 6]):
                prefix = "replicate %d, " % rep if rep >= 0 else ""
                for at, place in ((0, first), (n - 1, last)):
                    for v, shown in BAD:
                        vals = [1.0 + i for i in range(n)]
                        vals[at] = v
                        cmds.append(["check", what, r, pca, rep, of, n] + vals)
                        want.append("%d|%s of %s%s of %s is %s: it must be finite and positive" % (E_ARG, what, prefix, place, of, shown))
                    vals = [1.0 + i for i in range(n)]
                    vals[at] = 5e-324                   # the smallest denormal is positive and finite
                    cmds.append(["check", what, r, pca, rep, of, n] + vals)
                    want.append("%d|" % OK)
    assert len(cmds) == (4 + 4 + 3 + 3) * 2 * 6         # (qb of an LDS matrix: with two replicate numbers)
    assert driver(cmds) == want
    # the first bad value is the one that is named
    assert driver([["check", "b0", rows, 0, -1, "C", 15] + [1.0] * 7 + [-2.0, "nan"] + [1.0] * 6]) == \
        ["%d|b0 of column 1, row 2 of C is -2: it must be finite and positive" % E_ARG]


# ---- the broadcast ------------------------------------------------------------------------------------------------------------
def test_qb_of_a_model_s_first_replicate_goes_to_all_its_rows(driver):
    models, per = [0, 0, 1, 0], 2
    qb = np.arange(1.0, 9.0).reshape(4, per)
    out = driver([["bcast", 4, per, 0] + models + list(qb.ravel())])[0].split("|")
    assert out[:2] == ["%d" % OK, ""]
    assert np.array_equal(_floats(out[2]).reshape(4, per), qb[[0, 0, 2, 0]])
    # a bad value in a row that is not a model's first is never read; in a first row it is named with its replicate
    cmds, want = [], []
    for n, col in itertools.product(range(4), range(per)):
        bad = qb.copy()
        bad[n, col] = np.nan
        cmds.append(["bcast", 4, per, 0] + models + ["nan" if v != v else float(v) for v in bad.ravel()])
        want.append("%d|qb of replicate %d, column %d of A is nan: it must be finite and positive|" % (E_ARG, n, col) if n in (0, 2) else None)
    for line, w in zip(driver(cmds), want):
        assert (line == w) if w else line.startswith("%d||" % OK), (line, w)
    # per-entry parents: D = 2 columns of 3 rows
    bad = np.ones((4, 6)); bad[2, 5] = 0.0
    assert driver([["bcast", 4, 6, 3] + models + list(bad.ravel())]) == \
        ["%d|qb of replicate 2, column 1, row 2 of A is 0: it must be finite and positive|" % E_ARG]


def test_the_layout_of_a_block_is_the_one_the_kernels_were_given(driver):
    """a0 | b0 | qa [D], ex | ld_ref | ld_exact | qb [N][D] with Gamma parents; a0 | b0 | qa | ln qa | psi | cst [D][rows],
    ex | qb [N][D][rows], ld_ref | ld_exact | own [N][D] with DiagonalGamma parents."""
    for N, D, rows in ((1, 1, 1), (3, 3, 5), (7, 64, 64), (1024, 6, 4)):
        per = D * rows
        g, dg = ([int(x) for x in l.split()] for l in driver([["block", GAMMA, N, D, D], ["block", DIAGONAL_GAMMA, N, D, per]]))
        assert g == [3 * D, 3 * D, 3 * D + 3 * N * D, 3 * D + N * D, 3 * D + 2 * N * D, 0, 3 * D + 4 * N * D]
        assert dg == [6 * per, 6 * per, 6 * per + N * per, 6 * per + 2 * N * per, 6 * per + 2 * N * per + N * D,
                      6 * per + 2 * N * per + 2 * N * D, 6 * per + 2 * N * per + 3 * N * D]


# ---- the staging --------------------------------------------------------------------------------------------------------------
def _held(name, got, ref, f64):
    """got, f64: float64; ref: long double.  Units of max(1, |f|); the bar is FACTOR max(scipy's largest distance, 2^-52)."""
    unit = np.maximum(1.0, np.abs(ref))
    e = (np.abs(np.asarray(got).astype(E.LD) - ref) / unit).astype(float)
    e64 = (np.abs(np.asarray(f64).astype(E.LD) - ref) / unit).astype(float)
    y = max(float(e64.max()), E.U64)
    print("%-12s %d points: largest distance %.2e (scipy float64 %.2e), e / y %.2f, e / 1e-17 %.1f" % (name, e.size, e.max(), e64.max(), e.max() / y, e.max() / 1e-17))
    assert np.all(e <= E.FACTOR * y), (name, e.max(), y)


def _cst(a0, b0, dg, lg):
    qa = a0 + 0.5
    return (a0 - qa) * dg(qa) - lg(a0) + a0 * np.log(b0) + lg(qa) + qa


def test_gamma_staging_against_the_extended_oracle(driver):
    E.require_extended()
    a0, b0, qb = np.array(A0), np.array(B0), np.array(QB)
    n = a0.size
    for rows in (1, 5, 64):
        head, full = (_floats(l) for l in driver([["gamma", n, rows, 0] + A0 + B0, ["gamma", n, rows, 1] + A0 + B0 + QB]))
        qa = a0 + 0.5 * rows
        assert head.size == 3 * n and full.size == AR["COUNT"] * n
        r = full.reshape(AR["COUNT"], n)
        assert np.array_equal(head.reshape(3, n), [a0, b0, qa]) and np.array_equal(r[:4], [a0, b0, qa, qb])      # bit for bit
        assert np.all(r[AR["LN_REF"]:] == 0.0)                  # follow qb on the device
        ql = qa.astype(E.LD)
        _held("rows %d lgamma a0" % rows, r[AR["LGAMMA_A0"]], XS.gammaln(a0.astype(E.LD)), sp.gammaln(a0))
        _held("rows %d lgamma qa" % rows, r[AR["LGAMMA_QA"]], XS.gammaln(ql), sp.gammaln(qa))
        _held("rows %d psi(qa)" % rows, r[AR["DIGAMMA_QA"]], XS.digamma(ql), sp.digamma(qa))
        _held("rows %d ln qa" % rows, r[AR["LN_QA"]], np.log(ql), np.log(qa))


def test_diagonal_gamma_staging_against_the_extended_oracle(driver):
    """Every a0 with every b0, one entry each; the PCA form sums ES_EXACT over the entries in ascending order."""
    E.require_extended()
    a0, b0 = (np.array(v) for v in zip(*itertools.product(A0, B0)))
    qb = np.resize(np.array(QB), a0.size) * np.linspace(1.0, 2.0, a0.size)
    n = a0.size
    head, full = (_floats(l) for l in driver([["dgamma", n, 0] + list(a0) + list(b0), ["dgamma", n, 1] + list(a0) + list(b0) + list(qb)]))
    qa = a0 + 0.5
    assert head.size == 6 * n and full.size == EN["COUNT"] * n + EN["SCALARS"]
    h, r, scal = head.reshape(6, n), full[:EN["COUNT"] * n].reshape(EN["COUNT"], n), full[EN["COUNT"] * n:]
    assert np.array_equal(h[:3], [a0, b0, qa]) and np.array_equal(r[:4], [a0, b0, qa, qb])       # bit for bit
    assert np.array_equal(h[5], r[EN["CST"]])                   # the two forms stage the same constant
    al, bl, ql = a0.astype(E.LD), b0.astype(E.LD), qa.astype(E.LD)
    _held("ln qa", h[3], np.log(ql), np.log(qa))
    _held("psi(qa)", h[4], XS.digamma(ql), sp.digamma(qa))
    _held("cst", h[5], _cst(al, bl, XS.digamma, XS.gammaln), _cst(a0, b0, sp.digamma, sp.gammaln))
    # ES_EXACT = 1/2 sum (psi - ln qa): the staged psi and ln qa summed in ascending order, bit for bit; and held as a value
    exact = 0.0
    for p, l in zip(h[4], h[3]):
        exact += p - l
    assert scal[EN["ES_EXACT"]] == 0.5 * exact and scal[EN["ES_OWN"]] == 0.0 and np.all(scal[2:] == 0.0)
    _held("ES_EXACT", scal[EN["ES_EXACT"]:EN["ES_EXACT"] + 1], np.array([0.5 * (XS.digamma(ql) - np.log(ql)).sum()]),
          np.array([0.5 * (sp.digamma(qa) - np.log(qa)).sum()]))
