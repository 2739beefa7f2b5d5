"""CPU: the reference side of tests/test_pca_rows_gpu.py, alone.

  * the row patterns are what they are named (extended_ref.pca_pattern_mask), a pattern that is empty or degenerate at a width
    is replaced by the nearest one that is not and labelled so, and every case carries every pattern it is wide enough for;
  * the cases reach what they are there for: the partitions of the sweeps (pyvb_amd/csrc/geometry.h, through tests/c/geometry_driver.cpp)
    give the long cases several tiles a chunk, the tile counts and the kernel forms of the small ones are as the table says;
  * for every case the float64 oracle is within CAP = 1e-11 of the long-double run: quantity by quantity, part by part of the
    bound in both modes, and row by row in the row's own unit -- so 16 max(e64_row, n 2^-52) never exceeds 1.6e-10;
  * extended_ref.compare_pca_rows, fed a float64 oracle run with one defect planted in update_X, flags exactly the rows
    concerned, and none of the unmutated run.

The long cases are run at the CU count of the MI355X (256).
"""
import os
import subprocess

import numpy as np
import pytest

import extended_ref as E

LD = np.longdouble
HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
NCU = 256


@pytest.mark.parametrize("d", [1, 2, 17, 64, 128, 129, 240, 241, 256])
def test_patterns_are_what_they_are_named(d):
    k = np.arange(d)
    rng = np.random.default_rng(d)
    want = {"all": k >= 0, "one known, first": k != 0, "one known, last": k != d - 1, "one missing, first": k == 0,
            "one missing, last": k == d - 1, "a byte of a word": k == 5, "a word": (k >= 4) & (k <= 7), "a tile": (k >= 16) & (k <= 31),
            "a block": (k >= 32) & (k <= 63), "alternating": k % 2 == 0, "upper half": k >= d // 2, "low half": k <= 127,
            "the seam": (k == 127) | (k == 128), "the last tile": k >= 16 * ((d - 1) // 16), "observed": k < 0}
    assert set(want) | {"Bernoulli"} == set(E.PCA_ROW_PATTERNS) and len(E.PCA_ROW_PATTERNS) == 16
    for name in E.PCA_ROW_PATTERNS:
        m = E.pca_pattern_mask(name, d, rng)
        if name == "Bernoulli":
            assert (m is None) == (d < 2)
            assert m is None or (m.any() and not m.all())
            continue
        w = want[name]
        degenerate = (name != "all" and w.all()) or (name != "observed" and not w.any()) or (name == "the seam" and d < 129)
        assert (m is None) == bool(degenerate), (name, d)
        assert m is None or (m.dtype == bool and np.array_equal(m, w)), (name, d)
    # the widths at which a pattern first exists
    assert E.pca_pattern_mask("the seam", 128) is None and E.pca_pattern_mask("the seam", 129).sum() == 2
    assert E.pca_pattern_mask("low half", 128) is None and E.pca_pattern_mask("low half", 129).sum() == 128
    assert E.pca_pattern_mask("a block", 32) is None and E.pca_pattern_mask("a block", 33).sum() == 1
    assert E.pca_pattern_mask("the last tile", 16) is None and E.pca_pattern_mask("the last tile", 241).sum() == 1


def _wide_enough(d):
    return [p for p in E.PCA_ROW_PATTERNS if E.pca_pattern_mask(p, d, np.random.default_rng(0)) is not None]


@pytest.mark.parametrize("name", list(E.PCA_ROW_CASES))
def test_cases_carry_the_patterns(name):
    c = E.pca_rows_case(name, NCU)
    N, d, q, miss, labels = c["N"], c["d"], c["q"], c["miss"], c["patterns"]
    init = c["init"]
    print("%-28s N %d d %d q %d  %d rows with a missing entry, %d of them with nothing observed, %d fully observed"
          % (name, N, d, q, c["has"].sum(), miss.all(1).sum(), (~c["has"]).sum()))
    assert miss.shape == (N, d) and len(labels) == N and np.array_equal(init["obs"], ~miss)
    assert init["X"].shape == (N, d) and np.all(np.isfinite(init["X"]))
    # every pattern this width has room for occurs under its own name -- a later edit cannot silently drop the seam
    wide = _wide_enough(d)
    # (at d = 1, with 15 rows, "observed" occurs as what stands in for the patterns that need a second column)
    names = set(labels) if N >= len(E.PCA_ROW_PATTERNS) else {lab.split(" (")[0] for lab in labels}
    assert set(wide) <= names, (name, sorted(set(wide) - names))
    if d >= 129:
        assert "the seam" in labels and "low half" in labels
    # a replaced pattern says what it stands for, and is one that exists at this width
    for n, lab in enumerate(labels):
        if n == 0 and c["row0"] != "partial":
            continue
        asked = E.PCA_ROW_PATTERNS[n % 16]
        if asked in wide:
            assert lab == asked, (name, n, lab)
        else:
            assert lab.endswith(" (for %s)" % asked) and lab[:-len(" (for %s)" % asked)] in wide, (name, n, lab)
    # the rows are the patterns, under the two column patterns where N and d allow them
    cols = E.pca_has_column_patterns(N, d)
    assert cols == (name != "n15_d1_q1")
    rng = np.random.default_rng(0)
    for n, lab in enumerate(labels):
        base = lab.split(" (")[0]
        if base == "Bernoulli":
            continue
        m = E.pca_pattern_mask(base, d, rng).copy()
        if cols and not (n == 0 and c["row0"] == "observed"):
            m[d // 3] = True
            m[2] = n != 8
        assert np.array_equal(miss[n], m), (name, n, lab)
    if cols:
        seen = ~miss
        exempt = c["row0"] == "observed"
        assert seen[:, d // 3].sum() == (1 if exempt else 0)                   # a column no row observes
        assert np.array_equal(np.nonzero(seen[:, 2])[0], [0, 8] if exempt else [8])      # a column one row observes
    # row 0: the row the crawl order updates alone
    if c["row0"] == "partial":
        assert (miss[0].any() and not miss[0].all()) or d == 1
    elif c["row0"] == "missing":
        assert miss[0].all() and labels[0] == "all (row 0)"
    else:
        assert not miss[0].any() and labels[0] == "observed (row 0)"
    assert ("X_full" in init) == c["unpinned"] == ("X_var0" in init)
    if c["unpinned"]:
        assert init["X_full"].shape == (N, d) and init["X_var0"].shape == (N,) and np.all(init["X_var0"] > 0)


def test_the_problem_is_pca_problem_with_another_mask():
    init0, pri0 = E.pca_problem(40, 129, 16)
    c = E.pca_rows_case("n40_d129_q16")
    for k in ("W_mean", "Z", "Z_cov", "Mu_mean", "beta_b"):
        assert np.array_equal(init0[k], c["init"][k]), k
    assert all(np.array_equal(pri0[k], c["pri"][k]) for k in pri0)
    both = init0["obs"] & c["init"]["obs"]
    assert both.sum() > 1000 and np.array_equal(init0["X"][both], c["init"]["X"][both])
    assert E.pca_rows_case("long_d256_q16", NCU)["N"] == 80 * NCU + 24 and E.pca_rows_case("long_d32_q16", NCU)["N"] == 144 * NCU + 8
    assert E.pca_rows_case("long_d32_q16", 8)["N"] == 144 * 8 + 8


@pytest.fixture(scope="module")
def geometry(tmp_path_factory):
    """pca_geometry of pyvb_amd/csrc/geometry.h through tests/c/geometry_driver.cpp (tests/test_geometry_cpu.py runs the same
    driver under the sanitizers): (N, d, q, ncu) -> dict"""
    tmp = tmp_path_factory.mktemp("pca_rows_geometry")
    exe = tmp / "geometry_driver"
    subprocess.run(["g++", "-std=c++17", "-O1", "-I", os.path.join(REPO, "pyvb_amd", "csrc"), os.path.join(HERE, "c", "geometry_driver.cpp"),
                    "-o", str(exe)], check=True, capture_output=True)

    def run(N, d, q, ncu):
        (tmp / "in.txt").write_text("pca %d %d %d %d\n" % (N, d, q, ncu))
        p = subprocess.run([str(exe), str(tmp / "in.txt"), str(tmp / "out.txt")], capture_output=True, text=True)
        assert p.returncode == 0, p.stderr[-2000:]
        v = [int(x) for x in (tmp / "out.txt").read_text().split()]
        return dict(zip(("DP", "QP", "DT", "QT", "nchunk", "rows", "nchunkB", "rowsB", "sweep"), v))
    return run


def test_cases_reach_what_they_are_there_for(geometry):
    """The kernel forms follow from DT and QT (k_pca.hip: pca_launch_sweep, pca_pass2), the work of a wavefront from the partition.
    A pair of k_pca_pairs (four a workgroup) takes tiles pair, pair + 4, ...; k_pca_pass12 at QT = 1 takes two tiles a step."""
    g = {name: geometry(E.pca_rows_case(name, NCU)["N"], c["d"], c["q"], NCU) for name, c in E.PCA_ROW_CASES.items()}
    for name, v in g.items():
        c = E.pca_rows_case(name, NCU)
        print("%-28s N %6d  DT %2d QT %d  pass 2 / 1+2: %4d chunks of %3d rows   pairs: %4d chunks of %3d rows"
              % (name, c["N"], v["DT"], v["QT"], v["nchunk"], v["rows"], v["nchunkB"], v["rowsB"]))
        # the lazy sweeps exist at QT = 1 only (pca_plan.h: plan_sweep)
        assert v["QT"] == 1 or set(c["sweeps"]) == {"store"}, name
    assert [g[n]["DT"] for n in ("n70_d256_q16", "n37_d241_q16", "n70_d240_q7", "n40_d129_q16", "n33_d128_q5", "n20_d17_q1")] == [16, 16, 15, 9, 8, 2]
    assert [g[n]["DT"] for n in ("n35_d192_q17", "n35_d208_q17", "n37_d209_q32")] == [12, 13, 14] and g["n37_d209_q32"]["QT"] == 2
    # the DT >= 13 rule: one chunk a CU from DT = 13 on, 16384 / DT chunks below -- where the tile count does not cap them first
    assert geometry(10 ** 6, 192, 17, NCU)["nchunk"] > NCU and geometry(10 ** 6, 208, 17, NCU)["nchunk"] == NCU
    # a ragged last tile: 70 = 4 x 16 + 6, 37 = 2 x 16 + 5; exactly one full tile
    assert (g["n70_d256_q16"]["nchunk"], g["n70_d256_q16"]["rows"], g["n70_d256_q16"]["nchunkB"], g["n70_d256_q16"]["rowsB"]) == (5, 16, 2, 64)
    assert (g["n16_d64_q16"]["nchunk"], g["n16_d64_q16"]["rows"]) == (1, 16)
    # the long cases: N = 80 ncu + 24 and 144 ncu + 8 round up to SIX and TEN tiles a chunk (81 and 145 rows a CU, in tiles of 16)
    a, b = g["long_d256_q16"], g["long_d32_q16"]
    Na, Nb = 80 * NCU + 24, 144 * NCU + 8
    assert (a["rows"], a["rowsB"], b["rowsB"]) == (96, 96, 160)
    assert a["rowsB"] // 16 > 4 and b["rowsB"] // 16 > 8                # pair 0 goes on to a second / a third tile
    assert -(-(a["rows"] // 16) // 2) == 3                             # k_pca_pass12: three steps of two tiles
    assert Na % a["rowsB"] == 56 and Nb % b["rowsB"] == 72             # a ragged last chunk, its last tile half full
    assert a["nchunkB"] < NCU and b["nchunkB"] < NCU
    # ... and 24 rows below 80 a CU to five: pass12 ends on a step with one tile of its two, every CU has a chunk
    f = g["long_d256_q16_five_tiles"]
    assert (f["rows"], f["nchunk"], f["rowsB"], f["nchunkB"]) == (80, NCU, 80, NCU) and (80 * NCU - 24) % 80 == 56
    assert not E.PCA_ROW_CASES["long_d256_q16_five_tiles"]["bounds"] and all(c["bounds"] for n, c in E.PCA_ROW_CASES.items() if "five" not in n)


@pytest.mark.parametrize("name", list(E.PCA_ROW_CASES))
def test_float64_oracle_is_within_the_cap(name):
    c = E.pca_rows_case(name, NCU)
    ref = E.pca_rows_reference(name, NCU)
    assert all(v.dtype == LD for v in ref["ext"].values()) and ref["n"] == max(c["d"], c["q"], c["N"])
    worst = max(ref["e64"], key=ref["e64"].get)
    print("%-28s largest e64 %.2e at %r" % (name, ref["e64"][worst], worst))
    for key, e in ref["e64"].items():
        assert e <= E.CAP, "%s %r: float64 oracle %.3e from the extended run, cap %.0e" % (name, key, e, E.CAP)
    assert len(ref["bound"]) == (2 * c["iters"] if c["bounds"] else 0)
    for key, (ext, e64, _) in sorted(ref["bound"].items()):
        print("%-28s it%d %-9s " % (name, key[0], key[2]) + "  ".join("%s %.1e" % (nm, e64[:, p].max()) for p, nm in enumerate(E.PCA_PARTS)))
        assert ext.dtype == LD and ext.shape == (1, 5) and np.all(np.isfinite(ext)) and np.all(e64 <= E.CAP), (name, key, e64)
    # row by row
    stages = 3 if True in c["schedules"] else 0         # Z after update_Z, X and X_rowvar after update_X
    assert len(ref["rows"]) == c["iters"] * (stages + 3)
    largest = 0.0
    for key in sorted(ref["rows"]):
        e = ref["rows"][key]
        assert e.shape == (c["N"],)
        measured = np.ones(c["N"], dtype=bool) if key[2] == "Z" else c["has"]
        assert np.array_equal(np.isnan(e), ~measured), (name, key)
        r = int(np.nanargmax(e))
        largest = max(largest, float(e[r]))
        print("%-28s it%d %-11s %-8s largest e64_row %.2e (row %d, %s)" % (name, key[0], key[1], key[2], e[r], r, c["patterns"][r]))
        assert np.all(e[measured] <= E.CAP), "%s %r: float64 oracle %.3e from the extended run in a row's own unit (row %d, %s), cap %.0e" \
            % (name, key, e[r], r, c["patterns"][r], E.CAP)
    print("%-28s SUMMARY largest e64_row %.2e" % (name, largest))


def test_row_errors_are_row_errors():
    """pca_row_errors on X is row_errors (the LDS outputs' measure) for all rows at once"""
    c = E.pca_rows_case("n40_d129_q16")
    ref = E.pca_rows_reference("n40_d129_q16")
    run64 = dict(E.pca_float64_rows("n40_d129_q16"))
    for key in [k for k in ref["rows"] if k[2] == "X"]:
        slow = E.row_errors(run64[key][None], ref["ext"][key][None], c["miss"][None])[0]
        assert np.array_equal(np.isnan(slow), np.isnan(ref["rows"][key]))
        assert np.array_equal(slow[c["has"]], ref["rows"][key][c["has"]])


# ----------------------------------------------------------------------------------------------------------------------------
# mutants of update_X
# ----------------------------------------------------------------------------------------------------------------------------
# Planted in rows 1 .. N - 1 only: row 0 is updated before Mu, so a defect there reaches every row of the same iteration through
# <Mu> and there would be no "rows concerned".
def _pred(run):
    return run.st["Z"] @ run.st["W_mean"].T + run.st["Mu_mean"]


def _plant_last_column(run, c, rows):
    """the prediction written over the observed entry d - 1"""
    d = c["d"]
    hit = [n for n in rows if c["has"][n] and not c["miss"][n, d - 1]]
    run.st["X"][hit, d - 1] = _pred(run)[hit, d - 1]
    return hit


def _words(c, n):
    """the 4-entry mask words of row n with both missing and observed entries"""
    d, m = c["d"], c["miss"][n]
    return [w for w in range(0, d, 4) if m[w:w + 4].any() and not m[w:w + 4].all()]


def _plant_word(run, c, rows):
    """a whole mask word imputed when one of its bytes is missing"""
    pred = _pred(run)
    hit = [n for n in rows if _words(c, n)]
    for n in hit:
        for w in _words(c, n):
            run.st["X"][n, w:w + 4] = pred[n, w:w + 4]
    return hit


def _plant_128(run, c, rows):
    """column 128 treated as observed: it is left at its initial mean"""
    hit = [n for n in rows if c["miss"][n, 128]]
    run.st["X"][hit, 128] = c["init"]["X"][hit, 128]
    return hit


def _ragged(c):
    return range(16 * (c["N"] // 16), c["N"])


def _plant_stale_z(run, c, rows):
    """the rows of the last ragged tile imputed from the previous iteration's z"""
    hit = [n for n in rows if n in _ragged(c) and c["has"][n]]
    pred = run.Z_before @ run.st["W_mean"].T + run.st["Mu_mean"]
    for n in hit:
        run.st["X"][n, c["miss"][n]] = pred[n, c["miss"][n]]
    return hit


def _plant_rowvar(run, c, rows):
    """X_rowvar of the fully missing rows left at its initial value"""
    hit = [n for n in rows if c["miss"][n].all()]
    run.st["X_var"][hit] = 0.0
    return hit


# name -> (the cases it is planted in, plant(run, case, rows), the rows it concerns among 1 .. N - 1)
PCA_MUTANTS = {
    "the prediction over the observed entry d - 1": (["n70_d256_q16", "n40_d129_q16", "n20_d17_q1"], _plant_last_column,
                                                      lambda c: {n for n in range(1, c["N"]) if c["has"][n] and not c["miss"][n, -1]}),
    "a whole mask word imputed for one missing byte": (["n70_d256_q16", "n37_d241_q16", "n20_d17_q1"], _plant_word,
                                                        lambda c: {n for n in range(1, c["N"]) if _words(c, n)}),
    "column 128 treated as observed": (["n70_d256_q16", "n40_d129_q16"], _plant_128, lambda c: {n for n in range(1, c["N"]) if c["miss"][n, 128]}),
    "the last ragged tile imputed from the previous z": (["n70_d256_q16", "n37_d241_q16", "n33_d128_q5"], _plant_stale_z,
                                                          lambda c: {n for n in _ragged(c) if n >= 1 and c["has"][n]}),
    "X_rowvar of the fully missing rows left at 0": (["n70_d256_q16", "n20_d17_q1"], _plant_rowvar,
                                                      lambda c: {n for n in range(1, c["N"]) if c["miss"][n].all()}),
}


@pytest.mark.parametrize("mutant", list(PCA_MUTANTS))
def test_pca_row_comparison_catches_mutants(mutant):
    """compare_pca_rows on the float64 oracle with one defect planted in update_X (applied after every call of it, so it carries
    over into the next iteration as a kernel's would).  In the first iteration exactly the rows concerned are flagged, every one
    of them and no other; in the second they still are, beside whatever the carried-over defect has reached.  The unmutated
    oracle is within its own yardstick on every row (e_row = e64_row <= y) and holds every pin."""
    cases, plant, concerned = PCA_MUTANTS[mutant]
    for name in cases:
        c = E.pca_rows_case(name)
        want = {int(n) for n in concerned(c)}
        assert want and len(want) < c["N"] - 1, "%s: %s concerns %d rows of %d" % (mutant, name, len(want), c["N"])
        planted = set()

        class Mutant(E.OraclePCA):
            def update_Z(self):
                self.Z_before = self.st["Z"].copy()
                E.OraclePCA.update_Z(self)

            def update_X(self, lo, hi):
                E.OraclePCA.update_X(self, lo, hi)
                planted.update(plant(self, c, range(max(lo, 1), hi)))

        run64, runm = E.pca_float64_rows(name), E.pca_float64_rows(name, make=Mutant)
        assert planted == want
        clean = E.compare_pca_rows(name, run64, tag=name + " float64")
        assert len(clean) == c["N"] * 6 * c["iters"] and not E.offending_rows(clean) and max(r[6] for r in clean) <= 1.0 + 1e-9
        rows = E.compare_pca_rows(name, runm, tag=name + " mutant")
        assert [r[:4] for r in rows] == [r[:4] for r in clean]
        for it in range(c["iters"]):
            flagged = {r[2] for r in E.offending_rows(rows) if r[0][0] == it}
            print("%-50s %-16s it%d flags %s" % (mutant, name, it, sorted(flagged)))
            if it == 0:
                assert flagged == want, "%s, %s: flagged %r, concerned %r" % (mutant, name, sorted(flagged), sorted(want))
            else:
                assert flagged >= want, "%s, %s it%d: flagged %r, concerned %r" % (mutant, name, it, sorted(flagged), sorted(want))
