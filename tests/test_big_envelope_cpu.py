"""CPU: the reference side of tests/test_big_envelope_gpu.py, alone -- the 128-wide LDS class, 64 < max(D, K) <= 128, at every
tile count (extended_ref.BIG_CASES).

  * for every case the float64 oracle is within CAP = 1e-11 of the long-double run: quantity by quantity, tile by tile in the
    tile's own unit (extended_ref.tile_errors), part by part of the bound in both modes -- so 16 max(e64, n 2^-52) never exceeds
    1.6e-10, for a tile as for a whole array; the extended run keeps long double throughout;
  * the cases reach what they are there for: the chunks of the statistics pass and the parts of the time axis as
    pyvb_amd/csrc/geometry.h deals them out (through tests/c/geometry_driver.cpp), the segment lengths of k_sweep_big, and from D
    and K alone the tile counts, the store branch of k_prep_big, the instantiation of k_gy_big, the column blocks and the
    wavefronts of k_cols_big that own rows;
  * extended_ref.compare_tiles and known_offenders, fed a float64 oracle run with one defect planted, flag it where it lives --
    and one of the defects passes the whole-array comparison of tests/test_envelope_gpu.py on the same trace.
"""
import os
import subprocess

import numpy as np
import pytest

import extended_ref as E
from oracle import lds_closed_form as O
from test_extended_ref_cpu import _all_long, _check_bound_records

LD = np.longdouble
HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
NOISE = {"diagonal_gamma": 0, "gamma": 1, "wishart": 2}        # include/pyvb_hip.h: PYVB_NOISE_*


def _shape(name):
    c = E.lds_case(name)
    N, T, K = c["Y"].shape
    return c, N, T, c["st0"]["A_mean"].shape[1], K


def test_the_table_of_cases():
    """The shapes, iterations and priors are those the names say; the earlier tables are untouched by the new one."""
    assert list(E.BIG_CASES) == ["t35_d128_k128", "t27_d127_k113", "t27_d65_k65_n2", "t27_d113_k81_gamma", "t27_d128_k17", "t27_d17_k128",
                                 "t27_d97_k113_known", "t20_d128_k81_wishart", "t20_d97_k128_wishart", "t600_d128_k128_warm"]
    assert not set(E.BIG_CASES) & (set(E.LDS_CASES) | set(E.ROW_CASES))
    assert E.BIG_WARMUP_CASES == ["t35_d128_k128", "t27_d127_k113", "t27_d65_k65_n2", "t27_d128_k17", "t27_d17_k128", "t600_d128_k128_warm"]
    for name in E.BIG_CASES:
        c, N, T, D, K = _shape(name)
        t, d, k = name.split("_")[:3]
        assert (t[0], d[0], k[0]) == ("t", "d", "k") and (T, D, K) == (int(t[1:]), int(d[1:]), int(k[1:])) and 64 < max(D, K) <= 128, name
        assert N == (2 if name.endswith("_n2") else 1)
        assert c["iters"] == (1 if "wishart" in name or "warm" in name else 2)
        assert c["pri"]["noise"] == ("wishart" if "wishart" in name else "gamma" if "gamma" in name else "diagonal_gamma")
        assert not np.isnan(c["Y"]).any()
        # quirk Q2: a prior precision whose determinant is representable where max(D, K) > 102
        want = 1e-2 if max(D, K) > 102 else 1e-3
        assert np.all(c["pri"]["A_prior_prec"] == want) and np.all(c["pri"]["C_prior_prec"] == want), name
        assert ("A_obs" in c["pri"]) == ("known" in name)
    assert E.lds_case("t600_d128_k128_warm")["splits"] == (1, 2) and E.BIG_SPLITS == {"t600_d128_k128_warm": (1, 2)}


def test_the_known_entries_sit_at_the_block_edges():
    c, N, T, D, K = _shape("t27_d97_k113_known")
    for obs, rows in ((c["pri"]["A_obs"], D), (c["pri"]["C_obs"], K)):
        known = ~np.isnan(obs)
        assert obs.shape == (rows, D)
        for col in (15, 16, 17, 95, 96):                # either side of the edges of the 16-column blocks; 96: the last block's one column
            assert 0 < known[:, col].sum() < rows, col
        assert known[rows - 1].any()                    # the last row
        assert sum(known[:, j].all() for j in range(D)) == 1        # one fully known column
        assert known[rows - 1, 95] and not known[rows - 1, 96]      # (the corner entry is a tile of its own: it stays free)
        # no tile of the variances [column, entry] is made of known entries alone
        t = E._tile_max((~known).T.astype(float), (-2, -1))
        assert t.shape == (7, (rows + 15) // 16) and np.all(t == 1.0)
    assert not (~np.isnan(c["pri"]["C_obs"]))[:, 0].any()       # column 0 of C free
    assert (~np.isnan(c["pri"]["A_obs"]))[:, 4].all()


@pytest.fixture(scope="module")
def geometry(tmp_path_factory):
    """pyvb_amd/csrc/geometry.h through tests/c/geometry_driver.cpp (tests/test_geometry_cpu.py runs the same driver under the
    sanitizers): a list of command lines -> the output lines"""
    tmp = tmp_path_factory.mktemp("big_geometry")
    exe = tmp / "geometry_driver"
    subprocess.run(["g++", "-std=c++17", "-O1", "-I", os.path.join(REPO, "pyvb_amd", "csrc"), os.path.join(HERE, "c", "geometry_driver.cpp"),
                    "-o", str(exe)], check=True, capture_output=True)

    def run(lines):
        (tmp / "in.txt").write_text("".join(ln + "\n" for ln in lines))
        p = subprocess.run([str(exe), str(tmp / "in.txt"), str(tmp / "out.txt")], capture_output=True, text=True)
        assert p.returncode == 0, p.stderr[-2000:]
        return (tmp / "out.txt").read_text().splitlines()
    return run


# name -> (nchunk, chunk_len, rows of the last chunk) of the statistics pass
CHUNKS = {
    "t35_d128_k128": (3, 12, 11), "t27_d127_k113": (2, 16, 11), "t27_d65_k65_n2": (2, 16, 11), "t27_d113_k81_gamma": (2, 16, 11),
    "t27_d128_k17": (2, 16, 11), "t27_d17_k128": (2, 16, 11), "t27_d97_k113_known": (2, 16, 11), "t20_d128_k81_wishart": (2, 12, 8),
    "t20_d97_k128_wishart": (2, 12, 8), "t600_d128_k128_warm": (30, 20, 20),
}


def _segments(Tw):
    """(Lseg, live segment columns) of a part of Tw interior nodes in k_sweep_big: 16 columns of Lseg = ceil(Tw / 16) nodes"""
    Lseg = (Tw + 15) >> 4
    return Lseg, (Tw - 1) // Lseg + 1


@pytest.mark.parametrize("name", list(E.BIG_CASES))
def test_cases_reach_what_the_table_says(name, geometry):
    c, N, T, D, K = _shape(name)
    big, dense, nchunk, clen, W = (int(v) for v in geometry(["lds %d %d %d %d %d" % (N, T, D, K, NOISE[c["pri"]["noise"]])])[0].split("|")[0].split())
    assert big == 1 and dense == int("wishart" in name)
    assert W == 1 or name == "t600_d128_k128_warm"          # (the warm-up case is run at forced splits)
    last = T - (nchunk - 1) * clen
    print("%-24s statistics: %d chunks of %d rows, the last of %d" % (name, nchunk, clen, last))
    assert (nchunk, clen, last) == CHUNKS[name]
    # k_stats_big takes a chunk 12 rows at a time, in k-steps of 4 rows
    if name == "t35_d128_k128":
        assert [min(clen, T - i * clen) for i in range(nchunk)] == [12, 12, 11]
    if name == "t27_d127_k113":
        assert 12 < clen <= 24 and last % 4 == 3        # a second trip through the 12-row loop; the last chunk ends inside a k-step
    # the layout: both dimensions padded to eight tiles
    lay = [int(v) for v in geometry(["layout %d %d" % (D, K)])[0].split("|")[0].split()]
    assert lay[:6] == [D, K, 8, 8, 128, 128] and lay[8] == 128
    # from D and K alone
    DT, KT = (D + 15) // 16, (K + 15) // 16
    nbl = (D + 15) >> 4
    cols_A = [32 * w < D for w in range(4)]
    cols_C = [32 * w < K for w in range(4)]
    want = {
        "t35_d128_k128":        dict(DT=8, KT=8, d3=0, kodd=0, nbl=8, A=[1, 1, 1, 1], C=[1, 1, 1, 1], pad_d=0, pad_k=0),
        "t27_d127_k113":        dict(DT=8, KT=8, d3=3, kodd=1, nbl=8, A=[1, 1, 1, 1], C=[1, 1, 1, 1], pad_d=1, pad_k=15),
        "t27_d65_k65_n2":       dict(DT=5, KT=5, d3=1, kodd=1, nbl=5, A=[1, 1, 1, 0], C=[1, 1, 1, 0], pad_d=15, pad_k=15),
        "t27_d113_k81_gamma":   dict(DT=8, KT=6, d3=1, kodd=1, nbl=8, A=[1, 1, 1, 1], C=[1, 1, 1, 0], pad_d=15, pad_k=15),
        "t27_d128_k17":         dict(DT=8, KT=2, d3=0, kodd=1, nbl=8, A=[1, 1, 1, 1], C=[1, 0, 0, 0], pad_d=0, pad_k=15),
        "t27_d17_k128":         dict(DT=2, KT=8, d3=1, kodd=0, nbl=2, A=[1, 0, 0, 0], C=[1, 1, 1, 1], pad_d=15, pad_k=0),
        "t27_d97_k113_known":   dict(DT=7, KT=8, d3=1, kodd=1, nbl=7, A=[1, 1, 1, 1], C=[1, 1, 1, 1], pad_d=15, pad_k=15),
        "t20_d128_k81_wishart": dict(DT=8, KT=6, d3=0, kodd=1, nbl=8, A=[1, 1, 1, 1], C=[1, 1, 1, 0], pad_d=0, pad_k=15),
        "t20_d97_k128_wishart": dict(DT=7, KT=8, d3=1, kodd=0, nbl=7, A=[1, 1, 1, 1], C=[1, 1, 1, 1], pad_d=15, pad_k=0),
        "t600_d128_k128_warm":  dict(DT=8, KT=8, d3=0, kodd=0, nbl=8, A=[1, 1, 1, 1], C=[1, 1, 1, 1], pad_d=0, pad_k=0),
    }[name]
    got = dict(DT=DT, KT=KT, d3=D & 3, kodd=K & 1, nbl=nbl, A=[int(v) for v in cols_A], C=[int(v) for v in cols_C], pad_d=-D % 16, pad_k=-K % 16)
    print("%-24s %r" % (name, got))
    assert got == want
    # the sweeps: segment columns of the one part (of each part where the case is run split)
    if name == "t35_d128_k128":
        assert _segments(T - 2) == (3, 11)              # eleven live columns, five idle
    elif name == "t600_d128_k128_warm":
        parts = geometry(["parts %d 1" % T, "parts %d 2" % T, "check %d 2" % T])
        assert parts[0].split("|")[0].split()[0] == "598" and parts[1].split("|")[0].split() == ["304", "304"]
        assert parts[2].startswith("0|")                # pyvb_lds_set_time_split admits W = 2
        assert _segments(598) == (38, 16) and _segments(304) == (19, 16) and _segments(598 - 304) == (19, 16)
    else:
        assert _segments(T - 2)[0] == 2


@pytest.mark.parametrize("name", list(E.BIG_CASES))
def test_float64_oracle_is_within_the_cap_whole_by_tile_and_by_part(name):
    iters = E.lds_case(name)["iters"]
    for (rows, T, n, ext, e64, rec, run), bnd, til in zip(E.lds_reference(name), E.lds_bound_reference(name), E.lds_tile_reference(name)):
        _all_long(run.st, name)
        _all_long(run.S, name + " statistics")
        assert all(v.dtype == LD for v in ext.values())
        worst = max(e64, key=e64.get)
        print("%-24s largest e64 %.2e at %r" % (name, e64[worst], worst))
        for key, e in e64.items():
            assert e <= E.CAP, "%s %r: float64 oracle %.3e from the extended run, cap %.0e" % (name, key, e, E.CAP)
        assert set(til) == {k for k in ext if k[2] in E.TILE_QUANTITIES} and any(k[2] == "X" for k in til)
        byq = {}
        for key, e in til.items():
            assert e.shape == E.tile_errors(ext[key], ext[key], key[2]).shape and np.all(np.isfinite(e)), (name, key)
            byq[key[2]] = max(byq.get(key[2], 0.0), float(e.max()))
        print("%-24s largest e64 by tile: %s" % (name, "  ".join("%s %.2e" % kv for kv in byq.items())))
        for key, e in til.items():
            assert e.max() <= E.CAP, "%s %r: float64 oracle %.3e from the extended run in tile %r, cap %.0e" \
                % (name, key, e.max(), np.unravel_index(e.argmax(), e.shape), E.CAP)
        assert set(bnd) == {(it, "bound", m) for it in range(iters) for m in E.BOUND_MODES}
        _check_bound_records(name, bnd, E.LDS_PARTS)


def test_the_warmup_case_leaves_columns_that_start_from_zero():
    """The documented warm-up rule on the recurrence matrices of the extended run gives J* below the segment length at either
    split, so a kernel that follows it has columns that warm up from zero (the GPU test asserts 0 < J < Lseg on the handle)."""
    (rows, T, n, ext, e64, rec, run), = E.lds_reference("t600_d128_k128_warm")
    F, B = rec[0]
    Jf, Jb = E.warmup_rule(F[0], "inf"), E.warmup_rule(B[0], "1")
    print("t600_d128_k128_warm: J* forward %d, backward %d; Lseg 38 at W = 1, 19 at W = 2" % (Jf, Jb))
    assert 0 < Jf + 4 < 19 and 0 < Jb + 4 < 19


def test_tile_errors_on_arrays_whose_answer_is_known():
    ext = np.ones((2, 3, 40, 33), dtype=LD)
    got = ext.copy()
    got[1, 2, 39, 32] += LD(1e-12)              # the ragged corner tile
    got[0, 0, 16, 15] *= 1 + LD(1e-13)
    e = E.tile_errors(got, ext)
    assert e.shape == (2, 3, 3, 3) and e.dtype == np.float64
    want = np.zeros((2, 3, 3, 3)); want[1, 2, 2, 2] = 1e-12; want[0, 0, 1, 0] = 1e-13
    assert np.allclose(e, want, rtol=1e-6, atol=0)
    # a tile's own unit: a small tile beside a large one
    ext[0, 1, :16, 16:32] = LD(1e-6)
    got = ext.copy(); got[0, 1, 3, 20] += LD(1e-16)
    assert np.isclose(E.tile_errors(got, ext)[0, 1, 0, 1], 1e-10) and E.rel(got, ext) <= 1.0001e-16
    # a zero tile is zero or nothing
    ext[1, 0, 32:, :16] = 0
    got = ext.copy()
    assert E.tile_errors(got, ext)[1, 0, 2, 0] == 0.0
    got[1, 0, 35, 2] = 1e-300
    assert E.tile_errors(got, ext)[1, 0, 2, 0] == np.inf
    # the states: the 16-entry tile of each node
    x = np.arange(1.0, 2 * 5 * 20 + 1).reshape(2, 5, 20).astype(LD)
    g = x.copy(); g[1, 4, 19] *= 1 + LD(1e-12)
    e = E.tile_errors(g, x, "X")
    assert e.shape == (2, 5, 2) and np.isclose(e[1, 4, 1], 1e-12) and np.count_nonzero(e) == 1


# ----------------------------------------------------------------------------------------------------------------------------
# mutants
# ----------------------------------------------------------------------------------------------------------------------------
class _MirroredStoreGoneWrong(E.OracleLDS):
    """Block (7, 5) of Sxx formed without the last node; block (5, 7) is right."""

    def update_A(self):
        E.OracleLDS.update_A(self)
        xL = self.st["X"][:, -1]
        self.S["Sxx"] = self.S["Sxx"].copy()
        self.S["Sxx"][:, 112:128, 80:96] -= np.einsum("ni,nj->nij", xL[:, 112:128], xL[:, 80:96])


class _ClampedLoadOfTheLastOutput(E.OracleLDS):
    """Output K - 1 reads the observation of output K - 2 in the interior nodes of the forward sweep."""

    def sweep(self, direction):
        if direction != "forward":
            return E.OracleLDS.sweep(self, direction)
        keep = self.Y
        self.Y = keep.copy()
        self.Y[:, 1:-1, -1] = keep[:, 1:-1, -2]
        E.OracleLDS.sweep(self, direction)
        self.Y = keep


class _PaddedRowOfSigma(E.OracleLDS):
    """Row D - 1 of the interior Sigma taken from the padded system: the diagonal entry D - 1 of the precision + 1 before the
    inversion (what the identity in the padding of a 128 x 128 work matrix does to a row it leaks into)."""

    def sweep(self, direction):
        if direction != "forward":
            return E.OracleLDS.sweep(self, direction)
        self.post = O.state_posteriors(self.st, self.pri)
        P = self.post["P"][:, 1].copy()
        P[:, -1, -1] += 1.0
        self.post["Sigma"] = self.post["Sigma"].copy()
        self.post["Sigma"][:, 1, -1, :] = np.linalg.inv(P)[:, -1, :]
        O.sweep(self.st, self.pri, self.Y, direction, self.post)


def _float64_trace(name, make=E.OracleLDS, iters=1):
    c = E.lds_case(name)
    m = make(c["Y"].copy(), {k: v.copy() for k, v in c["st0"].items()}, c["pri"])
    return list(E.lds_trace(m, iters, False))


def _first(off):
    """the offending tiles of the first key that has any: where a defect shows first"""
    return off[0][1], [o[2] for o in off if o[1] == off[0][1]]


def test_big_comparison_catches_mutants():
    """extended_ref.compare_tiles (and compare_with_reference, known_offenders) on the float64 oracle with one defect planted,
    one iteration each.  The unmutated oracle has no offending tile: its e_tile is e64_tile, at most the yardstick."""
    for name in ("t35_d128_k128", "t27_d127_k113"):
        clean = _float64_trace(name)
        rows = E.compare_tiles(name, clean, tag="float64 oracle " + name)
        assert rows and not E.offending_tiles(rows) and max(float(r[4].max()) for r in rows) <= 1.0

    # 1. a mirrored store gone wrong: the defect is in Sxx alone (not in Sxx_m, which update_A reads), so update_C is its first
    # reader; columns 112..127 of C read rows 112..127 of Sxx, block (7, 5) among them, and the Gauss-Seidel pass has done the
    # columns before them by then
    off = E.offending_tiles(E.compare_tiles("t35_d128_k128", _float64_trace("t35_d128_k128", _MirroredStoreGoneWrong), tag="mutant: Sxx block (7, 5)"))
    key, tiles = _first(off)
    assert key == (0, "update_C", "C_mean") and tiles and all(t[-1] == 7 for t in tiles), (key, tiles)
    assert {t[-2] for t in tiles} == set(range(8))          # every row tile of those columns
    assert not [o for o in off if o[1][2] in ("X", "Sigma", "A_mean")]

    # 2. the clamp of the odd-K loads: shows in the states of the forward sweep, from node 1 on (node 0 is done before any interior node)
    off = E.offending_tiles(E.compare_tiles("t27_d127_k113", _float64_trace("t27_d127_k113", _ClampedLoadOfTheLastOutput), tag="mutant: output K - 1"))
    key, tiles = _first(off)
    assert key == (0, "forward sweep", "X") and tiles and all(t[1] >= 1 for t in tiles), (key, tiles)
    assert {t[1] for t in tiles} >= set(range(1, 26))       # every interior node

    # 3. a padded row of Sigma: row tile 7 of the interior class, no other class and no other row tile
    off = E.offending_tiles(E.compare_tiles("t27_d127_k113", _float64_trace("t27_d127_k113", _PaddedRowOfSigma), tag="mutant: Sigma row D - 1"))
    tiles = [o[2] for o in off if o[1] == (0, "backward sweep", "Sigma")]
    assert tiles and all(t[1] == 1 and t[2] == 7 for t in tiles), tiles
    assert _first(off)[0] == (0, "forward sweep", "X")      # (and the states read it first)

    # 4. one small off-diagonal tile of the interior Sigma, off by half of what the whole-array bound admits
    name = "t35_d128_k128"
    (rows_, T, n, ext, e64, _, _), = E.lds_reference(name)
    key = (0, "backward sweep", "Sigma")
    big = E._tile_max(ext[key], (-2, -1))[0, 1]
    off_diag = np.where(np.eye(8, dtype=bool), np.inf, big.astype(float))
    i, j = (int(v) for v in np.unravel_index(off_diag.argmin(), off_diag.shape))
    whole = float(np.abs(ext[key]).max())
    eps = 0.5 * E.FACTOR * E.yardstick(e64[key], n) * whole / float(big[i, j])
    print("mutant: Sigma tile (%d, %d) of the interior class times 1 + %.2e: the tile's largest entry %.2e, the array's %.2e" % (i, j, eps, big[i, j], whole))
    assert eps < 1e-8           # the suite's RTOL cannot see it either
    trace = [(k, a.copy()) for k, a in _float64_trace(name)]
    dict(trace)[key][0, 1, 16 * i:16 * i + 16, 16 * j:16 * j + 16] *= 1.0 + eps
    whole_rows = E.compare_with_reference(name, trace)
    assert max(r[4] for r in whole_rows) <= E.FACTOR, "the whole-array comparison was to pass"
    off = E.offending_tiles(E.compare_tiles(name, trace, tag="mutant: one tile of Sigma"))
    assert [(o[1], o[2]) for o in off] == [(key, (0, 1, i, j))], off

    # 5. a known entry of A times 1 + 2^-50
    c = E.lds_case("t27_d97_k113_known")
    obs = c["pri"]["A_obs"]
    D = obs.shape[0]
    mean = np.where(np.isnan(obs), 0.25, obs)[None].copy()
    colvar = np.where(np.isnan(obs), 1e-3, 0.0).T[None].copy()
    assert E.known_offenders("A", mean, colvar, obs) == []
    assert not np.isnan(obs[D - 1, 95])
    mean[0, D - 1, 95] *= 1.0 + 2.0 ** -50
    assert E.known_offenders("A", mean, colvar, obs) == [("A", 0, D - 1, 95, "mean")]
    colvar[0, 16, 31] = 1e-300          # (column 16, row 31)
    assert not np.isnan(obs[31, 16])
    assert E.known_offenders("A", mean, colvar, obs) == [("A", 0, D - 1, 95, "mean"), ("A", 0, 31, 16, "variance")]
