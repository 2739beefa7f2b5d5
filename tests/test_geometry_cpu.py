"""CPU-only: what a handle is sized as (pyvb_amd/csrc/geometry.h) needs no device.  tests/c/geometry_driver.cpp is built here with
the address and undefined-behaviour sanitizers (runtimes linked statically, as tests/test_replicates_cpu.py builds its driver)
and run on commands written out below; what it answers is compared with tables recorded from the library on a device, and with
the rules spelled out in numpy / Python in this file:

* the recorded tables -- the time split, the chunks of the statistics pass and the partitions of the VB-PCA sweeps that handles
  of commit 83891e5 (the parent of the commit that introduced geometry.h) had on an MI355X with 256 compute units;
* properties of the cut of the time axis, of the extents and of the layouts on a few thousand random shapes, with the time split
  forced over every admitted value;
* the pinned cases with a part that holds no node, and the verbatim refusals of check_time_split.
"""
import os
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
SAN = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan"]
OK, E_ARG = 0, 1
DIAGONAL_GAMMA, WISHART = 0, 2

# Recorded at commit 83891e5 on one MI355X by a job that created a handle per shape with the library built from that commit:
# W is pyvb_lds_get_time_split(); nchunk is the x extent of the grid of k_stats / k_stats_big (in workgroups) in a
# rocprofv3 --kernel-trace of one iterate(1).  chunk_len is not visible from outside a handle and is held to its rule below.
# (N, T, D, K): (nchunk, W)
LDS_TABLE = {
    (1, 66, 16, 16): (5, 1), (1, 129, 16, 16): (9, 1), (1, 130, 16, 16): (9, 2), (1, 600, 6, 4): (30, 7), (2, 777, 16, 16): (28, 10),
    (3, 1030, 33, 17): (29, 13), (5, 4099, 8, 8): (32, 43),
    (1, 2050, 64, 64): (31, 26), (8, 2000, 64, 64): (32, 21), (64, 1000, 32, 32): (16, 13), (200, 700, 16, 16): (6, 5), (512, 300, 16, 16): (2, 2),
    (1, 10000, 16, 16): (32, 125), (1024, 10000, 64, 64): (1, 1),
    (2, 1500, 100, 70): (32, 16), (3, 130, 100, 70): (9, 2), (300, 400, 128, 128): (4, 1), (2, 12, 6, 4): (1, 1),
}
# The same job, VB-PCA: the default kind is pyvb_pca_get_sweep(); nchunk is the x extent of the grid of k_pca_pass2 and nchunkB
# that of k_pca_pairs (put on the handle with set_sweep), in workgroups; None: latent dimensions beyond 16 never reach k_pca_pairs.
# (N, d, q): (nchunk, nchunkB, default sweep)
PCA_NCU = 256
PCA_TABLE = {
    (16, 3, 1): (1, 1, "columns"), (17, 250, 31): (2, None, "columns"), (77, 33, 17): (5, None, "columns"), (300, 20, 4): (19, 5, "columns"),
    (600, 250, 16): (38, 10, "columns"), (1000, 64, 16): (63, 16, "columns"), (5000, 256, 16): (157, 79, "columns"),
    (140000, 256, 16): (250, 250, "pairs"), (10 ** 6, 256, 16): (256, 256, "pairs"),
}
SWEEP_NAMES = {0: "store", 1: "columns", 2: "pairs"}


def test_the_constants_are_the_header_s():
    from pyvb_amd import _capi
    assert (OK, E_ARG) == (_capi.OK, _capi.E_ARG)
    assert (DIAGONAL_GAMMA, WISHART) == (_capi.NOISE_DIAGONAL_GAMMA, _capi.NOISE_WISHART)
    assert {v: k for k, v in _capi.PCA_SWEEPS.items()} == SWEEP_NAMES


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("geometry")
    probe = tmp / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    if subprocess.run(SAN + [str(probe), "-o", str(tmp / "probe")], capture_output=True).returncode != 0:
        pytest.skip("this compiler cannot link the static sanitizer runtimes")
    exe = tmp / "geometry_driver"
    subprocess.run(SAN + ["-Wall", "-I", os.path.join(REPO, "pyvb_amd", "csrc"), os.path.join(HERE, "c", "geometry_driver.cpp"), "-o", str(exe)],
                   check=True, capture_output=True)

    def run(commands):
        """commands: lists of a word and integers.  Returns the output lines."""
        (tmp / "in.txt").write_text("".join(" ".join(str(x) for x in c) + "\n" for c in commands))
        p = subprocess.run([str(exe), str(tmp / "in.txt"), str(tmp / "out.txt")], capture_output=True, text=True)
        assert p.returncode == 0, "the sanitized driver failed:\n" + p.stderr[-4000:]
        lines = (tmp / "out.txt").read_text().split("\n")[:-1]
        assert len(lines) == len(commands)
        return lines
    return run


def _ints(s):
    return [int(x) for x in s.split()]


def _lds(line):
    head, ext = line.split("|")
    big, dense, nchunk, chunk_len, W = _ints(head)
    return dict(big=bool(big), dense=bool(dense), nchunk=nchunk, chunk_len=chunk_len, W=W), dict(zip(
        ("sxx", "U2", "trash", "scratch", "SG", "stats", "mom", "priors"), _ints(ext)))


def _tiles(d):
    return 1 if d <= 16 else 2 if d <= 32 else 4 if d <= 64 else 8


def _extents(N, T, D, K, dense, nchunk, W):
    """Every extent of a handle in doubles, as the creation of a handle spelled them before geometry.h."""
    big = D > 64 or K > 64
    DP = 128 if big else 16 * _tiles(D)
    KP = 128 if big else 16 * _tiles(K)
    return dict(sxx=8 if big else N * W * DP * DP, U2=N * T * DP if big and W > 1 else 0, trash=N * (W if big else 1) * 512,
                scratch=N * 2 * DP * DP if big else N * 2 * D * D, SG=0 if not dense else N * 2 * (128 * 128 if big else 64 * 64),
                stats=N * nchunk * (2 * DP * DP + KP * DP), mom=N * (3 * D * D + K * D + D),
                priors=D + 3 * D * D + 2 * K * D + 2 * D + 2 * K + D * D + K * D + 2 * D + D * D + K * K)


def _admitted(T):
    return [W for W in range(1, 129) if W == 1 or (T - 2) // W >= 16]


# ---- the recorded tables ------------------------------------------------------------------------------------------------------
def test_lds_geometry_reproduces_the_recorded_table(driver):
    shapes = list(LDS_TABLE)
    out = driver([["lds", N, T, D, K, DIAGONAL_GAMMA] for (N, T, D, K) in shapes])
    for shape, line in zip(shapes, out):
        g, _ = _lds(line)
        T = shape[1]
        assert (g["nchunk"], g["W"]) == LDS_TABLE[shape], (shape, g)
        # the chunks cover the chain, none is empty, and k_stats reads rows four at a time
        assert g["chunk_len"] % 4 == 0 and (g["nchunk"] - 1) * g["chunk_len"] < T <= g["nchunk"] * g["chunk_len"], (shape, g)
        assert g["big"] == (max(shape[2:]) > 64)


def test_pca_geometry_reproduces_the_recorded_table(driver):
    shapes = list(PCA_TABLE)
    out = driver([["pca", N, d, q, PCA_NCU] for (N, d, q) in shapes])
    for (N, d, q), line in zip(shapes, out):
        DP, QP, DT, QT, nchunk, rows, nchunkB, rowsB, sweep = _ints(line)
        want = PCA_TABLE[(N, d, q)]
        assert (nchunk, SWEEP_NAMES[sweep]) == (want[0], want[2]), ((N, d, q), line)
        assert want[1] is None or nchunkB == want[1], ((N, d, q), line)
        assert (DP, QP, DT, QT) == ((d + 15) // 16 * 16, (q + 15) // 16 * 16, (d + 15) // 16, (q + 15) // 16)


def test_pca_partitions_cover_the_rows_in_tiles_of_sixteen(driver):
    rng = np.random.default_rng(5)
    cases = [(int(10 ** rng.uniform(0, 6.3)), int(rng.integers(1, 257)), int(rng.integers(1, 33)), int(rng.choice([0, 1, 8, 104, 256, 304])))
             for _ in range(2000)]
    cases += [(N, d, q, PCA_NCU) for (N, d, q) in PCA_TABLE]
    for (N, d, q, ncu), line in zip(cases, driver([["pca"] + list(c) for c in cases])):
        DP, QP, DT, QT, nchunk, rows, nchunkB, rowsB, sweep = _ints(line)
        for nc, r in ((nchunk, rows), (nchunkB, rowsB)):
            assert nc >= 1 and r % 16 == 0 and (nc - 1) * r < N <= nc * r, ((N, d, q, ncu), line)
        assert nchunkB <= nchunk and nchunkB <= max(ncu, 1)
        assert SWEEP_NAMES[sweep] == ("pairs" if DT >= 13 and N >= 512 * max(ncu, 1) else "columns")
        if DT >= 13 and ncu > 0:
            assert nchunk <= ncu


# ---- properties ---------------------------------------------------------------------------------------------------------------
def _random_shapes(n, seed):
    rng = np.random.default_rng(seed)
    return [(int(10 ** rng.uniform(0, 3.3)), int(10 ** rng.uniform(np.log10(2), 3.5)), int(rng.integers(1, 129)), int(rng.integers(1, 129)),
             int(rng.choice([DIAGONAL_GAMMA, 1, WISHART]))) for _ in range(n)]


def test_the_cut_of_the_time_axis(driver):
    """W * part_len >= T - 2; parts are multiples of 16 where the axis is split; live_parts counts the parts whose first interior
    node, w * part_len, lies inside a chain of TL nodes."""
    rng = np.random.default_rng(11)
    cmds = []
    for T in sorted(set([2, 3, 18, 19, 33, 34, 35, 50, 51, 66, 129, 130] + [int(10 ** rng.uniform(0.4, 4.1)) for _ in range(300)])):
        for W in _admitted(T):
            Lw = ((T - 2 + W - 1) // W + 15) // 16 * 16 if W > 1 else T - 2
            TLs = sorted(set(min(max(x, 2), T) for x in [2, 3, T - 1, T, int(rng.integers(2, T + 1))] + [w * Lw + 2 + e for w in range(1, W + 1) for e in (-1, 0, 1)][:24]))
            cmds.append(["parts", T, W] + TLs)
    assert len(cmds) > 5000
    for c, line in zip(cmds, driver(cmds)):
        T, W, TLs = c[1], c[2], c[3:]
        (Lw, split), live = (_ints(x) for x in line.split("|"))
        assert W * Lw >= T - 2, c
        if W > 1:
            assert Lw == split and Lw % 16 == 0 and W * (Lw - 16) < T - 2, c      # (a smaller multiple of 16 would not cover the interior)
        else:
            assert Lw == T - 2
        assert live == [sum(1 for w in range(W) if w * Lw < TL - 2) for TL in TLs], c


def test_parts_without_nodes(driver):
    """T = 51 .. 55 in three parts: 49 .. 53 interior nodes in parts of 32, and the third part holds none."""
    for T, line in zip(range(51, 56), driver([["parts", T, 3, T] for T in range(51, 56)])):
        assert line == "32 32|2", (T, line)
    assert [_ints(x.split("|")[1]) for x in driver([["parts", 100, 3, 100, 99, 98, 51, 50, 3, 2]])] == [[3, 3, 2, 2, 1, 1, 0]]    # parts of 48


def test_every_extent_for_every_admitted_time_split(driver):
    shapes = _random_shapes(1500, 21) + [(N, T, D, K, kind) for (N, T, D, K) in LDS_TABLE for kind in (DIAGONAL_GAMMA, WISHART)]
    base = driver([["lds"] + list(s) for s in shapes])
    cmds, want = [], []
    for s, line in zip(shapes, base):
        N, T, D, K, kind = s
        g, ext = _lds(line)
        assert g["big"] == (D > 64 or K > 64) and g["dense"] == (kind == WISHART)
        assert g["chunk_len"] % 4 == 0 and (g["nchunk"] - 1) * g["chunk_len"] < T <= g["nchunk"] * g["chunk_len"] and g["nchunk"] <= 32
        assert g["W"] in _admitted(T) and (g["W"] == 1 or (T - 2) // g["W"] >= 64), (s, g)      # its own choice leaves parts of 64 nodes
        assert ext == _extents(N, T, D, K, g["dense"], g["nchunk"], g["W"]), (s, g)
        for W in _admitted(T):
            cmds.append(["split"] + list(s) + [W])
            want.append((dict(g, W=W), _extents(N, T, D, K, g["dense"], g["nchunk"], W)))
    assert len(cmds) > 20000
    for c, line, w in zip(cmds, driver(cmds), want):
        assert _lds(line) == w, c


def test_the_default_time_split_is_the_cost_model_s(driver):
    """W minimises rounds x steps -- 1024 resident wavefronts (256 workgroups in the 128-wide class), ceil(part / 16) + 32 steps --
    over the splits that leave parts of at least 64 nodes, and a larger W has to be 3 % better."""
    shapes = _random_shapes(1500, 31)
    for (N, T, D, K, kind), line in zip(shapes, driver([["lds"] + list(s) for s in shapes])):
        slots = 256 if max(D, K) > 64 else 1024
        best, W = 1e300, 1
        for w in range(1, 129):
            if w > 1 and (T - 2) // w < 64:
                break
            part = ((T - 2 + w - 1) // w + 15) // 16 * 16
            cost = float((N * w + slots - 1) // slots) * float((part + 15) // 16 + 32)
            if cost < best * 0.97:
                best, W = cost, w
        assert _lds(line)[0]["W"] == W, (N, T, D, K)


def test_layout_offsets_are_disjoint_and_end_at_the_totals(driver):
    cases = [(D, K) for D in (1, 6, 16, 17, 32, 33, 64, 65, 100, 128) for K in (1, 4, 16, 17, 33, 64, 70, 128)]
    for (D, K), line in zip(cases, driver([["layout", D, K] for D, K in cases])):
        dims, gains, stats = (_ints(x) for x in line.split("|"))
        d, k, DT, KT, DP, KP, DS, KS, QR = dims
        big = max(D, K) > 64
        assert (d, k) == (D, K) and (DT, KT) == ((8, 8) if big else (_tiles(D), _tiles(K)))
        assert (DP, KP, DS, KS, QR) == (16 * DT, 16 * KT, 4 * DT, 4 * KT, 128 if big else 64)
        sizes = [DT * DS * 64, DT * DS * 64, DT * KS * 64, DP * DP, DP * DP, 2 * QR, DP]      # Fn, Bn, Gp, S0, S2, qr, w0
        assert gains[0] == 0 and all(gains[i] + sizes[i] == gains[i + 1] for i in range(7)), line
        assert stats[0] == 0 and [stats[i + 1] - stats[i] for i in range(3)] == [DP * DP, DP * DP, KP * DP], line


def test_positions_are_bijections(driver):
    for n, line in zip((16, 32, 64, 128), driver([["xpos", n] for n in (16, 32, 64, 128)])):
        p = np.array(_ints(line))
        assert sorted(p) == list(range(n)) and np.all(p // 16 == np.arange(n) // 16)
        d = np.arange(n)
        assert np.array_equal(p, (d & ~15) | ((d & 3) << 2) | ((d >> 2) & 3))
    cases = [(kind, 16 * MT, 4 * S, S) for kind in ("nat", "perm") for MT in (1, 2, 4, 8) for S in (4, 8, 16, 32)]
    for (kind, R, C, S), line in zip(cases, driver([list(c) for c in cases])):
        assert sorted(_ints(line)) == list(range(R * C)), (kind, R, C, S)
    for rows, line in zip((1, 8, 9, 16, 64, 70, 128), driver([["cov", r] for r in (1, 8, 9, 16, 64, 70, 128)])):
        RT = (rows + 7) // 8
        assert _ints(line) == [RT * (RT + 1) // 2, RT * (RT + 1) // 2 * 64]


# ---- refusals -----------------------------------------------------------------------------------------------------------------
def test_check_time_split_messages(driver):
    out = driver([["check", 100, 0], ["check", 5000, 129], ["check", 40, 3], ["check", 40, 2], ["check", 2, 1], ["check", 2050, 128], ["check", 51, 3]])
    assert out == ["%d|W must be in 1..128" % E_ARG, "%d|W must be in 1..128" % E_ARG, "%d|parts of fewer than 16 nodes" % E_ARG,
                   "%d|" % OK, "%d|" % OK, "%d|" % OK, "%d|" % OK]
