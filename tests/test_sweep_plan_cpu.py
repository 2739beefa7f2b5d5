"""CPU-only: the plan of a segmented sweep (pyvb_amd/csrc/sweep_plan.h) needs no device.  tests/c/sweep_plan_driver.cpp is built
here with the address and undefined-behaviour sanitizers (runtimes linked statically, as tests/test_geometry_cpu.py builds its
driver) and run directly.  Over a grid of chain lengths and warm-up lengths the plan must

* deal every interior node out to exactly one column,
* start a column at a seam (from zero at its own first node, made good by the correction loop) only in a forward sweep without
  time split, and only where the column and its left neighbour both own at least J nodes,
* correct exactly the first J nodes of those columns, for J steps,
* and in every other case be the warm-up rule as it was: jc = -min(J, before), the wave starting with its last column.
"""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
SAN = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan"]
BOUNDARY, SEAM, WARM = 0, 1, 2
LENGTHS = (3, 18, 34, 530, 546, 642, 10000)
WARMUPS = (4, 28, 32, 40)


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("sweep_plan")
    probe = tmp / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    if subprocess.run(SAN + [str(probe), "-o", str(tmp / "probe")], capture_output=True).returncode != 0:
        pytest.skip("this compiler cannot link the static sanitizer runtimes")
    exe = tmp / "sweep_plan_driver"
    subprocess.run(SAN + ["-Wall", "-I", os.path.join(REPO, "pyvb_amd", "csrc"), os.path.join(HERE, "c", "sweep_plan_driver.cpp"), "-o", str(exe)],
                   check=True, capture_output=True)

    def run(commands):
        (tmp / "in.txt").write_text("".join(" ".join(str(x) for x in c) + "\n" for c in commands))
        p = subprocess.run([str(exe), str(tmp / "in.txt"), str(tmp / "out.txt")], capture_output=True, text=True)
        assert p.returncode == 0, "the sanitized driver failed:\n" + p.stderr[-4000:]
        lines = (tmp / "out.txt").read_text().split("\n")[:-1]
        assert len(lines) == len(commands)
        return lines
    return run


def _plans(driver, cases):
    """cases: (TL, T, W, w, J, forward).  Returns per case (head, columns): head = Tint, ow, Tw, Lseg, first_step,
    correction_steps; columns = 16 x (before, count, jc, kind)."""
    out = []
    for line in driver([("plan",) + tuple(int(v) for v in c) for c in cases]):
        parts = [[int(x) for x in f.split()] for f in line.split("|")]
        assert len(parts) == 17
        out.append((parts[0], parts[1:]))
    return out


def _unsplit_cases():
    cases = []
    for T in LENGTHS:
        # the chain fills the handle, and ragged lengths below the stride T (down to the shortest chain there is)
        for TL in sorted({T, T - 1, T - 7, (T + 3) // 2, 16 * 32 + 2, 16 * 32 - 14, 3} & set(range(3, T + 1))):
            for J in WARMUPS:
                for fwd in (1, 0):
                    cases.append((TL, T, 1, 0, J, fwd))
    return cases


def test_unsplit_plan(driver):
    cases = _unsplit_cases()
    seen_seam = 0
    for (TL, T, W, w, J, fwd), (head, cols) in zip(cases, _plans(driver, cases)):
        Tint, ow, Tw, Lseg, first, ncorr = head
        tag = "TL %d T %d J %d fwd %d" % (TL, T, J, fwd)
        assert (Tint, ow, Tw) == (TL - 2, 0, TL - 2), tag
        assert Lseg == (Tw + 15) // 16, tag
        # every interior node is owned once: the columns' ranges tile 0 .. Tint-1 in order
        nxt = 0
        for c, (before, count, jc, kind) in enumerate(cols):
            assert before == c * Lseg and 0 <= count <= Lseg, tag
            if count:
                assert before == nxt, tag
                nxt = before + count
        assert nxt == Tint, tag
        seams = [c for c, s in enumerate(cols) if s[3] == SEAM]
        for c, (before, count, jc, kind) in enumerate(cols):
            legacy_jc = -min(J, before)
            if kind == BOUNDARY:
                assert before <= J and jc == -before == legacy_jc, tag
            elif kind == SEAM:
                # both length conditions, the direction, and not the first column; its left neighbour ends right before it
                assert fwd and c > 0 and before > J and count >= J and cols[c - 1][1] >= J and jc == 0, tag
                assert cols[c - 1][0] + cols[c - 1][1] == before, tag
            else:
                assert kind == WARM and before > J and jc == -J == legacy_jc, tag
                assert not (fwd and c > 0 and count >= J and cols[c - 1][1] >= J), tag      # nothing warms up that could take a seam
        assert first == min(s[2] for s in cols), tag
        if not seams:
            assert first == -min(J, 15 * Lseg) and ncorr == 0, tag       # the rule as it was
        else:
            # the correction runs J steps over exactly the first J nodes of the seam columns, all of which those columns own
            assert ncorr == J, tag
            corrected = set()
            for c in seams:
                rng = set(range(cols[c][0], cols[c][0] + ncorr))
                assert not (rng & corrected), tag
                corrected |= rng
            want = set()
            for c in seams:
                want |= set(range(cols[c][0], cols[c][0] + J))
                assert cols[c][0] + J <= cols[c][0] + cols[c][1] <= Tint, tag
            assert corrected == want, tag
        if not fwd:
            assert not seams, tag
        seen_seam += len(seams)
    assert seen_seam > 0


def test_headline_and_edges(driver):
    """The cases the kernel tests lean on: the headline has 15 seam columns and no warm-up step; a column length of exactly J is
    admitted (column 1 then reaches the boundary instead); one node less and every column warms up."""
    J = 32
    cases = [(10000, 10000, 1, 0, J, 1), (16 * (J + 8) + 2, 16 * (J + 8) + 2, 1, 0, J, 1), (16 * J + 2, 16 * J + 2, 1, 0, J, 1),
             (16 * J - 14, 16 * J - 14, 1, 0, J, 1), (20, 20, 1, 0, J, 1), (16 * J + 2, 16 * J + 2, 1, 0, J, 0)]
    p = _plans(driver, cases)
    kinds = [[s[3] for s in cols] for _, cols in p]
    assert kinds[0] == [BOUNDARY] + [SEAM] * 15 and p[0][0][3:] == [625, 0, J]
    assert kinds[1] == [BOUNDARY] + [SEAM] * 15 and p[1][0][3:] == [J + 8, 0, J]
    assert kinds[2] == [BOUNDARY, BOUNDARY] + [SEAM] * 14 and p[2][0][3:] == [J, -J, J]
    assert kinds[3] == [BOUNDARY, BOUNDARY] + [WARM] * 14 and p[3][0][3:] == [J - 1, -J, 0]
    assert kinds[4] == [BOUNDARY] * 16 and p[4][0][3:] == [2, -30, 0]
    assert kinds[5] == [BOUNDARY, BOUNDARY] + [WARM] * 14 and p[5][0][3:] == [J, -J, 0]


def test_active_matches_ownership(driver):
    """sweep_active at loop indices j >= 0 is the column's ownership; below 0 it is the warm-up, -jc steps where the column owns nodes."""
    cases = [(642, 642, 1, 0, 32, 1), (514, 530, 1, 0, 32, 1), (498, 498, 1, 0, 32, 1), (20, 34, 1, 0, 4, 1), (642, 642, 1, 0, 32, 0)]
    plans = _plans(driver, cases)
    cmds, keys = [], []
    for case, (head, cols) in zip(cases, plans):
        for c in range(16):
            cmds.append(("active",) + case + (c, -48, head[3] + 4))
            keys.append((head, cols[c]))
    for line, (head, (before, count, jc, kind)) in zip(driver(cmds), keys):
        js = [j for j, ch in zip(range(-48, head[3] + 4), line) if ch == "1"]
        assert [j for j in js if j >= 0] == list(range(count))
        if count:
            assert [j for j in js if j < 0] == list(range(jc, 0))


def test_split_never_takes_a_seam(driver):
    cases = []
    for T, W in ((642, 2), (10000, 4), (10000, 125), (2050, 8)):
        for TL in (T, T - 100, 40):
            for J in WARMUPS:
                for fwd in (1, 0):
                    for w in range(W):
                        cases.append((TL, T, W, w, J, fwd))
    owned = {}
    for (TL, T, W, w, J, fwd), (head, cols) in zip(cases, _plans(driver, cases)):
        Tint, ow, Tw, Lseg, first, ncorr = head
        Lw = (((T - 2 + W - 1) // W) + 15) & ~15
        assert ow == w * Lw and Tw == min(Lw, Tint - ow)
        assert ncorr == 0 and all(s[3] != SEAM for s in cols)
        if Tw > 0:
            assert all(s[2] == -min(J, s[0]) for s in cols) and first == -min(J, ow + 15 * Lseg)
        nodes = owned.setdefault((TL, T, W, J, fwd), [])
        for before, count, jc, kind in cols:
            nodes.extend(range(before, before + count))
    for (TL, T, W, J, fwd), nodes in owned.items():
        assert sorted(nodes) == list(range(TL - 2)), (TL, T, W)
