"""CPU-only: the host half of the generic path (pyvb_amd/csrc/tape_plan.h) needs no device.  tests/c/tape_plan_driver.cpp
is built here with the address and undefined-behaviour sanitizers (runtimes linked statically, so that a preloaded library
cannot upset their start-up) and run on the tapes of tests/tape_cases.py:

* the plan -- windows, segments, resolved and bundled records -- replayed in numpy with oracle/tape_ref.py leaves BITWISE the
  arena that the records leave in tape order (independent records commute exactly, so there is no tolerance);
* the structural promises of the plan, checked against an extent table written out here from the record layouts;
* which single records are accepted, against verdicts worked out by hand (tests/test_generic_gpu.py confirms the same list
  on pyvb_graph_tape_create);
* the entries of the built library refuse bad arguments before any HIP call.
"""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import tape_cases as TC  # noqa: E402
from oracle import tape_ref as R  # noqa: E402

SAN = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan"]
OFFSET_FIELDS = [1, 2, 3, 6, 7]


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("tape_plan")
    probe = tmp / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    if subprocess.run(SAN + [str(probe), "-o", str(tmp / "probe")], capture_output=True).returncode != 0:
        pytest.skip("this compiler cannot link the static sanitizer runtimes")
    exe = tmp / "tape_plan_driver"
    subprocess.run(SAN + ["-Wall", "-I", os.path.join(REPO, "pyvb_amd", "csrc"), os.path.join(HERE, "c", "tape_plan_driver.cpp"), "-o", str(exe)],
                   check=True, capture_output=True)

    def run(arena_n, records, blocks=None, launches=None, plan=True):
        records = np.ascontiguousarray(records, dtype=np.int32).reshape(-1, 8)
        blocks = np.asarray([[0, len(records)]] if blocks is None else blocks, dtype=np.int32).reshape(-1, 2)
        launches = np.asarray([[0, 1]] if launches is None else launches, dtype=np.int32).reshape(-1, 2)
        with open(tmp / "in.bin", "wb") as f:
            f.write(np.int64(arena_n).tobytes())
            f.write(np.asarray([len(records), len(blocks), len(launches), int(plan)], dtype=np.int32).tobytes())
            f.write(records.tobytes()); f.write(blocks.tobytes()); f.write(launches.tobytes())
        p = subprocess.run([str(exe), str(tmp / "in.bin"), str(tmp / "out.bin")], capture_output=True, text=True)
        assert p.returncode == 0, "the sanitized planner failed:\n" + p.stderr[-4000:]
        buf = open(tmp / "out.bin", "rb").read()
        pos = [0]

        def take(dtype, n):
            a = np.frombuffer(buf, dtype=dtype, count=n, offset=pos[0])
            pos[0] += a.nbytes
            return a
        out = dict(valid=take(np.int32, len(records)).astype(bool), tiled=take(np.int64, 2))
        if plan:
            head = take(np.int64, 11)
            out.update(in_lds=bool(head[0]), stats=head[6:], cops=take(np.int32, head[1]).reshape(-1, 8), blocks=take(np.int32, head[2]).reshape(-1, 2),
                       windows=take(np.int32, 8 * head[3]).reshape(-1, 8), segs=take(np.int32, 4 * head[4]).reshape(-1, 4),
                       width=take(np.int32, head[5]), lds_bytes=take(np.int64, head[5]))
        assert pos[0] == len(buf)
        return out
    return run


def strip_lds(recs):
    """Resolved records -> plain records whose offsets are positions in the window."""
    recs = np.array(recs, dtype=np.int64)
    f = recs[:, OFFSET_FIELDS]
    recs[:, OFFSET_FIELDS] = np.where((f >= 0) & (f & TC.T_LDS != 0), f & ~TC.T_LDS, f)
    return recs


def replay(plan, arena, launches):
    """What k_tape_cached does with a plan, in numpy: per block its windows in order -- load the segments, run the records out of
    the window (the records of a bundle LAST FIRST: they are promised to be independent), write the written segments back.  The
    blocks of a launch last first, as oracle.tape_ref.NumpyExecutor runs them."""
    for (first, count), width in zip(np.asarray(launches).reshape(-1, 2), plan["width"]):
        for w0, nw in reversed(plan["blocks"][first:first + count].tolist()):
            for rec0, nrec, seg0, nseg, doubles, bundled, _, _ in plan["windows"][w0:w0 + nw].tolist():
                recs = plan["cops"][rec0:rec0 + nrec]
                if nseg == 0:
                    R.run(arena, recs)
                    continue
                segs = plan["segs"][seg0:seg0 + nseg]
                win = np.full(doubles, np.nan)
                for off, n, lds, _ in segs:
                    win[lds:lds + n] = arena[off:off + n]
                before = win.copy()
                recs = strip_lds(recs)
                if bundled:
                    assert nrec % width == 0
                    for b in range(0, nrec, width):
                        R.run(win, recs[b:b + width][::-1])
                else:
                    R.run(win, recs)
                for off, n, lds, written in segs:
                    if written:
                        arena[off:off + n] = win[lds:lds + n]
                    else:
                        np.testing.assert_array_equal(win[lds:lds + n], before[lds:lds + n], "a segment that is not written back was written")
    return arena


def check_structure(plan, raw, blocks, launches):
    """The promises of a plan, against TC.extents (the record layouts written out in Python)."""
    raw = np.asarray(raw, dtype=np.int64).reshape(-1, 8)
    widths = np.repeat(plan["width"], np.asarray(launches).reshape(-1, 2)[:, 1])
    assert len(plan["blocks"]) == len(blocks) == len(widths)
    for (first, count), (w0, nw), width in zip(np.asarray(blocks).reshape(-1, 2).tolist(), plan["blocks"].tolist(), widths):
        seen = []
        for rec0, nrec, seg0, nseg, doubles, bundled, _, _ in plan["windows"][w0:w0 + nw].tolist():
            recs = np.array(plan["cops"][rec0:rec0 + nrec], dtype=np.int64)
            if nseg == 0:
                plain = recs[(recs[:, 0] != R.T_GATHER) & (recs[:, 0] != R.T_SCATTER)][:, OFFSET_FIELDS]
                assert not bundled and not np.any((plain >= 0) & (plain & TC.T_LDS != 0)), "a record on the arena carries a window offset"
                seen += recs.tolist()
                continue
            assert doubles <= TC.TAPE_LDS_CAP and nseg <= TC.TAPE_MAX_SEGS
            segs = plan["segs"][seg0:seg0 + nseg]
            ends = segs[:, 0] + segs[:, 1]
            assert np.all(segs[:, 1] > 0) and np.all(segs[1:, 0] > ends[:-1]), "segments of a window overlap or touch"
            assert np.all(segs[1:, 2] >= segs[:-1, 2] + segs[:-1, 1]) and segs[0, 2] == 0 and segs[-1, 2] + segs[-1, 1] <= doubles
            # un-resolve every record through the segments and compare with what its extents ask for
            orig = recs.copy()
            for k, rec in enumerate(recs):
                assert rec[0] not in (R.T_GATHER, R.T_SCATTER), "a record whose addresses are data sits in an LDS window"
                for f in OFFSET_FIELDS:
                    if rec[f] >= 0 and rec[f] & TC.T_LDS:
                        pos = rec[f] & ~TC.T_LDS
                        s = np.searchsorted(segs[:, 2], pos, side="right") - 1
                        assert pos < segs[s, 2] + segs[s, 1]
                        orig[k, f] = segs[s, 0] + pos - segs[s, 2]
                for off, n, write in TC.extents(orig[k]):
                    if n:
                        s = np.searchsorted(segs[:, 0], off, side="right") - 1
                        assert s >= 0 and off + n <= ends[s], "an extent of a record is not inside one segment"
                        assert not write or segs[s, 3], "a segment that a record writes is not written back"
            if bundled:
                assert nrec % width == 0
                for b in range(0, nrec, width):
                    live = [r for r in orig[b:b + width] if r[0] != R.T_NOP]
                    assert live, "an empty bundle"
                    for i in range(len(live)):
                        for j in range(i):
                            assert not TC.hazard(live[i], live[j]), "two records of one bundle touch the same elements"
            seen += [r for r in orig.tolist() if bundled == 0 or r[0] != R.T_NOP]
        # every record of the block exactly once (records that are equal are interchangeable), T_NOP only as filler
        assert sorted(seen) == sorted(raw[first:first + count].tolist())
    assert plan["windows"][:, 1].sum() == len(plan["cops"])


def plan_and_check(driver, ops, arena, blocks=None, launches=None):
    blocks = [[0, len(ops)]] if blocks is None else blocks
    launches = [[0, 1]] if launches is None else launches
    plan = driver(arena.size, ops, blocks, launches)
    assert plan["valid"].all() and plan["tiled"].tolist() == [len(ops), len(blocks)]
    check_structure(plan, ops, blocks, launches)
    return plan


def test_bundled_plans_of_random_tapes_compute_bitwise_what_the_tape_order_computes(driver):
    dropped, bundled, lds = 0, 0, 0
    for case, ops, arena in TC.random_tapes():
        ref = arena.copy()
        R.run(ref, ops)
        if not np.all(np.isfinite(ref)) or np.abs(ref).max() > 1e100:
            dropped += 1
            continue
        plan = plan_and_check(driver, ops, arena)
        assert plan["in_lds"]
        bundled += int(plan["stats"][1]); lds += int(plan["stats"][0])
        np.testing.assert_array_equal(replay(plan, arena.copy(), [[0, 1]]), ref, "case %d" % case)
        if case == 11:
            assert plan["stats"][0] > 1, "the working set of the last case does not fit one window"
    assert dropped <= 3, "%d of the 12 random tapes have no finite reference" % dropped
    assert bundled > 0 and lds >= bundled


def test_plans_of_long_tapes_compute_bitwise_what_the_tape_order_computes(driver):
    tapes = TC.long_tapes()
    for name, (ops, arena, _) in sorted(tapes.items()):
        ref = arena.copy()
        R.run(ref, ops)
        assert np.all(np.isfinite(ref))
        plan = plan_and_check(driver, ops, arena)
        np.testing.assert_array_equal(replay(plan, arena.copy(), [[0, 1]]), ref, "tape (%s)" % name)
    a, b, c = [driver(tapes[k][1].size, tapes[k][0]) for k in "abc"]
    assert a["in_lds"] and a["windows"][:, 1].max() > 512                  # more records in a window than are staged at a time
    assert np.any(b["windows"][:, 3] == 0)                                  # the 80 x 80 products stay on the arena
    gather = [w for w in c["windows"] if np.any(c["cops"][w[0]:w[0] + w[1], 0] == R.T_GATHER)]
    assert gather and all(w[3] == 0 for w in gather)


def test_a_program_of_many_short_blocks_is_planned_four_wide_and_computes_bitwise_the_same(driver):
    ops, arena, blocks, launches = TC.many_short_blocks()
    assert launches[0, 1] >= 512
    plan = plan_and_check(driver, ops, arena, blocks, launches)
    assert plan["width"].tolist() == [4, TC.TAPE_BUNDLE] and plan["in_lds"]
    assert plan["stats"][1] > 0
    ref = arena.copy()
    for first, count in launches:                       # tape order: launch by launch, block by block
        for a, n in blocks[first:first + count]:
            R.run(ref, ops[a:a + n])
    assert np.all(np.isfinite(ref))
    np.testing.assert_array_equal(replay(plan, arena.copy(), launches), ref)


def test_an_arena_that_needs_bit_30_of_an_offset_is_not_planned(driver):
    ops = [[R.T_UNARY, 0, 8, 0, 2, 2, 0, 4]] * 4
    assert driver(64, ops)["in_lds"]
    big = driver(TC.T_LDS, ops)
    assert not big["in_lds"] and len(big["cops"]) == 0 and len(big["windows"]) == 0 and big["valid"].all()


def test_which_records_are_accepted(driver):
    out = driver(TC.VALIDATION_ARENA, [rec for rec, _ in TC.VALIDATION], plan=False)
    wrong = [(rec, ok) for (rec, ok), got in zip(TC.VALIDATION, out["valid"]) if bool(got) != ok]
    assert not wrong, "verdicts that differ from the list (record, expected): %r" % wrong


def test_tables_that_do_not_tile_are_told_apart(driver):
    ops = [[R.T_NOP, 0, 0, 0, 0, 0, 0, 0]] * 6
    for blocks, launches, expect in (([[0, 2], [2, 4]], [[0, 1], [1, 1]], [6, 2]), ([[0, 2], [3, 3]], [[0, 2]], [-1, 2]),
                                     ([[0, 2], [2, 0]], [[1, 1]], [-1, -1]), ([[0, 2], [2, 3]], [[0, 1], [1, 1], [2, 0]], [5, -1])):
        assert driver(64, ops, blocks, launches, plan=False)["tiled"].tolist() == expect


def test_the_graph_entries_refuse_bad_arguments_without_a_gpu():
    from pyvb_amd import _capi
    lib = _capi.lib
    one, h, x = ctypes.c_int(0), ctypes.c_void_p(), ctypes.c_double(0.0)
    ip, dp = ctypes.cast(ctypes.byref(one), _capi._ip), ctypes.cast(ctypes.byref(x), _capi.SIGNATURES["pyvb_graph_write"][1][2])
    for call, msg in ((lambda: lib.pyvb_graph_create(None, 0, 64), b"bad arguments (the arena is addressed with 32-bit offsets)"),
                      (lambda: lib.pyvb_graph_create(ctypes.byref(h), 0, 0), b"bad arguments (the arena is addressed with 32-bit offsets)"),
                      (lambda: lib.pyvb_graph_create(ctypes.byref(h), 0, 1 << 31), b"bad arguments (the arena is addressed with 32-bit offsets)"),
                      (lambda: lib.pyvb_graph_write(None, 0, dp, 1), b"write outside the arena"),
                      (lambda: lib.pyvb_graph_read(None, 0, dp, 1), b"read outside the arena"),
                      (lambda: lib.pyvb_graph_sync(None), b"handle is NULL"),
                      (lambda: lib.pyvb_graph_tape_create(None, ip, 1, ip), b"bad arguments"),
                      (lambda: lib.pyvb_graph_tape_set_program(None, 0, ip, 1, ip, 1), b"no such tape"),
                      (lambda: lib.pyvb_graph_tape_run(None, 0), b"no such tape"),
                      (lambda: lib.pyvb_graph_tape_destroy(None, 0), b"no such tape")):
        assert call() == _capi.E_ARG
        assert lib.pyvb_last_error() == msg
    assert lib.pyvb_graph_destroy(None) == _capi.OK
