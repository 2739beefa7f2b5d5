"""The tape interpreter on the device (pyvb_amd/csrc/k_tape.hip), every opcode in every execution form, at its accuracy.

The cases and their forms are those of tests/tape_forms.py; tests/test_tape_forms_cpu.py pins each case's plan to the form it
declares, with the header the library plans with.  Two rules (tape_forms.judge):

1. every double outside the written extents of a case is bitwise what was uploaded (the arena is full of distinct sentinels),
   and what the exact records write -- data movement, one IEEE multiplication -- is bitwise what oracle/tape_ref.py writes;
2. every output of an arithmetic record obeys e_gpu <= FACTOR max(e64, n 2^-52) against the extended-precision interpreter
   (tests/tape_xref.py), in the unit and with the n listed there; FACTOR and CAP are extended_ref's.

Every test prints e64, e_gpu and e_gpu / max(e64, n 2^-52) case by case before it asserts; profiles/tape_envelope.txt is that
output.  T_SCALE divide and U_RECIP measured 0 against NumPy in every case and form when they were still under rule 2 (one
IEEE division each), so they are under rule 1; the column `=np` says where the arithmetic outputs of the other records happen
to be bitwise NumPy's as well."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import extended_ref as E  # noqa: E402
import tape_cases as TC  # noqa: E402
import tape_forms as F  # noqa: E402
import tape_xref as X  # noqa: E402
from oracle import tape_ref as R  # noqa: E402


def on_device(c, sync_error=None):
    """The arena the device leaves for case c.  sync_error: the exception the first sync after the run must raise."""
    from pyvb_amd import generic as G
    ex = G.DeviceExecutor(c.arena.size)
    try:
        ex.write(0, c.arena)
        tid = ex.tape(c.records, program=c.program)
        ex.run(tid)
        if sync_error is not None:
            with pytest.raises(sync_error):
                ex.sync()
        return ex.read(0, c.arena.size)
    finally:
        ex.close()


@pytest.mark.parametrize("name,form", F.opcode_forms())
def test_opcode_in_form(name, form):
    problems = []
    print()
    for label, c in F.cases(name, form):
        j = F.judge(c, on_device(c))
        print("%-12s %-20s %-44s e64 %.3e  e_gpu %.3e  ratio %6.3f  =np %d" % (name, form, label, j["e64"], j["e_gpu"], j["ratio"], j["same64"]))
        assert j["e64"] <= E.CAP
        problems += ["%s: %s" % (label, p) for p in j["problems"]]
    assert not problems, "\n".join(problems)


IEEE_POINTS = [("log", [0.0, -1.0, 1.0, np.inf]), ("recip", [0.0, -0.0, 2.0, np.inf]), ("exp", [710.0, -800.0, 0.0, -np.inf]), ("lgamma", [0.0, 1.0, 2.0])]


@pytest.mark.parametrize("form", F.FORMS)
def test_unary_functions_at_the_ieee_points(form):
    """log 0 = -inf, log -1 = NaN, 1 / 0 = inf, exp 710 = inf, lgamma 0 = inf: what NumPy / SciPy give, in each form."""
    for fname, pts in IEEE_POINTS:
        L = F.Loc()
        a, d = L.put(pts), L.hole(len(pts))
        c = F.case(L.core(fname, [R.T_UNARY, d, a, 0, len(pts), 1, 0, F.UNARY_NAMES.index(fname)]), form)
        ref, _ = F.reference(c, R.run)
        got = on_device(c)
        print("%-8s %-20s device %r  numpy %r" % (fname, form, got[d:d + len(pts)].tolist(), ref[d:d + len(pts)].tolist()))
        out = F.everywhere(c, c.outputs.written)
        special = ~np.isfinite(ref[out])
        assert special.any()
        np.testing.assert_array_equal(got[out][special], ref[out][special])
        np.testing.assert_allclose(got[out], ref[out], rtol=1e-15, atol=1e-15)
        keep = np.ones(c.arena.size, dtype=bool); keep[out] = False
        np.testing.assert_array_equal(got[keep], c.arena[keep])


@pytest.mark.parametrize("core", F.not_pd_cores(), ids=lambda c: c.name.replace(" ", "_"))
def test_a_matrix_that_is_not_positive_definite(core):
    """PYVB_E_LINALG at the next sync, whichever pivot fails, and an arena unchanged outside dst, the two scalars and the scratch."""
    for form in F.forms_of(core):
        c = F.case(core, form)
        got = on_device(c, sync_error=np.linalg.LinAlgError)
        o = c.outputs
        keep = np.ones(c.arena.size, dtype=bool); keep[F.everywhere(c, np.concatenate([o.written, o.scratch]))] = False
        same = np.array_equal(F._bits(got[keep]), F._bits(c.arena[keep]))
        print("%-60s %-20s outside unchanged %d" % (core.name, form, same))
        assert same, form
        if not np.any(c.records[:, 0] == R.T_UNARY):        # no companion record in this form
            continue
        comp = got.reshape(o.nblocks, o.stride)[:, core.state.size + 66:core.state.size + 131]
        assert np.all(comp > -3.0), "the records beside the failed one still ran"


def test_scatter_with_an_index_outside_the_arena():
    """Status bit 2 (PYVB_E_ARG at the next sync) and nothing written for that element, as for T_GATHER; arena and plain forms."""
    from pyvb_amd import _capi
    for form in ("plain", "blocks", "arena-in-cached-512"):
        for acc in (0, X.T_ACC):
            L = F.Loc()
            a = L.put([1.5, 2.5, 3.5, 4.5]); r = L.put([1.0, 1e9]); cidx = L.put([0.0, 2.0]); d = L.put(np.arange(16.0) + 0.25)
            c = F.case(L.core("scatter outside", [R.T_SCATTER, d, a, r, 2, 2, 4, cidx | acc]), form)
            got = on_device(c, sync_error=_capi.PyvbHipError)
            want = c.arena.copy()
            want[d + 4], want[d + 6] = (want[d + 4] + 1.5, want[d + 6] + 2.5) if acc else (1.5, 2.5)
            if form == "arena-in-cached-512":       # the gather and the companion beside the record ran as well
                S = c.arena.size - F.EXTRA
                want[S + 132], want[S + 66:S + 131] = 2.5, -c.arena[S:S + 65]
            np.testing.assert_array_equal(got, want, "%s, accumulate %d" % (form, bool(acc)))


def test_windows():
    """Segments on both sides of the loader's split, merged extents, a window of exactly the LDS budget and one double more,
    more bundled slots than are staged at a time, the gaps of a strided copy in a window: all exact records, bitwise."""
    for label, (c, _) in F.window_cases().items():
        j = F.judge(c, on_device(c))
        print("%-28s %-12s problems %r" % (label, c.form, j["problems"]))
        assert not j["problems"], label


def test_records_at_the_element_limit_are_accepted_and_refused():
    from pyvb_amd import _capi, generic as G
    ex = G.DeviceExecutor(TC.VALIDATION_BOUND_ARENA)
    for rec, ok in TC.VALIDATION_BOUND:
        if ok:
            ex.drop(ex.tape([rec]))
        else:
            with pytest.raises(_capi.PyvbHipError):
                ex.tape([rec])
    ex.close()


def test_the_largest_tall_records_the_limit_admits():
    """n = 3, m = 2^22 div 3, form plain: a strided T_COPY2D (ld = n + 1), an identity T_FILL and a T_GEMM with k = 1, bitwise
    against NumPy, the sentinel gaps of the strided targets included: the row and column of every element below the limit."""
    from pyvb_amd import generic as G
    n, ld = 3, 4
    m = TC.TAPE_MAX_ELEMS // n
    src, dst = 8, 8 + ld * m + 8
    size = dst + ld * m + 8
    rng = np.random.default_rng(F.SEED)
    arena = F.sentinels(0, size)
    rows = src + ld * np.arange(m)[:, None] + np.arange(n)[None, :]
    arena[rows] = rng.uniform(1.0, 2.0, (m, n))
    out_rows = rows - src + dst
    ex = G.DeviceExecutor(size)
    try:
        for name, rec in (("copy2d", [R.T_COPY2D, dst, src, ld, m, n, ld, 0]), ("fill", [R.T_FILL, dst, 0, ld, m, n, 0, 1]),
                          ("gemm", [R.T_GEMM, dst, src, src + m, m, n, 1, 0])):
            up = arena.copy()
            if name == "gemm":
                up[src:src + m + n] = rng.uniform(1.0, 2.0, m + n)          # a (m x 1), then b (1 x n); dst contiguous
            ex.write(0, up)
            ex.run(ex.tape([rec]))
            got = ex.read(0, size)
            want = up.copy()
            if name == "copy2d":
                want[out_rows] = up[rows]
            elif name == "fill":
                want[out_rows] = np.eye(m, n)
            else:
                want[dst:dst + m * n] = (up[src:src + m, None] * up[None, src + m:src + m + n]).reshape(-1)
            bad = int(np.sum(F._bits(got) != F._bits(want)))
            print("%-7s m %d n %d: %d of %d doubles differ" % (name, m, n, bad, size))
            assert bad == 0, name
    finally:
        ex.close()
