"""Cases for the tape interpreter (pyvb_amd/csrc/k_tape.hip) that NAME THE EXECUTION FORM they run in, shared by
tests/test_tape_forms_cpu.py (which pins the form with the sanitized planner driver and measures the float64 reference) and
tests/test_tape_forms_gpu.py (which runs them on the device).

The interpreter is tape_exec<WIN, NT> in these forms; which one a record runs in follows from tape_plan.h alone:

    plain                 k_tape, arena, 256 threads: a tape of one record (a run shorter than 3 stays on the arena, so nothing
                          is uploaded)
    blocks                k_tape_blocks, arena, 256: a program whose blocks all have fewer than 3 records
    arena-in-cached-512   tape_exec<false, 512> inside k_tape_cached<8>: the record beside a T_GATHER, in a tape that has a window
                          elsewhere
    window-512            tape_exec<true, 512>: [T_NOP, record, T_NOP]; a record of at most 64 elements gets a companion of 65
                          elements on scratch, which keeps the window from being bundled
    bundled-8             tape_exec<true, 64>, a wavefront per record, bundles of 8: [T_NOP, record, T_NOP], at most 64 elements
    window-256, bundled-4 the same in a program whose one launch has 512 blocks on disjoint state (k_tape_cached<4>)

A CORE is one record on a local state (inputs separated by sentinel doubles, so that extents do not merge and odd lengths are
padded); case(core, form) lays it out for the form.  A case is (records, arena, program or None, outputs, form); outputs is an
Outputs tuple: the positions the records may write, the positions whose content is unspecified (scratch), and the geometry
(blocks, stride, period) the comparisons need.  In the 512-block forms every block has its own sentinels and the inputs of
block b are those of block b % PERIOD, so the references interpret PERIOD blocks and not 512."""
import collections

import numpy as np

import tape_cases as TC
from oracle import tape_ref as R
import extended_ref as E
import tape_xref as X

FORMS = ("plain", "blocks", "arena-in-cached-512", "window-512", "window-256", "bundled-8", "bundled-4")
NBLOCKS, PERIOD = 512, 4
SEED = 20260
Case = collections.namedtuple("Case", "records arena program outputs form")
Outputs = collections.namedtuple("Outputs", "written scratch nblocks stride period")
Core = collections.namedtuple("Core", "name rec state data")       # data: mask of the inputs (the rest becomes sentinels)
NOP = [R.T_NOP, 0, 0, 0, 0, 0, 0, 0]
EXTRA = 141         # per block after the core's state: companion source (65) and target (65), a 1 x 1 gather, sentinels between


class Loc(object):
    """The local state of a core: operands one after the other with `gap` sentinel doubles in between."""

    def __init__(self, gap=1):
        self.vals, self.mask, self.gap = [0.0] * gap, [False] * gap, gap

    def put(self, arr):
        a = np.asarray(arr, dtype=float).reshape(-1)
        off = len(self.vals)
        self.vals += a.tolist() + [0.0] * self.gap; self.mask += [True] * a.size + [False] * self.gap
        return off

    def hole(self, n):
        off = len(self.vals)
        self.vals += [0.0] * (n + self.gap); self.mask += [False] * (n + self.gap)
        return off

    def core(self, name, rec):
        return Core(name, [int(v) for v in rec], np.array(self.vals), np.array(self.mask, dtype=bool))


def sentinels(first, n):
    """Distinct, non-zero, exactly representable, and nothing an operation on the inputs produces."""
    return -(np.arange(first, first + n, dtype=float) + 1000.5)


def offset_fields(rec):
    op, b, fl = int(rec[0]), int(rec[3]), int(rec[7])
    return {R.T_NOP: [], R.T_COPY2D: [1, 2], R.T_FILL: [1], R.T_AXPBY: [1, 2, 6] + ([3, 7] if b >= 0 else []), R.T_GEMM: [1, 2, 3],
            R.T_SCALE: [1, 2, 3], R.T_TRACE: [1, 2], R.T_DIAG: [1, 2], R.T_CHOLINV: [1, 2, 3, 6], R.T_DOT: [1, 2, 3], R.T_UNARY: [1, 2],
            R.T_GATHER: [1, 2, 3, 7], R.T_SCATTER: [1, 2, 3, 7], R.T_MUL: [1, 2, 3]}[op]


def shift(rec, by):
    rec = [int(v) for v in rec]
    for f in offset_fields(rec):
        rec[f] += by            # (T_ACC in field 7 of a scatter survives: the offsets stay far below bit 30)
    return rec


def elements(rec):
    """What tape_resolve takes for the size of a record: at most 64 everywhere in a window, and the window is bundled."""
    op, m, n = int(rec[0]), int(rec[4]), int(rec[5])
    return m * m if op in (R.T_CHOLINV, R.T_DIAG, R.T_TRACE) else m * n


def lds_doubles(rec):
    ext = TC.extents(rec)
    return None if ext is None else sum((n + 1) & ~1 for _, n, _ in ext)


def forms_of(core):
    """The forms that admit the record: no window for records whose addresses are data or whose extents exceed the LDS budget
    (those run on the arena whatever surrounds them), no bundle above 64 elements."""
    need = lds_doubles(core.rec)
    out = ["plain", "blocks", "arena-in-cached-512"]
    if need is not None and need + 132 <= TC.TAPE_LDS_CAP:
        out += ["window-512", "window-256"]
        if elements(core.rec) <= 64:
            out += ["bundled-8", "bundled-4"]
    return out


def written_positions(rec, arena):
    """(positions the record may write, positions it leaves unspecified) on `arena` as uploaded."""
    op, d, a, b, m, n, p, fl = [int(v) for v in rec]
    if op in (R.T_COPY2D, R.T_FILL):
        return (d + b * np.arange(m)[:, None] + np.arange(n)[None, :]).reshape(-1), np.zeros(0, dtype=int)
    if op == R.T_GATHER:
        return d + np.arange(m * n), np.zeros(0, dtype=int)
    if op == R.T_SCATTER:
        co = fl & ~X.T_ACC
        pos = (d + arena[b:b + m].astype(np.int64)[:, None] * p + arena[co:co + n].astype(np.int64)[None, :]).reshape(-1)
        return pos[(pos >= 0) & (pos < arena.size)], np.zeros(0, dtype=int)
    if op == R.T_CHOLINV:
        return np.concatenate([d + np.arange(m * m), b + np.arange(2)]), p + np.arange(2 * m * m)
    w = [o + np.arange(k) for o, k, wr in TC.extents(rec) if wr and k]
    return (np.concatenate(w) if w else np.zeros(0, dtype=int)), np.zeros(0, dtype=int)


def case(core, form):
    assert form in forms_of(core), (core.name, form)
    S = core.state.size
    stride = S + EXTRA
    nb = NBLOCKS if form in ("window-256", "bundled-4") else 1
    csrc, cdst, gdst, gsrc, grow, gcol = S, S + 66, S + 132, S + 134, S + 136, S + 138
    comp = [R.T_UNARY, cdst, csrc, 0, 65, 1, 0, X.U_NEG]
    gather = [R.T_GATHER, gdst, gsrc, grow, 1, 1, 1, gcol]
    if form == "plain":
        block, program = [core.rec], None
    elif form == "blocks":
        block, program = [core.rec, NOP], ([[0, 1], [1, 1]], [[0, 2]])
    elif form == "arena-in-cached-512":
        block, program = [core.rec, gather, NOP, comp, NOP], None
    else:
        block = [NOP, core.rec, NOP]
        if form.startswith("window") and elements(core.rec) <= 64:
            block.append(comp)
        program = ([[len(block) * b, len(block)] for b in range(nb)], [[0, nb]]) if nb > 1 else None
    arena = sentinels(0, nb * stride).reshape(nb, stride)
    rng = np.random.default_rng(SEED)
    local = np.zeros(stride); mask = np.zeros(stride, dtype=bool)
    local[:S], mask[:S] = core.state, core.data
    local[csrc:csrc + 65] = rng.uniform(0.5, 2.0, 65); mask[csrc:csrc + 65] = True
    local[gsrc], local[grow], local[gcol] = 2.5, 0.0, 0.0; mask[[gsrc, grow, gcol]] = True
    index = np.zeros(stride, dtype=bool)            # index vectors and the gather's operands are the same in every block
    index[[gsrc, grow, gcol]] = True
    if core.rec[0] in (R.T_GATHER, R.T_SCATTER):
        op, d, a, b, m, n, p, fl = core.rec
        index[b:b + m] = True; index[(fl & ~X.T_ACC):(fl & ~X.T_ACC) + n] = True
    arena[:, mask] = local[mask]
    vary = mask & ~index                # the other blocks of a period: the same inputs exactly scaled (same signs, same pattern)
    arena[:, vary] *= (1.0 + 0.125 * (np.arange(nb) % PERIOD))[:, None]
    fields = np.zeros((len(block), 8), dtype=np.int64)
    for k, r in enumerate(block):
        fields[k, offset_fields(r)] = 1         # (T_ACC in field 7 of a scatter survives: the offsets stay far below bit 30)
    records = (np.asarray(block, dtype=np.int64)[None] + fields[None] * (np.arange(nb) * stride)[:, None, None]).reshape(-1, 8).astype(np.int32)
    flat = arena.reshape(-1)
    w, s = [], []
    for r in block:
        wi, si = written_positions(r, flat)
        w.append(wi); s.append(si)
    out = Outputs(np.unique(np.concatenate(w)).astype(int), np.unique(np.concatenate(s)).astype(int), nb, stride, min(nb, PERIOD))
    return Case(records, flat, program, out, form)


def reference(c, runner, dtype=float):
    """The arena `runner` (oracle.tape_ref.run, tape_xref.run, a defective copy) leaves: the first `period` blocks interpreted,
    their written and scratch positions copied to the blocks with the same inputs.  Returns (arena, what the runner returned for
    each of the interpreted blocks).  A LinAlgStatus of the runner passes through."""
    o = c.outputs
    ref = c.arena.astype(dtype)
    recs = c.records.reshape(o.nblocks, -1, 8) if o.nblocks > 1 else c.records.reshape(1, -1, 8)
    got = [runner(ref, recs[b]) for b in range(o.period)] if o.nblocks > 1 else [runner(ref, c.records)]
    if o.nblocks > o.period:
        two = ref.reshape(o.nblocks, o.stride)
        pos = np.concatenate([o.written, o.scratch])
        two[o.period:, pos] = two[np.arange(o.period, o.nblocks) % o.period][:, pos]
    return ref, got


def errors(c, got, ext, units):
    """[(record, offset in its block, e, n)]: e = max |got - ext| / unit over the blocks that share the output's inputs."""
    o = c.outputs
    g2, e2 = np.asarray(got).reshape(o.nblocks, o.stride), ext.reshape(o.nblocks, o.stride)
    out = []
    for blk, per_block in enumerate(units):
        for rec, off, n, unit, acc in per_block:
            lo = off - blk * o.stride if o.nblocks > 1 else off
            rows = slice(blk, None, o.period) if o.nblocks > 1 else slice(0, 1)
            diff = np.abs(g2[rows, lo:lo + n].astype(E.LD) - e2[rows, lo:lo + n])
            with np.errstate(invalid="ignore", divide="ignore"):
                e = 0.0 if not n or not np.any(diff != 0) else float("inf") if np.isnan(diff).any() else float((diff / unit).max())
            out.append((rec, lo, e, acc))
    return out


# ----------------------------------------------------------------------------------------------------------------------------
# the cores, opcode by opcode
# ----------------------------------------------------------------------------------------------------------------------------
COUNTS = [(1, 1), (9, 7), (1, 64), (1, 65), (85, 3), (4, 64), (257, 1), (73, 7), (8, 64), (171, 3), (1025, 1)]
UNARY_NAMES = ["log", "digamma", "lgamma", "recip", "neg", "exp"]


def _rng(*key):
    return np.random.default_rng([SEED] + [int(k) for k in key])


def elementwise_cores():
    out = {}
    for i, (m, n) in enumerate(COUNTS):
        mn = m * n
        for v, kind in enumerate(("a", "ab", "dst=a", "dst=b")):
            g = _rng(1, i, v); L = Loc()
            a, b = L.put(g.uniform(-2, 2, mn)), L.put(g.uniform(-2, 2, mn))
            al, be = L.put([1.75]), L.put([-0.3])
            d = {"a": None, "ab": None, "dst=a": a, "dst=b": b}[kind]
            d = L.hole(mn) if d is None else d
            out.setdefault("axpby", []).append(L.core("axpby %s %dx%d" % (kind, m, n), [R.T_AXPBY, d, a, -1 if kind == "a" else b, m, n, al, be]))
        for v, name in enumerate(("scale_mul", "scale_div")):
            g = _rng(2, i, v); L = Loc()
            a, s, d = L.put(g.uniform(-2, 2, mn)), L.put([g.uniform(0.5, 3)]), L.hole(mn)
            out.setdefault(name, []).append(L.core("%s %dx%d" % (name, m, n), [R.T_SCALE, d, a, s, m, n, 0, v]))
        g = _rng(3, i); L = Loc()
        a, b, d = L.put(g.uniform(-2, 2, mn)), L.put(g.uniform(-2, 2, mn)), L.hole(mn)
        out.setdefault("mul", []).append(L.core("mul %dx%d" % (m, n), [R.T_MUL, d, a, b, m, n, 0, 0]))
        for f, name in enumerate(UNARY_NAMES):
            g = _rng(4, i, f); L = Loc()
            a, d = L.put(g.uniform(-3, 3, mn) if name in ("exp", "neg") else g.uniform(0.5, 3, mn)), L.hole(mn)
            out.setdefault(name, []).append(L.core("%s %dx%d" % (name, m, n), [R.T_UNARY, d, a, 0, m, n, 0, f]))
    grid = E.special_grid()
    for f, name in enumerate(UNARY_NAMES):      # the arguments the bounds give the special functions, in each function's domain
        x = {"log": np.abs(grid), "exp": grid[np.abs(grid) < 500]}.get(name, grid)
        L = Loc()
        a, d = L.put(x), L.hole(x.size)
        out[name].append(L.core("%s on the special grid" % name, [R.T_UNARY, d, a, 0, x.size, 1, 0, f]))
    return out


def copy_fill_cores():
    out = {"copy2d": [], "fill": []}
    for i, (m, n) in enumerate([(1, 1), (1, 5), (5, 1), (7, 3), (9, 8), (33, 2)]):
        g = _rng(5, i)
        ld_d, ld_s = n + 2, n + 3
        L = Loc()
        src = L.put(g.uniform(-2, 2, (m - 1) * ld_s + n)); dst = L.hole((m - 1) * ld_d + n)
        c = L.core("copy2d %dx%d ld %d <- %d" % (m, n, ld_d, ld_s), [R.T_COPY2D, dst, src, ld_d, m, n, ld_s, 0])
        c.data[src:src + (m - 1) * ld_s + n] = (np.arange((m - 1) * ld_s + n) % ld_s) < n       # the gaps of the source: sentinels
        out["copy2d"].append(c)
        for ident in (0, 1):
            L = Loc()
            dst = L.hole((m - 1) * ld_d + n)
            out["fill"].append(L.core("fill %dx%d ld %d identity %d" % (m, n, ld_d, ident), [R.T_FILL, dst, 0, ld_d, m, n, 0, ident]))
        L = Loc()           # contiguous
        src, dst = L.put(g.uniform(-2, 2, m * n)), L.hole(m * n)
        out["copy2d"].append(L.core("copy2d %dx%d contiguous" % (m, n), [R.T_COPY2D, dst, src, n, m, n, n, 0]))
    L = Loc()               # hstack: column i of a row-major rows x q matrix from a contiguous vector (generic.py, pass_down_Ex)
    src, dst = L.put(_rng(5, 99).uniform(-2, 2, 6)), L.hole(6 * 4)
    out["copy2d"].append(L.core("copy2d hstack column", [R.T_COPY2D, dst + 2, src, 4, 6, 1, 1, 0]))
    for m, n in ((3, 7), (7, 3)):       # identity with m != n, contiguous
        L = Loc()
        out["fill"].append(L.core("fill identity %dx%d" % (m, n), [R.T_FILL, L.hole(m * n), 0, n, m, n, 0, 1]))
    return out


GEMM_K = [0, 1, 3, 8, 9, 63, 64, 65, 71, 79, 200]
GEMM_MN = [(1, 1), (1, 5), (5, 1), (4, 8), (3, 11), (8, 16), (9, 15), (16, 16), (16, 17)]


def gemm_core(m, n, k, fl, key):
    g = _rng(6, *key); L = Loc()
    a, b = L.put(g.uniform(-1, 1, m * k)) if k else 0, L.put(g.uniform(-1, 1, k * n)) if k else 0
    d = L.put(g.uniform(-1, 1, m * n)) if fl & 4 else L.hole(m * n)
    return L.core("gemm %dx%d k %d flags %d" % (m, n, k, fl), [R.T_GEMM, d, a, b, m, n, k, fl])


def gemm_cores():
    """Every (k, (m, n)) pair with flags that run through all 16 combinations, and all 16 at four (k, shape) of their own."""
    out = [gemm_core(m, n, k, (5 * ik + 3 * imn) % 16, (ik, imn)) for ik, k in enumerate(GEMM_K) for imn, (m, n) in enumerate(GEMM_MN)]
    flags = []
    for j, (k, (m, n)) in enumerate(((0, (3, 11)), (9, (3, 11)), (64, (4, 8)), (71, (9, 15)))):
        flags += [gemm_core(m, n, k, fl, (100 + j, fl)) for fl in range(16)]
    return {"gemm": out, "gemm_flags": flags}


def reduce_cores():
    out = {"trace": [], "dot": []}
    for fl in (0, 4):
        for i, m in enumerate([1, 8, 9, 63, 64, 65, 100, 300]):
            g = _rng(7, i, fl); L = Loc()
            a = L.put(g.uniform(-2, 2, m * m)); d = L.put([0.625]) if fl else L.hole(1)
            out["trace"].append(L.core("trace m %d flags %d" % (m, fl), [R.T_TRACE, d, a, 0, m, m, 0, fl]))
        for i, (m, n) in enumerate([(1, 1), (1, 64), (5, 13), (257, 1), (171, 3), (8, 125)]):
            g = _rng(8, i, fl); L = Loc()
            a, b = L.put(g.uniform(-2, 2, m * n)), L.put(g.uniform(-2, 2, m * n)); d = L.put([0.625]) if fl else L.hole(1)
            out["dot"].append(L.core("dot %dx%d flags %d" % (m, n, fl), [R.T_DOT, d, a, b, m, n, 0, fl]))
    return out


def diag_cores():
    out = []
    for i, m in enumerate([1, 8, 9, 23]):
        g = _rng(9, i)
        L = Loc()
        a, d = L.put(g.uniform(-2, 2, m * m)), L.hole(m)
        out.append(L.core("diag of a matrix m %d" % m, [R.T_DIAG, d, a, 0, m, 0, 0, 0]))
        L = Loc()
        a, d = L.put(g.uniform(-2, 2, m)), L.hole(m * m)
        out.append(L.core("diagonal matrix m %d" % m, [R.T_DIAG, d, a, 0, m, 0, 0, 1]))
    return {"diag": out}


CHOL_M = [1, 2, 8, 9, 33, 55, 56, 70]


def chol_matrix(m, key):
    """G G^T + m I; times 16 for m <= 2, where sum log diag L would otherwise be near 0 and the quirk 0.5 / s near its pole."""
    G = _rng(10, *key).standard_normal((m, m))
    M = G @ G.T
    return ((M + M.T) / 2 + m * np.eye(m)) * (16.0 if m <= 2 else 1.0)       # the two triangles bitwise the same


def chol_core(name, M):
    m = M.shape[0]
    L = Loc()
    a, d, b, s = L.put(M), L.hole(m * m), L.hole(2), L.hole(2 * m * m)
    return L.core(name, [R.T_CHOLINV, d, a, b, m, 0, s, 0])


def cholinv_cores():
    out = []
    for i, m in enumerate(CHOL_M):
        M = chol_matrix(m, (i,))
        out.append(chol_core("cholinv m %d" % m, M))
        if m > 1:
            N = M.copy(); N[np.triu_indices(m, 1)] = np.nan         # the kernel reads the lower triangle only
            out.append(chol_core("cholinv m %d, NaN above the diagonal" % m, N))
    # one ill-conditioned matrix: eigenvalues 1 .. 1e6 on a random orthogonal basis; NumPy's own inverse is 9.0e-12 from the
    # extended one in units of max |inverse| here, under extended_ref.CAP
    Q, _ = np.linalg.qr(_rng(10, 77).standard_normal((33, 33)))
    M = (Q * np.logspace(0, 6, 33)) @ Q.T
    out.append(chol_core("cholinv m 33, condition 1e6", (M + M.T) / 2))
    return {"cholinv": out}


def not_pd_cores():
    """Not positive definite at the first and at the last pivot; m = 8 (every form), 9 and 56 (no bundle / no window)."""
    out = []
    for i, m in enumerate([8, 9, 56]):
        for where in ("first", "last"):
            M = chol_matrix(m, (50 + i,))
            if where == "first":
                M[0, 0] = -1.0
            else:       # the last pivot is a_mm - |row of L|^2: lower a_mm to just under the row's share
                Lc = np.linalg.cholesky(M)
                M[-1, -1] = float(np.sum(Lc[-1, :-1] ** 2)) * (1.0 - 1e-6) if m > 1 else -1.0
            out.append(chol_core("not positive definite at the %s pivot, m %d" % (where, m), M))
    return out


def index_cores():
    out = {"gather": [], "scatter": [], "scatter_acc": []}
    for i, (m, n) in enumerate([(m, n) for m in (1, 3, 65) for n in (1, 3, 65)]):
        g = _rng(11, i)
        rows, cols, p = 70, 70, 75                  # a 70 x 70 block with leading dimension 75: p larger than the block
        L = Loc()
        src = L.put(g.uniform(-2, 2, rows * p))
        r = L.put(g.integers(0, rows, m)); c = L.put(g.integers(0, cols, n))        # repeated indices
        d = L.hole(m * n)
        out["gather"].append(L.core("gather %dx%d" % (m, n), [R.T_GATHER, d, src, r, m, n, p, c]))
        for acc, name in ((0, "scatter"), (X.T_ACC, "scatter_acc")):
            L = Loc()
            a = L.put(g.uniform(-2, 2, m * n))
            r = L.put(g.permutation(rows)[:m]); c = L.put(g.permutation(cols)[:n])      # distinct pairs
            d = L.put(g.uniform(-2, 2, rows * p)) if acc else L.hole(rows * p)
            out[name].append(L.core("%s %dx%d" % (name, m, n), [R.T_SCATTER, d, a, r, m, n, p, c | acc]))
    return out


@E.functools.lru_cache(maxsize=None)
def cores():
    """{opcode name: [Core]}"""
    out = {}
    for part in (elementwise_cores(), copy_fill_cores(), gemm_cores(), reduce_cores(), diag_cores(), cholinv_cores(), index_cores()):
        out.update(part)
    return out


def opcode_forms():
    """(opcode name, form) for every form that admits at least one core of the opcode: the parameters of the tests."""
    return [(name, form) for name, cs in sorted(cores().items()) for form in FORMS if any(form in forms_of(c) for c in cs)]


def cases(name, form):
    return [(c.name, case(c, form)) for c in cores()[name] if form in forms_of(c)]


# ----------------------------------------------------------------------------------------------------------------------------
# windows: tapes of exact records whose plan is the point.  {name: (Case, what the plan must look like)}
# ----------------------------------------------------------------------------------------------------------------------------
def _tape(recs, size, fill, form):
    arena = sentinels(0, size)
    for off, arr in fill:
        arena[off:off + len(arr)] = arr
    recs = np.asarray(recs, dtype=np.int32)
    w, s = zip(*[written_positions(r, arena) for r in recs])
    return Case(recs, arena, None, Outputs(np.unique(np.concatenate(w)).astype(int), np.zeros(0, dtype=int), 1, size, 1), form)


def window_cases():
    g = _rng(12)
    out = {}
    neg = lambda d, a, n: [R.T_UNARY, d, a, 0, n, 1, 0, X.U_NEG]
    for n in (63, 64, 65):          # segments on both sides of the loader's split: the source read-only, the target written
        out["segments of %d" % n] = (_tape([NOP, neg(200, 10, n), NOP, neg(600, 400, 65)], 800, [(10, g.uniform(1, 2, n)), (400, g.uniform(1, 2, 65))],
                                           "window-512"), dict(nseg=4, seglen=[n, n, 65, 65]))
    # adjacent extents merge: source 10 .. 42, target 43 .. 75 -> one written segment of 66
    out["adjacent extents"] = (_tape([NOP, neg(43, 10, 33), NOP], 100, [(10, g.uniform(1, 2, 33))], "bundled-8"), dict(nseg=1, seglen=[66]))
    cap = TC.TAPE_LDS_CAP
    for extra in (0, 1):            # one window of exactly TAPE_LDS_CAP doubles; one double more and the records stay on the arena
        n = cap // 2 + extra
        out["window of the cap + %d" % extra] = (_tape([NOP, neg(20000, 10, n), NOP], 30000, [(10, g.uniform(1, 2, n))], "plain" if extra else "window-512"),
                                                 dict(in_lds=False) if extra else dict(nseg=2, seglen=[n, n], doubles=cap))
    # 513 independent records in one bundled window: one past TAPE_CHUNK
    recs = [neg(3000 + 3 * k, 10 + 3 * k, 2) for k in range(513)]
    out["513 bundled records"] = (_tape(recs, 5000, [(10, g.uniform(1, 2, 3 * 513))], "bundled-8"), dict(bundled=1, min_count=513))
    # a written strided copy inside a window: the gaps of its span are loaded and written back as they were
    out["strided copy in a window"] = (_tape([NOP, [R.T_COPY2D, 300, 10, 9, 13, 5, 7, 0], NOP, neg(700, 500, 65)], 900,
                                             [(10, g.uniform(1, 2, 12 * 7 + 5)), (500, g.uniform(1, 2, 65))], "window-512"), dict(nseg=4))
    return out


# ----------------------------------------------------------------------------------------------------------------------------
# the comparison: what tests/test_tape_forms_gpu.py asks of the device and tests/test_tape_forms_cpu.py of defective interpreters
# ----------------------------------------------------------------------------------------------------------------------------
def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


def everywhere(c, pos):
    o = c.outputs
    return (np.arange(o.nblocks)[:, None] * o.stride + np.asarray(pos, dtype=int)[None, :]).reshape(-1) if o.nblocks > 1 else np.asarray(pos, dtype=int)


def judge(c, got):
    """`got`: the arena an interpreter left for case c.  Rule 1: every double outside the written extents (and the scratch of a
    T_CHOLINV) is bitwise what was uploaded, and what the exact records wrote is bitwise what oracle/tape_ref.py writes.  Rule 2:
    every output of an arithmetic record has e_gpu <= FACTOR max(e64, n 2^-52) in the unit of tests/tape_xref.py.
    Returns dict(problems [str], e64, e_gpu, ratio = max e_gpu / max(e64, n 2^-52), same64: arithmetic outputs bitwise NumPy's)."""
    o = c.outputs
    got = np.asarray(got, dtype=float)
    ref64, _ = reference(c, R.run)
    ext, units = reference(c, X.run, E.LD)
    problems = []
    touched = np.zeros(c.arena.size, dtype=bool)
    touched[everywhere(c, np.concatenate([o.written, o.scratch]))] = True
    if not np.array_equal(_bits(got[~touched]), _bits(c.arena[~touched])):
        problems.append("%d doubles outside the written extents changed" % int(np.sum(_bits(got[~touched]) != _bits(c.arena[~touched]))))
    arith = np.zeros(c.arena.size, dtype=bool)
    for blk, per_block in enumerate(units):
        for rec, off, n, unit, acc in per_block:
            lo = off - blk * o.stride if o.nblocks > 1 else off
            arith[everywhere(c, lo + np.arange(n))[blk::1] if o.nblocks == 1 else (np.arange(blk, o.nblocks, o.period)[:, None] * o.stride + lo + np.arange(n)[None, :]).reshape(-1)] = True
    exact = np.zeros(c.arena.size, dtype=bool)
    exact[everywhere(c, o.written)] = True
    exact &= ~arith
    if not np.array_equal(_bits(got[exact]), _bits(ref64[exact])):
        problems.append("%d doubles of exact records differ from the NumPy interpreter" % int(np.sum(_bits(got[exact]) != _bits(ref64[exact]))))
    e64, eg, ratio = 0.0, 0.0, 0.0
    for (rec, lo, a, n), (_, _, g, _) in zip(errors(c, ref64, ext, units), errors(c, got, ext, units)):
        y = E.yardstick(a, n)
        e64, eg, ratio = max(e64, a), max(eg, g), max(ratio, g / y if g else 0.0)
        if not g <= E.FACTOR * y:
            problems.append("record %d at +%d: e_gpu %.3e > %g max(e64 %.3e, %d 2^-52)" % (rec, lo, g, E.FACTOR, a, n))
    return dict(problems=problems, e64=e64, e_gpu=eg, ratio=ratio, same64=bool(np.array_equal(_bits(got[arith]), _bits(ref64[arith]))))
