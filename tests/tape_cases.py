"""Tapes and single records shared by the CPU test of the host-only tape planner (tests/test_tape_plan_cpu.py, which
replays the planner's output in numpy) and the GPU tests of the interpreter (tests/test_generic_gpu.py): the same inputs
go through pyvb_amd/csrc/tape_plan.h under the host sanitizers and through the built library on the device."""
import numpy as np

from pyvb_amd import generic as G

T_ACC = 0x40000000
T_LDS = 0x40000000
TAPE_LDS_CAP, TAPE_MAX_SEGS, TAPE_BUNDLE = 12288, 4096, 8


def extents(rec):
    """[(offset, length, write)] of a record, written out from the record layouts (pyvb_amd/csrc/tape.h), zero lengths
    included; None for a record whose addresses are data (gather / scatter)."""
    op, d, a, b, m, n, p, fl = [int(v) for v in rec]
    span = lambda ld: (m - 1) * ld + n if m > 0 and n > 0 else 0
    mn, mm = m * n, m * m
    if op == G.T_NOP: return []
    if op == G.T_COPY2D: return [(d, span(b), True), (a, span(p), False)]
    if op == G.T_FILL: return [(d, span(b), True)]
    if op == G.T_AXPBY: return [(d, mn, True), (a, mn, False), (p, 1, False)] + ([(b, mn, False), (fl, 1, False)] if b >= 0 else [])
    if op == G.T_GEMM: return [(d, mn, True), (a, m * p, False), (b, p * n, False)]
    if op == G.T_SCALE: return [(d, mn, True), (a, mn, False), (b, 1, False)]
    if op == G.T_TRACE: return [(d, 1, True), (a, mm, False)]
    if op == G.T_DIAG: return [(d, mm, True), (a, m, False)] if fl & 1 else [(d, m, True), (a, mm, False)]
    if op == G.T_CHOLINV: return [(d, mm, True), (a, mm, False), (b, 2, True), (p, 2 * mm, True)]
    if op == G.T_DOT: return [(d, 1, True), (a, mn, False), (b, mn, False)]
    if op == G.T_UNARY: return [(d, mn, True), (a, mn, False)]
    if op == G.T_MUL: return [(d, mn, True), (a, mn, False), (b, mn, False)]
    assert op in (G.T_GATHER, G.T_SCATTER)
    return None


def hazard(x, y):
    """Two records touch a common element and at least one of them writes it."""
    return any((wa or wb) and la and lb and oa < ob + lb and ob < oa + la for oa, la, wa in extents(x) for ob, lb, wb in extents(y))


def random_tapes():
    """The twelve random tapes of small records on a crowded arena -- plenty of RAW, WAR and WAW hazards, accumulating
    records, reductions, a few gathers that interrupt the windows; the last one is a chain whose working set is larger than
    one window.  Yields (case, records [n, 8] int32, arena).  One generator runs through all cases: the order is part of it."""
    rng = np.random.default_rng(11)
    for case in range(12):
        size = 4096 if case < 11 else 40000
        nslot = 24 if case < 11 else 4000
        base = 64
        shapes = [(2, 2), (3, 3), (2, 1), (3, 1), (1, 1), (4, 4)]
        slots = []                              # (offset, m, n): matrices laid out back to back, so neighbours never overlap
        off = base
        for k in range(nslot):
            m, n = shapes[int(rng.integers(len(shapes)))]
            slots.append((off, m, n)); off += m * n
        assert off + 64 < size
        by_shape = {}
        for sl in slots:
            by_shape.setdefault((sl[1], sl[2]), []).append(sl)
        scal = [o for o, m, n in slots if (m, n) == (1, 1)] or [base]
        ops = []
        nrec = 700 if case < 11 else 6000
        idx_rows, idx_cols = size - 40, size - 30
        for r in range(nrec):
            kind = int(rng.integers(9))
            (m, n) = shapes[int(rng.integers(len(shapes)))]
            cand = by_shape.get((m, n), [])
            if len(cand) < 3:
                continue
            pick = lambda: cand[int(rng.integers(len(cand)))][0] if case < 11 else cand[min(len(cand) - 1, (r * len(cand)) // nrec + int(rng.integers(3)))][0]
            d_, a_, b_ = pick(), pick(), pick()
            if kind == 0 and d_ != a_: ops.append([G.T_COPY2D, d_, a_, n, m, n, n, 0])
            elif kind == 1 and len({d_, a_, b_}) == 3: ops.append([G.T_AXPBY, d_, a_, b_, m, n, int(rng.choice(scal)), int(rng.choice(scal))])
            elif kind == 2 and m == n and len({d_, a_, b_}) == 3: ops.append([G.T_GEMM, d_, a_, b_, m, n, m, int(rng.integers(8)) & 7])
            elif kind == 3 and len({d_, a_, b_}) == 3: ops.append([G.T_MUL, d_, a_, b_, m, n, 0, 0])
            elif kind == 4 and d_ != a_: ops.append([G.T_UNARY, d_, a_, 0, m, n, 0, 4])
            elif kind == 5 and m == n: ops.append([G.T_TRACE, int(rng.choice(scal)), a_, 0, m, m, 0, int(rng.integers(2)) * 4])
            elif kind == 6 and len({a_, b_}) == 2: ops.append([G.T_DOT, int(rng.choice(scal)), a_, b_, m, n, 0, 0])
            elif kind == 7 and d_ != a_: ops.append([G.T_FILL, d_, 0, n, m, n, 0, int(rng.integers(2))])
            elif kind == 8 and case % 3 == 2 and r % 50 == 49 and m == n and m >= 2:
                ops.append([G.T_GATHER, d_, a_, idx_rows, m, n, n, idx_cols])
        ops = np.asarray(ops, dtype=np.int32)
        arena = np.zeros(size)
        arena[base:off] = rng.uniform(-0.9, 0.9, off - base)        # |values| < 1: products and sums of a few hundred records stay finite
        arena[idx_rows:idx_rows + 4] = [1, 0, 2, 1]; arena[idx_cols:idx_cols + 4] = [0, 1, 1, 0]
        yield case, ops, arena


def _plan_stub():
    class P(object):
        temp_base, temp_high = 4096, 4096

        def __init__(self):
            self.vals = []

        def const(self, v):
            self.vals.append(float(v))
            return G.Ref(len(self.vals) - 1, 1, 1)

        def ones(self, n):
            o = len(self.vals)
            self.vals.extend([1.0] * n)
            return G.Ref(o, n, 1)
    return P()


def _arena(plan, fill):
    arena = np.zeros(plan.temp_high + 64)
    arena[:len(plan.vals)] = plan.vals
    for ref, arr in fill:
        arena[ref.off:ref.off + arr.size] = np.asarray(arr, dtype=float).reshape(-1)
    return arena


def long_tapes():
    """(a) 1700 records -- more than the 512 staged at a time -- on a small working set, (b) a working set (three 80 x 80
    matrices and their products) that exceeds the window and stays on global memory, (c) a tape with a gather record (addresses
    that are data: never cached).  {name: (records, arena, refs and inputs for the checks of the caller)}."""
    rng = np.random.default_rng(4)
    out = {}
    plan = _plan_stub()
    a = G.Ref(2048, 6, 6); b = G.Ref(2100, 6, 6)
    A = rng.standard_normal((6, 6)) * 0.3; B = rng.standard_normal((6, 6)) * 0.3
    t = G.Tape(plan)
    acc = t.copy(a)
    for k in range(560):                    # three records per turn
        g = t.gemm(acc, b)
        t.axpby(0.5, g, 0.5, a, dst=acc)
        t.mul(acc, acc) if k % 7 == 0 else t.unary(acc, G.U_NEG)
    assert len(t.ops) > 3 * 512
    out["a"] = (t.array(), _arena(plan, [(a, A), (b, B)]), dict(acc=acc))
    plan = _plan_stub()
    m = 80
    x, y, z = G.Ref(8192, m, m), G.Ref(8192 + m * m, m, m), G.Ref(8192 + 2 * m * m, m, m)
    plan.temp_base = plan.temp_high = 8192 + 3 * m * m
    t = G.Tape(plan)
    p1 = t.gemm(x, y); p2 = t.gemm(p1, z, tb=True); p3 = t.add(p2, t.transpose(p1))
    tr = t.trace(p3)
    mats = [rng.standard_normal((m, m)) / m for _ in range(3)]
    assert (plan.temp_high - 8192) > 12288      # larger than the LDS window
    out["b"] = (t.array(), _arena(plan, [(x, mats[0]), (y, mats[1]), (z, mats[2])]), dict(p3=p3, tr=tr, mats=mats, m=m))
    plan = _plan_stub()
    s = G.Ref(2048, 5, 5); rows = G.Ref(2100, 2, 1); cols = G.Ref(2110, 3, 1)
    t = G.Tape(plan)
    sq = t.gemm(s, s, tb=True)
    ga = t.gather(sq, rows, cols)
    res = t.scale(ga, 2.0)
    t.axpby(1.0, res, 1.0, res, dst=res)
    S = rng.standard_normal((5, 5))
    out["c"] = (t.array(), _arena(plan, [(s, S), (rows, np.array([4.0, 1.0])), (cols, np.array([0.0, 2.0, 3.0]))]), dict(out=res, S=S))
    return out


def many_short_blocks(nblocks=600):
    """A program of two launches: `nblocks` (>= 512: workgroups of four wavefronts) short blocks on disjoint state, each with
    independent records and a chain, then eight blocks that each sum up what a slice of the first launch left.
    (records, arena, blocks [nb, 2], launches [nl, 2])."""
    rng = np.random.default_rng(23)
    stride, base = 40, 64               # per block: x (3 x 3) at +0, y at +9, u at +18, v at +27, scalars at +36, +37
    ops, blocks = [], []
    for b in range(nblocks):
        o = base + stride * b
        x, y, u, v, s0, s1 = o, o + 9, o + 18, o + 27, o + 36, o + 37
        first = len(ops)
        ops += [[G.T_GEMM, u, x, y, 3, 3, 3, 0], [G.T_MUL, v, x, y, 3, 3, 0, 0], [G.T_TRACE, s0, x, 0, 3, 3, 0, 0],
                [G.T_DOT, s1, x, y, 3, 3, 0, 0], [G.T_AXPBY, x, u, v, 3, 3, s0, s1], [G.T_GEMM, y, x, u, 3, 3, 3, 4 | (b & 3)]]
        if b % 5 == 0:
            ops.append([G.T_UNARY, v, y, 0, 3, 3, 0, 4])
        blocks.append([first, len(ops) - first])
    tot = base + stride * nblocks
    per = nblocks // 8
    for k in range(8):                  # sums over the x of `per` blocks each, through a running 3 x 3 accumulator
        first = len(ops)
        acc = tot + 16 * k
        ops.append([G.T_FILL, acc, 0, 3, 3, 3, 0, 0])
        for b in range(k * per, (k + 1) * per):
            ops.append([G.T_AXPBY, acc, acc, base + stride * b, 3, 3, 0, 0])
        ops.append([G.T_TRACE, acc + 9, acc, 0, 3, 3, 0, 0])
        blocks.append([first, len(ops) - first])
    arena = np.zeros(tot + 16 * 8 + 64)
    arena[base:tot] = rng.uniform(-0.9, 0.9, tot - base)
    arena[0] = 1.0                      # the AXPBY of the second launch: alpha = beta = arena[0]
    return np.asarray(ops, dtype=np.int32), arena, np.asarray(blocks, dtype=np.int32), np.asarray([[0, nblocks], [nblocks, 8]], dtype=np.int32)


# ---- single records against an arena of 64 doubles: (record, accepted by pyvb_graph_tape_create).  Each verdict is worked out
# by hand from the record layouts: a record is accepted when its opcode is known, m, n (and p where it is a size) are not
# negative, leading dimensions are at least n, a T_UNARY function is 0..5, and every extent of non-zero length lies in [0, 64).
VALIDATION_ARENA = 64
_M = 2 ** 31 - 1
VALIDATION = [
    # the records tests/test_generic_gpu.py has always refused (and the well-formed one beside them)
    ([G.T_GEMM, 0, 16, 32, 4, 4, 4, 0], True),          # dst 0..15, a 16..31, b 32..47
    ([G.T_GEMM, 56, 0, 16, 4, 4, 4, 0], False),         # dst 56..71 leaves the arena of 64
    ([G.T_COPY2D, 0, 8, 2, 3, 4, 4, 0], False),         # leading dimension of dst (2) smaller than n (4)
    ([G.T_CHOLINV, 0, 16, 32, 4, 0, 40, 0], False),     # scratch 40 .. 40 + 2 * 16 leaves the arena
    ([G.T_UNARY, 0, 8, 0, 2, 2, 0, 9], False),          # no such function
    ([99, 0, 0, 0, 1, 1, 0, 0], False),                 # no such opcode
    ([G.T_AXPBY, 0, 8, -1, 70, 1, 1, 0], False),        # 70 elements
    # an extent that ends exactly at the arena end, and one element past it: dst, a, the scalar
    ([G.T_SCALE, 60, 0, 8, 2, 2, 0, 0], True), ([G.T_SCALE, 61, 0, 8, 2, 2, 0, 0], False),
    ([G.T_SCALE, 0, 60, 8, 2, 2, 0, 0], True), ([G.T_SCALE, 0, 61, 8, 2, 2, 0, 0], False),
    ([G.T_SCALE, 0, 4, 63, 2, 2, 0, 0], True), ([G.T_SCALE, 0, 4, 64, 2, 2, 0, 0], False),
    ([G.T_MUL, 0, 16, 48, 4, 4, 0, 0], True), ([G.T_MUL, 0, 16, 49, 4, 4, 0, 0], False),
    ([G.T_DOT, 63, 0, 32, 4, 8, 0, 0], True), ([G.T_DOT, 63, 0, 33, 4, 8, 0, 0], False), ([G.T_DOT, 64, 0, 32, 4, 8, 0, 0], False),
    ([G.T_TRACE, 63, 0, 0, 8, 0, 0, 0], True), ([G.T_TRACE, 63, 0, 0, 9, 0, 0, 0], False), ([G.T_TRACE, 63, 1, 0, 8, 0, 0, 0], False),
    ([G.T_DIAG, 0, 0, 0, 8, 0, 0, 0], True), ([G.T_DIAG, 57, 0, 0, 8, 0, 0, 0], False),      # flags 0: dst m, a m x m
    ([G.T_DIAG, 0, 56, 0, 8, 0, 0, 1], True), ([G.T_DIAG, 0, 57, 0, 8, 0, 0, 1], False),     # flags 1: dst m x m, a m
    ([G.T_CHOLINV, 0, 16, 62, 4, 0, 32, 0], True),      # dst 0..15, a 16..31, the two scalars 62, 63, scratch 32..63
    ([G.T_CHOLINV, 0, 16, 63, 4, 0, 32, 0], False), ([G.T_CHOLINV, 0, 16, 62, 4, 0, 33, 0], False),
    ([G.T_FILL, 56, 0, 4, 2, 4, 0, 0], True), ([G.T_FILL, 57, 0, 4, 2, 4, 0, 0], False),     # span (m - 1) ld + n = 8
    ([G.T_FILL, 0, 0, 30, 3, 4, 0, 1], True), ([G.T_FILL, 0, 0, 31, 3, 4, 0, 1], False),     # span 64, 66
    ([G.T_FILL, 0, 0, 3, 3, 4, 0, 0], False),           # ld < n
    ([G.T_COPY2D, 0, 0, 4, 3, 4, 30, 0], True), ([G.T_COPY2D, 0, 0, 4, 3, 4, 31, 0], False), ([G.T_COPY2D, 0, 0, 4, 3, 4, 3, 0], False),
    ([G.T_GEMM, 0, 16, 32, 4, 4, -1, 0], False), ([G.T_GEMM, 0, 999, 999, 2, 2, 0, 0], True),   # k = 0: a and b are empty
    ([G.T_UNARY, 0, 8, 0, 2, 2, 0, 5], True), ([G.T_UNARY, 0, 8, 0, 2, 2, 0, 6], False), ([G.T_UNARY, 0, 8, 0, 2, 2, 0, -1], False),
    ([14, 0, 0, 0, 1, 1, 0, 0], False), ([-1, 0, 0, 0, 1, 1, 0, 0], False),
    # negative offsets: refused with a length, nothing touched without one
    ([G.T_UNARY, -1, 8, 0, 2, 2, 0, 0], False), ([G.T_UNARY, 0, -1, 0, 2, 2, 0, 0], False),
    ([G.T_UNARY, -5, -7, 0, 0, 3, 0, 0], True), ([G.T_UNARY, 1000, 2000, 0, 3, 0, 0, 0], True),
    ([G.T_SCALE, -5, -7, -1, 0, 3, 0, 0], False),       # ... but its scalar is read whatever m and n are
    # m or n = 0
    ([G.T_COPY2D, 500, 500, 4, 0, 4, 4, 0], True), ([G.T_COPY2D, 500, 500, 3, 0, 4, 4, 0], False),     # the shape is still checked
    ([G.T_GEMM, 999, 999, 0, 0, 4, 4, 0], True), ([G.T_GEMM, 999, 999, 60, 0, 4, 4, 0], False),         # b is k x n = 16
    ([G.T_NOP, -9, -9, -9, 0, 0, -9, -9], True), ([G.T_NOP, 0, 0, 0, -1, 0, 0, 0], False), ([G.T_NOP, 0, 0, 0, 0, -1, 0, 0], False),
    ([G.T_TRACE, 63, 0, 0, 8, -1, 0, 0], False),        # n is not used by the opcode, and still must not be negative
    # T_AXPBY: alpha = arena[p]; b < 0: no third operand and no beta
    ([G.T_AXPBY, 0, 8, -1, 2, 2, 63, 9999], True), ([G.T_AXPBY, 0, 8, -1, 2, 2, 64, 0], False),
    ([G.T_AXPBY, 0, 8, 16, 2, 2, 63, 9999], False), ([G.T_AXPBY, 0, 8, 16, 2, 2, 63, 63], True), ([G.T_AXPBY, 0, 8, 61, 2, 2, 63, 63], False),
    ([G.T_AXPBY, 0, 0, -1, 0, 0, 64, 0], False),        # alpha is read whatever m and n are
    # T_GATHER / T_SCATTER: the block, the two index vectors, the base element; T_SCATTER keeps T_ACC in its column-index field
    ([G.T_GATHER, 48, 0, 40, 2, 2, 4, 44], True), ([G.T_GATHER, 48, 0, 40, 2, 2, 4, 63], False), ([G.T_GATHER, 48, 0, 63, 2, 2, 4, 44], False),
    ([G.T_GATHER, 48, 64, 40, 2, 2, 4, 44], False), ([G.T_GATHER, 61, 0, 40, 2, 2, 4, 44], False), ([G.T_GATHER, 48, 0, 40, 2, 2, -1, 44], False),
    ([G.T_GATHER, 48, 0, 40, 2, 2, 4, 44 | T_ACC], False),      # no flag in a gather: the offset is far outside
    ([G.T_SCATTER, 0, 8, 40, 2, 2, 4, 44], True), ([G.T_SCATTER, 0, 8, 40, 2, 2, 4, 44 | T_ACC], True),
    ([G.T_SCATTER, 0, 8, 40, 2, 2, 4, 62], True), ([G.T_SCATTER, 0, 8, 40, 2, 2, 4, 62 | T_ACC], True),
    ([G.T_SCATTER, 0, 8, 40, 2, 2, 4, 63], False), ([G.T_SCATTER, 0, 8, 40, 2, 2, 4, 63 | T_ACC], False),
    ([G.T_SCATTER, 63, 8, 40, 2, 2, 4, 44], True), ([G.T_SCATTER, 64, 8, 40, 2, 2, 4, 44], False), ([G.T_SCATTER, 0, 8, 40, 2, 2, -1, 44], False),
    ([G.T_SCATTER, 0, 61, 40, 2, 2, 4, 44], False), ([G.T_SCATTER, 0, 8, 63, 2, 2, 4, 44], False),
]
# m = n = 2^31 - 1 for every opcode (sizes whose products need 62 bits), with small and with equally large other fields:
# only T_NOP, which touches nothing, is accepted
VALIDATION += [([op, 0, 0, _M, _M, _M, _M, 0], op == G.T_NOP) for op in range(14)]
VALIDATION += [([op, _M, _M, _M, _M, _M, _M, _M], op == G.T_NOP) for op in range(14)]

# ---- the element limit of the opcodes that take tape_divmod (TAPE_MAX_ELEMS = 2^22, pyvb_amd/csrc/tape.h), against an arena of
# 2^24 doubles in which every extent below fits: only the limit decides.  Pairs: the largest record accepted, one row more refused.
TAPE_MAX_ELEMS = 1 << 22
VALIDATION_BOUND_ARENA = 1 << 24
_E, _H = TAPE_MAX_ELEMS, 1 << 23
VALIDATION_BOUND = [
    ([G.T_FILL, 0, 0, 4, _E // 4, 4, 0, 1], True), ([G.T_FILL, 0, 0, 4, _E // 4 + 1, 4, 0, 1], False),
    ([G.T_FILL, 0, 0, 1, _E, 1, 0, 0], True), ([G.T_FILL, 0, 0, 1, _E + 1, 1, 0, 0], False),
    ([G.T_COPY2D, 0, _H, 3, _E // 3, 3, 3, 0], True), ([G.T_COPY2D, 0, _H, 3, _E // 3 + 1, 3, 3, 0], False),     # 4 194 303, 4 194 306
    ([G.T_COPY2D, 0, _H, _E, 1, _E, _E, 0], True), ([G.T_COPY2D, 0, _H, _E + 1, 1, _E + 1, _E + 1, 0], False),
    ([G.T_GEMM, 0, _H, _H + 4096, 2048, 2048, 1, 0], True), ([G.T_GEMM, 0, _H, _H + 4096, 2049, 2048, 1, 0], False),
    ([G.T_GEMM, 0, 64, _H, 1, 1, _E + 1, 0], True),                 # k is not limited: a and b hold 2^22 + 1 doubles each
    ([G.T_DIAG, 0, _H, 0, 2048, 0, 0, 1], True), ([G.T_DIAG, 0, _H, 0, 2049, 0, 0, 1], False),
    ([G.T_DIAG, 0, _H, 0, 2049, 0, 0, 0], True),                    # flags 0 reads a[i m + i]: no division
    ([G.T_CHOLINV, 0, 0, 4 * _E - 2, 2048, 0, _E, 0], True),        # dst = a 0 .. 2^22, scratch 2^22 .. 3 * 2^22, scalars at the end
    ([G.T_CHOLINV, 0, 0, 4 * _E - 2, 2049, 0, 2049 * 2049, 0], False),      # scratch ends at 3 * 2049^2 = 12 595 203 < 2^24 - 2
    # the opcodes that address element idx as it is are limited by the arena alone
    ([G.T_UNARY, 0, _H, 0, _E + 1, 1, 0, 4], True), ([G.T_MUL, 0, _H, _H, 2049, 2048, 0, 0], True),
    ([G.T_AXPBY, 0, _H, -1, _E + 1, 1, 4 * _E - 1, 0], True), ([G.T_TRACE, 0, _H, 0, 2049, 0, 0, 0], True),
]
