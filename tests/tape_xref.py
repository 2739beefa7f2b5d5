"""TEST INFRASTRUCTURE: the tape interpreter in extended precision (np.longdouble), the reference that oracle/tape_ref.py
(float64 NumPy / SciPy) and the device interpreter (pyvb_amd/csrc/k_tape.hip) are measured against in
tests/test_tape_forms_cpu.py and tests/test_tape_forms_gpu.py.

run() interprets the records of pyvb_amd/csrc/tape.h on a long-double arena: products and sums in long double, the Cholesky
factor and the inverse through oracle/_xlinalg.py, digamma and gammaln through oracle/_xspecial.py.  For every ARITHMETIC
record it also returns the unit in which the error of each of its outputs is measured, the forward-error scale of the
operation formed in long double from the record's inputs, and the length n of its longest accumulation:

    T_GEMM      max_ij (|op(a)| |op(b)|)_ij  (+ max |dst| when accumulating)        n = k
    T_DOT       sum |a_ij b_ij|              (+ |dst|)                               n = m n
    T_TRACE     sum |a_ii|                   (+ |dst|)                               n = m
    T_AXPBY     max (|alpha a| + |beta b|)                                           n = 1
    T_CHOLINV   dst: max |inverse|; each of the two scalars: max(1, |value|)         n = m
    log, exp, digamma, lgamma: max(1, |f|) point by point                            n = 1

so that e = max |got - extended| / unit obeys e_gpu <= FACTOR max(e64, n 2^-52) (extended_ref.yardstick).  The records that
move data or do one correctly rounded IEEE operation (T_COPY2D, T_FILL, T_DIAG, T_GATHER, T_SCATTER without T_ACC, U_NEG, T_MUL,
T_SCALE both ways, U_RECIP) have no unit: they are compared bitwise with oracle/tape_ref.py.  T_SCALE divide and U_RECIP were
first measured in the unit max |result|: the device was bitwise NumPy's in every case and form (profiles/tape_envelope.txt), one
IEEE division each, so they are held to that."""
import numpy as np

from oracle import _xlinalg as XL
from oracle import _xspecial as XS
from oracle import tape_ref as R
import extended_ref as E

LD = np.longdouble
T_ACC = 0x40000000
U_LOG, U_DIGAMMA, U_LGAMMA, U_RECIP, U_NEG, U_EXP = range(6)


def is_exact(rec):
    op, fl = int(rec[0]), int(rec[7])
    return (op in (R.T_NOP, R.T_COPY2D, R.T_FILL, R.T_DIAG, R.T_GATHER, R.T_MUL) or (op == R.T_SCATTER and not fl & T_ACC)
            or (op == R.T_UNARY and fl in (U_NEG, U_RECIP)) or op == R.T_SCALE)


def _mx(x):
    return np.abs(x).max() if np.size(x) else LD(0)


def run(arena, ops):
    """arena: 1-D np.longdouble array, modified in place; ops [nops, 8].  Returns [(record index, offset, length, unit, n)], one
    entry per output of every arithmetic record; unit is a long-double scalar or an array of `length` (point by point)."""
    E.require_extended()
    assert arena.dtype == LD
    A = arena
    out = []
    for idx, o in enumerate(np.asarray(ops, dtype=np.int64).reshape(-1, 8)):
        op, d, a, b, m, n, p, fl = [int(v) for v in o]
        mn = m * n
        if is_exact(o):
            if op == R.T_MUL:
                A[d:d + mn] = A[a:a + mn] * A[b:b + mn]
            elif op == R.T_SCALE:
                A[d:d + mn] = A[a:a + mn] / A[b] if fl & 1 else A[a:a + mn] * A[b]
            elif op == R.T_UNARY:
                with np.errstate(all="ignore"):
                    A[d:d + mn] = 1.0 / A[a:a + mn] if fl == U_RECIP else -A[a:a + mn]
            else:
                R.run(A, [o])               # pure data movement: the float64 interpreter does not care about the dtype
            continue
        if op == R.T_AXPBY:
            x = A[p] * A[a:a + mn]
            y = A[fl] * A[b:b + mn] if b >= 0 else np.zeros(mn, dtype=LD)
            A[d:d + mn] = x + y
            out.append((idx, d, mn, _mx(np.abs(x) + np.abs(y)), 1))
        elif op == R.T_GEMM:
            k = p
            X = A[a:a + m * k].reshape((k, m)).T if (fl & 1) else A[a:a + m * k].reshape((m, k))
            Y = A[b:b + k * n].reshape((n, k)).T if (fl & 2) else A[b:b + k * n].reshape((k, n))
            Z = X @ Y if k else np.zeros((m, n), dtype=LD)
            unit = _mx(np.abs(X) @ np.abs(Y)) if k else LD(0)
            if fl & 8:
                Z = -Z
            cur = A[d:d + mn].reshape((m, n)).copy()
            if fl & 4:
                unit = unit + _mx(cur)
                Z = cur + Z
            A[d:d + mn] = Z.reshape(-1)
            out.append((idx, d, mn, unit, k))
        elif op in (R.T_TRACE, R.T_DOT):
            terms = A[a:a + m * m:m + 1].copy() if op == R.T_TRACE else A[a:a + mn] * A[b:b + mn]
            v, unit = terms.sum(), np.abs(terms).sum()
            if fl & 4:
                unit = unit + abs(A[d])
                v = A[d] + v
            A[d] = v
            out.append((idx, d, 1, unit, m if op == R.T_TRACE else mn))
        elif op == R.T_CHOLINV:
            M = A[a:a + m * m].reshape((m, m))
            Ms = np.tril(M) + np.tril(M, -1).T          # the kernel reads the lower triangle
            L = XL.cholesky(Ms)
            s = np.sum(np.log(np.diag(L)))
            inv = XL.inv(Ms)
            A[d:d + m * m] = inv.reshape(-1)
            A[b], A[b + 1] = LD(0.5) / s, s
            out.append((idx, d, m * m, _mx(inv), m))
            out.append((idx, b, 1, max(LD(1), abs(A[b])), m))
            out.append((idx, b + 1, 1, max(LD(1), abs(s)), m))
        elif op == R.T_UNARY:
            x = A[a:a + mn].copy()
            with np.errstate(all="ignore"):
                f = [np.log, XS.digamma, XS.gammaln, None, None, np.exp][fl](x)
            A[d:d + mn] = f
            out.append((idx, d, mn, np.maximum(LD(1), np.abs(f)), 1))
        elif op == R.T_SCATTER:                         # with T_ACC: one addition per element
            co = fl & ~T_ACC
            r = A[b:b + m].astype(int); c = A[co:co + n].astype(int)
            pos = (d + r[:, None] * p + c[None, :]).reshape(-1)
            before = A[pos].copy()
            A[pos] = before + A[a:a + mn]
            for q, e in enumerate(pos):
                out.append((idx, int(e), 1, abs(before[q]) + abs(A[a + q]), 1))
        else:
            raise ValueError("unknown opcode %d" % op)
    return out
