// What the host planner (tape_plan.h) and the device interpreter (k_tape) of the generic per-node path share: the opcodes
// and record layout of a TAPE, and the tables of its LDS-window form.  Plain C++: no device header is needed to read it.
#pragma once

enum {
    T_NOP = 0,
    T_COPY2D = 1,     // dst[i*p0 + j] = a[i*p1 + j]                         i < m, j < n       (p0, p1: leading dimensions)
    T_FILL = 2,       // dst[i*p0 + j] = (flags & 1) ? (i == j) : 0
    T_AXPBY = 3,      // dst = alpha a + beta b (m x n, contiguous); alpha = arena[p0], beta = arena[p1]; b < 0: dst = alpha a
    T_GEMM = 4,       // dst[m x n] (+)= op(a)[m x k] op(b)[k x n]; flags 1: a^T, 2: b^T, 4: accumulate, 8: subtract
    T_SCALE = 5,      // dst = a * s (flags 0) or a / s (flags 1), s = arena[b]; m x n
    T_TRACE = 6,      // dst[0] (+)= tr(a[m x m]) (flags 4: accumulate)
    T_DIAG = 7,       // flags 0: dst[m] = diag(a[m x m]); flags 1: dst[m x m] = diag(a[m])
    T_CHOLINV = 8,    // dst[m x m] = inverse of the s.p.d. a[m x m]; arena[b] = 0.5 / sum log diag chol (quirk Q1), arena[b+1] = sum log diag chol; p0 = scratch (2 m^2)
    T_DOT = 9,        // dst[0] (+)= sum_ij a_ij b_ij (m x n); flags 4: accumulate
    T_UNARY = 10,     // dst = f(a) elementwise, m x n; flags: 0 log, 1 digamma, 2 lgamma, 3 reciprocal, 4 negate, 5 exp
    T_GATHER = 11,    // dst[i*n + j] = a[r_i * p + c_j], r = (int)arena[b + i], c = (int)arena[flags + j]
    T_SCATTER = 12,   // dst[r_i * p + c_j] (+)= a[i*n + j], c = (int)arena[(flags & ~T_ACC) + j]; flags & T_ACC: accumulate
    T_MUL = 13,       // dst = a .* b elementwise, m x n
};

#define T_ACC 0x40000000
// record layout: o[0] opcode, o[1] dst, o[2] a, o[3] b (or a leading dimension / scalar offset), o[4] m, o[5] n, o[6] p, o[7] flags
//
// T_SCATTER with repeated (r_i, c_j) pairs: the elements that share a target are stored by different threads in no defined order.
// Without T_ACC one of their values is left there, which one is not specified; with T_ACC every one of them is an unordered
// read-modify-write of the target, so terms may be lost.  Emitters give a scatter distinct pairs (a gather may repeat its indices).
//
// The element limit.  The interpreter gives element idx of an m x n record its row and column without an integer division
// (tape_divmod in k_tape.hip): i = (int)((float(idx) + 0.5) * rn), rn the hardware's float reciprocal of n, then one step of
// fix-up by j = idx - i n.  That is exact for every idx < TAPE_MAX_ELEMS = 2^22:
//   * x = float(idx) + 0.5 is exact: 2 idx + 1 < 2^24 is an integer of 24 bits (true up to idx < 2^23); n <= 2^22 is exact too;
//   * rn = (1 / n)(1 + d1): the reciprocal instruction is good to 1 ulp; allowing the rounded float(1 / n) and either neighbour
//     of it gives |d1| <= 1.5 ulp <= 1.5 * 2^-23.  The product is rounded once, |d2| <= 2^-24.  So the computed quotient is
//     q' = q (1 + d), q = (idx + 0.5) / n, |d| <= (1.5 * 2^-23 + 2^-24)(1 + 2^-24) = 2^-22 (1 + 2^-24);
//   * |q' - q| <= q 2^-22 (1 + 2^-24) <= (2^22 - 0.5) / n * 2^-22 (1 + 2^-24) = (1 - 2^-23)(1 + 2^-24) / n < 1 / n;
//   * with i = idx div n and j = idx mod n the true q = i + (j + 0.5) / n lies in [i + 0.5 / n, i + 1 - 0.5 / n], hence
//     q' in (i - 0.5 / n, i + 1 + 0.5 / n), q' >= 0, and (int)q' is i - 1, i or i + 1: what the fix-up covers.
// Beyond the limit the row can be off by more than one (in a float32 simulation first at idx = 8 388 609 for n = 1 with the
// reciprocal one ulp high, at 12 582 911 for n = 2), and a strided store then lands
// outside the record's span.  So a record of an opcode that takes this path -- T_COPY2D, T_FILL, T_GEMM (m n; k is free),
// T_DIAG with flags 1 and T_CHOLINV (m m) -- with more than TAPE_MAX_ELEMS elements is malformed (tape_describe).  The other
// opcodes address element idx as it is and are limited by the arena alone.
#define TAPE_MAX_ELEMS (1 << 22)
//
// The LDS-window form: when a tape is uploaded the host cuts every block of records that one workgroup
// interprets into WINDOWS, the longest runs of consecutive records whose extents, merged into segments, fit the LDS budget.  The
// workgroup takes them in order: load the segments, run the records out of LDS (their offsets rewritten to window positions and
// tagged T_LDS), write the written segments back.  Records whose addresses are data (gather / scatter) and runs too short to pay
// for a window stay on the arena.  The records of a window of node-sized operands are also scheduled into BUNDLES of mutually
// independent records, a wavefront each; slots without a record hold T_NOP.
#define T_LDS 0x40000000        // in an offset field of a resolved record: position in the workgroup's LDS window, not in the arena
#define TAPE_CHUNK 512          // records staged at a time
#define TAPE_LDS_CAP 12288      // doubles of arena a block may keep in LDS (96 KB)
#define TAPE_MAX_SEGS 4096
#define TAPE_BUNDLE 8           // records per bundle = wavefronts of a k_tape_cached workgroup
#define TAPE_BUNDLE_MAX 2048    // records scheduled together (the dependency search is quadratic)

// The window form as the device reads it.  Block table: {first window, number of windows} per block, two ints.
struct TapeWindow {
    int first, count;           // device records (resolved, window by window) of this window
    int seg0, nseg;             // its segments; nseg == 0: the records address the arena
    int doubles;                // LDS doubles the segments take
    int bundled;                // 1: count is a multiple of the launch's bundle width, record w of a bundle belongs to wavefront w
    int pad[2];
};
struct TapeSegment {
    int off, len;               // arena extent
    int lds;                    // where it sits in the window
    int written;                // 1: copied back after the window's records
};
static_assert(sizeof(TapeWindow) == 8 * sizeof(int), "TapeWindow is eight ints on the device");
static_assert(sizeof(TapeSegment) == 4 * sizeof(int), "TapeSegment is four ints on the device");
