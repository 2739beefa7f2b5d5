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
