// What a handle is sized as and how it is cut: the layout of a replicate's gains and statistics, the parts of the time axis a
// sweep deals out, the chunks of the statistics passes, and every buffer extent that depends on the shape class or on the time
// split -- for pyvb_lds (lds_geometry) and pyvb_pca (pca_geometry).  Standard C++ only: nothing here needs a device, so
// tests/c/geometry_driver.cpp runs it under the host sanitizers and tests/test_geometry_cpu.py compares it with recorded tables.
// The few functions kernels call are PYVB_HD.  api.hip and api_pca.hip allocate from these records and spell no extent themselves.
#pragma once
#include <cstddef>
#include "../../include/pyvb_hip.h"

#ifdef __HIPCC__
#define PYVB_HD __host__ __device__
#else
#define PYVB_HD
#endif

void pyvb_set_error(const char* fmt, ...);

// Per-replicate block of "gains": every matrix the state updates multiply by, written by
// k_prep once per parameter change and read by the sweep / step kernels.
//   Sigma_c = posterior covariance of class c (0: X_0, 1: interior, 2: X_{T-1})
//   F  = Sigma_1 <Q><A>      B  = Sigma_1 <A>^T<Q>     G  = Sigma_1 <C>^T<R>
// The two boundary nodes are single matrix-vector chains, mu = Sigma_c (sum of the messages), so for them
// the block holds the pieces instead of products: S0 = Sigma_0, S2 = Sigma_2 ([row][DP]), qr = <Q> diagonal
// (QR = 64 entries, 128 in the second shape class) then <R> diagonal (QR), w0 = L0 m0 (the Constant parents of X_0).
// "n"/"p" blocks are laid out as v_mfma_f64_16x16x4 A-operands: element [(m*S+s)*64+lane]
// = M[16m + (lane&15)][kidx(s, lane>>4)], kidx natural = 4s+q (F, B: they meet states, which come in
// accumulator order), permuted = 8(s>>1)+2q+(s&1) (G: it meets rows of Y read 16 bytes per lane).
// (pos_nat / pos_perm below give the position of element (i, j) in such a block.)
struct Layout {
    int D, K, DT, KT, DP, KP, DS, KS;
    int QR;                 // length of each of the two noise diagonals at oqr: 64, or 128 in the second shape class
    size_t oFn, oBn, oGp;
    size_t oS0, oS2, oqr, ow0;
    size_t gains_total;     // doubles per replicate
    size_t stats_total;     // doubles per replicate per chunk: Sxx[DP][DP], Sx1x[DP][DP], Syx[KP][DP]
    size_t oSxx, oSx1x, oSyx;
};

// Internal layout of a state row (X buffers, stride DP): "accumulator order".  Dimension
// d = 16m + 4r + q sits at 16m + 4q + r, which is where lane group q keeps register r of tile m of a
// v_mfma_f64_16x16x4 accumulator -- and also its B operand of k-step 4m + r.  A lane therefore moves
// four contiguous doubles per tile, for the state stores as well as for the neighbour loads.
PYVB_HD static inline int xpos(int d) { return (d & ~15) | ((d & 3) << 2) | ((d >> 2) & 3); }

// position of matrix element (i, j) in an MFMA A-operand block with S k-steps
PYVB_HD static inline size_t pos_nat(int i, int j, int S) {
    return ((size_t)((i >> 4) * S + (j >> 2)) * 64) + (j & 3) * 16 + (i & 15);
}
PYVB_HD static inline size_t pos_perm(int i, int j, int S) {
    int s = 2 * (j >> 3) + (j & 1), q = (j & 7) >> 1;
    return ((size_t)((i >> 4) * S + s) * 64) + q * 16 + (i & 15);
}

// column covariances under Wishart noise are stored as the upper 8 x 8 tiles of the matrix (k_wishart.hip: cov_pos)
PYVB_HD static inline int cov_tiles(int rows) { const int RT = (rows + 7) >> 3; return RT * (RT + 1) / 2; }
PYVB_HD static inline size_t cov_stride(int rows) { return (size_t)cov_tiles(rows) * 64; }

static inline int tiles16(int d) { return d <= 16 ? 1 : (d <= 32 ? 2 : (d <= 64 ? 4 : 8)); }

static inline Layout make_layout(int D, int K) {
    Layout L;
    L.D = D; L.K = K;
    L.DT = tiles16(D); L.KT = tiles16(K);
    if (L.DT > 4 || L.KT > 4) L.DT = L.KT = 8;      // the second shape class (k_big.hip): both dimensions padded to 128
    L.QR = L.DT > 4 ? 128 : 64;
    L.DP = 16 * L.DT; L.KP = 16 * L.KT;
    L.DS = 4 * L.DT; L.KS = 4 * L.KT;
    size_t o = 0;
    size_t dd = (size_t)L.DT * L.DS * 64, dk = (size_t)L.DT * L.KS * 64;
    L.oFn = o; o += dd; L.oBn = o; o += dd; L.oGp = o; o += dk;
    size_t tdd = (size_t)L.DP * L.DP, tkd = (size_t)L.KP * L.DP;
    L.oS0 = o; o += tdd; L.oS2 = o; o += tdd; L.oqr = o; o += 2 * (size_t)L.QR; L.ow0 = o; o += L.DP;
    L.gains_total = o;
    L.oSxx = 0; L.oSx1x = tdd; L.oSyx = 2 * tdd;
    L.stats_total = 2 * tdd + tkd;
    return L;
}

// ---- the time split: the sweeps deal the interior nodes 1 .. T-2 of a chain out to W parts (k_sweep.hip: a wavefront each;
// k_big.hip: a workgroup each), counted from the side the sweep starts at.  The one definition of the cut.
// Interior nodes per part where the axis is split (W > 1): a multiple of 16, since every part is again cut into 16 segments.
PYVB_HD static inline int split_part_len(int T, int W) { return (((T - 2 + W - 1) / W) + 15) & ~15; }
PYVB_HD static inline int part_len(int T, int W) { return W > 1 ? split_part_len(T, W) : T - 2; }
// Parts that hold nodes of a chain of TL <= T nodes: part w starts at interior node w * Lw, and a chain shorter than the
// handle's T fills the first parts and leaves the others without nodes.  (live_parts_of: for a kernel, which is handed
// Lw = part_len(T, W) and has the chain's interior nodes, TL - 2, at hand.  The chain's own number comes last: with it
// first k_moments compiles to other, equivalent instructions than with the expression written out in the kernel.)
PYVB_HD static inline int live_parts_of(int Lw, int W, int interior) {
    const int live = interior <= 0 ? 0 : (W == 1 ? 1 : (interior + Lw - 1) / Lw);
    return live < W ? live : W;
}
static inline int live_parts(int TL, int T, int W) { return live_parts_of(part_len(T, W), W, TL - 2); }

enum {
    MAX_TIME_SPLIT = 128,           // W is in 1 .. 128
    MIN_PART_DEFAULT = 64,          // the W a handle picks for itself leaves parts of at least 64 nodes
    MIN_PART_FORCED = 16,           // pyvb_lds_set_time_split admits parts down to 16 nodes: one per segment
    RESIDENT_SLOTS = 1024,          // wavefronts of k_sweep the chip runs at a time
    RESIDENT_SLOTS_BIG = 256,       // the 128-wide class: a part is a workgroup of four wavefronts, one per CU at a time
    WARMUP_STEPS = 32               // J, the warm-up steps a part pays before its first node (about; k_prep sets the real one)
};

// the conditions of pyvb_lds_set_time_split: PYVB_OK, or PYVB_E_ARG with the message set
static inline int check_time_split(int T, int W) {
    if (!(W >= 1 && W <= MAX_TIME_SPLIT)) { pyvb_set_error("%s", "W must be in 1..128"); return PYVB_E_ARG; }
    if (!(W == 1 || (T - 2) / W >= MIN_PART_FORCED)) { pyvb_set_error("%s", "parts of fewer than 16 nodes"); return PYVB_E_ARG; }
    return PYVB_OK;
}

// ---- pyvb_lds
struct LdsGeometry {
    int N, T, D, K;
    bool big;               // 64 < max(D, K) <= 128: the workgroup-per-replicate kernels of k_big.hip
    bool dense;             // Wishart noise
    Layout L;
    int nchunk, chunk_len;  // time chunks of the statistics kernel
    int W;                  // parts of the time axis in the sweeps
    // extents in doubles
    size_t sxx;             // [N][W][DP][DP] (the 128-wide sweeps fuse no statistics: a stub)
    size_t U2;              // [N][T][DP] in the 128-wide class with W > 1, else 0: no such buffer
    size_t trash;           // [N][512], in the 128-wide class [N][W][512]: per (replicate, part of the time axis)
    size_t scratch;         // [N][2][D][D], in the 128-wide class [N][2][DP][DP]
    size_t SG;              // [N][2][64][64], in the 128-wide class [N][2][128][128]; 0 unless dense
    size_t stats;           // [N][nchunk][L.stats_total]
    size_t mom;             // [N][3 D^2 + K D + D]
    size_t priors;          // x0_mean D, x0_prec D*D, A_pm D*D, A_pp D*D, C_pm K*D, C_pp D*K, Q_a0 D, Q_b0 D, R_a0 K, R_b0 K,
                            // A_obs D*D, C_obs K*D, A_pld D, C_pld D, Q_w0 D*D, R_w0 K*K

    // the same record for a forced time split (check_time_split admits W)
    LdsGeometry with_time_split(int W_) const {
        LdsGeometry g = *this;
        const size_t n = (size_t)N;
        g.W = W_;
        g.sxx = big ? 8 : n * (size_t)W_ * L.DP * L.DP;
        g.U2 = big && W_ > 1 ? n * T * L.DP : 0;
        g.trash = n * (size_t)(big ? W_ : 1) * 512;
        return g;
    }
};

static inline LdsGeometry lds_geometry(int N, int T, int D, int K, int noise_kind) {
    LdsGeometry g;
    g.N = N; g.T = T; g.D = D; g.K = K;
    g.L = make_layout(D, K);
    g.big = D > 64 || K > 64;
    g.dense = noise_kind == PYVB_NOISE_WISHART;
    // time chunks of the statistics kernel: enough wavefronts to fill the chip when N is small
    int nchunk = (1024 + N - 1) / N;
    if (nchunk > 32) nchunk = 32;
    if (nchunk > (T + 15) / 16) nchunk = (T + 15) / 16;
    if (nchunk < 1) nchunk = 1;
    int clen = (T + nchunk - 1) / nchunk;
    clen = (clen + 3) & ~3;
    nchunk = (T + clen - 1) / clen;
    g.nchunk = nchunk; g.chunk_len = clen;
    // The sweeps may split the time axis over W wavefronts per replicate (k_sweep.hip).  A wavefront takes
    // ceil(part/16) + J steps (J ~ 32 warm-up steps), the chip runs 1024 of them at a time: W minimises
    // rounds x steps, with parts of at least 64 nodes.  At N >= 1024 that is W = 1.
    // (The 128-wide class: a part is a workgroup of four wavefronts, one per CU at a time.)
    int W = 1;
    const long Tint = T - 2, slots = g.big ? RESIDENT_SLOTS_BIG : RESIDENT_SLOTS;
    double best = 1e300;
    for (int w = 1; w <= MAX_TIME_SPLIT && (w == 1 || Tint / w >= MIN_PART_DEFAULT); ++w) {
        const long part = part_len(T, w);
        const double cost = (double)(((long)N * w + slots - 1) / slots) * (double)((part + 15) / 16 + WARMUP_STEPS);
        if (cost < best * 0.97) { best = cost; W = w; }      // prefer fewer wavefronts unless clearly better
    }
    const size_t n = (size_t)N;
    g.scratch = g.big ? n * 2 * g.L.DP * g.L.DP : n * 2 * D * D;
    g.SG = !g.dense ? 0 : (g.big ? n * 2 * 128 * 128 : n * 2 * 64 * 64);
    g.stats = n * nchunk * g.L.stats_total;
    g.mom = n * ((size_t)3 * D * D + (size_t)K * D + D);
    g.priors = (size_t)D + 3 * (size_t)D * D + 2 * (size_t)K * D + 2 * (size_t)D + 2 * (size_t)K + (size_t)D * D + (size_t)K * D + 2 * (size_t)D
               + (size_t)D * D + (size_t)K * K;
    return g.with_time_split(W);
}

// ---- pyvb_pca
struct PcaGeometry {
    int DP, QP, DT, QT;
    int nchunk; long chunk_rows;        // pass 2 runs nchunk workgroups of ceil(DT / 2) wavefronts, pass 1 nchunk x 4
    int nchunkB; long chunk_rowsB;      // k_pca_pairs: one workgroup per CU, the rows dealt out in multiples of 16
    int sweep;                          // PYVB_PCA_SWEEP_*: the default kind of the lazy sweep
};

// ncu: the device's compute units.  A count below 1 leaves nchunk at its size-independent default and gives the pairs partition
// one CU (what the two queries of the CU count that creation once made did, the first tolerant, the second not, with such a count).
static inline PcaGeometry pca_geometry(long N, int d, int q, int ncu) {
    PcaGeometry g;
    g.DP = (d + 15) & ~15; g.QP = (q + 15) & ~15; g.DT = g.DP / 16; g.QT = g.QP / 16;
    long nchunk = (16384 + g.DT - 1) / g.DT;
    // the sweep's workgroup (seven or eight wavefronts, 120 KB of LDS) has a CU to itself: ONE chunk per CU, so that every
    // workgroup pays its prologue (operands, first tiles) and its partial sums once -- measured at N = 10^6 x 256:
    // 1024 chunks (four rounds) 1.040 ms per iteration, 768: 1.028, 512: 1.009, 256: 0.990 (profiles/r04/pca_chunks.txt)
    if (g.DT >= 13 && ncu > 0) nchunk = ncu;
    const long ntile = (N + 15) / 16;
    if (nchunk > ntile) nchunk = ntile;
    if (nchunk < 1) nchunk = 1;
    long rows = (N + nchunk - 1) / nchunk;
    rows = (rows + 15) & ~15L;
    nchunk = (N + rows - 1) / rows;
    g.nchunk = (int)nchunk; g.chunk_rows = rows;
    if (ncu < 1) ncu = 1;
    long rowsB = (N + ncu - 1) / ncu;
    rowsB = (rowsB + 15) & ~15L;
    if (rowsB < 64) rowsB = 64;
    long ncB = (N + rowsB - 1) / rowsB;
    if (ncB > nchunk) { ncB = nchunk; rowsB = ((N + ncB - 1) / ncB + 15) & ~15L; ncB = (N + rowsB - 1) / rowsB; }
    g.nchunkB = (int)ncB; g.chunk_rowsB = rowsB;
    // which kernel the lazy sweep is (k_pca.hip): pairs (k_pca_pairs) where a CU's share is long enough to stream (measured
    // at 10^6 x 256: 0.95 against 0.97 ms per iteration), columns (k_pca_pass12<.., LAZY>) otherwise; pyvb_pca_set_sweep
    // changes it
    g.sweep = (g.DT >= 13 && N >= 512L * ncu) ? PYVB_PCA_SWEEP_PAIRS : PYVB_PCA_SWEEP_COLUMNS;
    return g;
}
