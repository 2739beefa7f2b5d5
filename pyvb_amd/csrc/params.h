// Shared by the parameter-update translation units (k_params.hip, k_cols.hip).
#pragma once
#include "common.h"
#include "digamma.h"

#define LN2PI 1.8378770664093453

// The prior precision of the columns of one matrix (A or C) as the column kernels read it: a strided view, so that Constant
// parents (one [D][rows] array shared by the replicates) and Gamma parents (one expectation per replicate and column, the same
// in every row: automatic relevance determination, k_ard.hip) are the same loads.
//   precision of row k of column i in replicate n:  pp[n * pp_n + i * pp_c + k * pp_r]
//   ln det of column i's prior precision:            pld[n * pld_n + i]
// Constant parents: strides (0, rows, 1) over Priors::A_pp / C_pp and (0) over A_pld / C_pld.  Gamma parents: (D, 1, 0) over the
// expectations qa / qb and (D) over the log-determinants of the handle's bound mode.  DiagonalGamma parents (one Gamma per entry,
// k_ard.hip: k_entry): (D rows, rows, 1) over the expectations and (D) over the log-determinants.
struct ColumnPrior {
    const double* pp; int pp_n, pp_c, pp_r;
    const double* pld; int pld_n;
    // Gamma parents alpha_i ~ Gamma(a0_i, b0_i) of the columns; all null with Constant parents
    const double *a0, *b0, *qa;             // [D]; qa_i = a0_i + rows / 2 is fixed by the graph (nodes_todo.py:125-128)
    double *qb, *ex, *ld_ref, *ld_exact;    // [N][D]: qb, qa / qb, rows (ln qa - ln qb) (quirk Q2), rows (psi(qa) - ln qb)
    // DiagonalGamma parents: a0, b0, qa are [D][rows] (qa = a0 + 1/2), qb and ex [N][D][rows], ld_ref / ld_exact [N][D] the sums
    // over the rows of ln qa - ln qb / psi(qa) - ln qb, and the four below are set; all null otherwise
    const double *lnqa, *psi, *cst;         // [D][rows]: ln qa, psi(qa), the part of gamma_llb(a0, b0, qa, qb) that does not depend on qb
    double* own;                            // [N][D]: sum over the rows of the nodes' own terms
};

struct ParamArgs {
    // statistics
    const double* part; int nchunk; const double* Sigma; const double* qld_x; const double* X; const double* Syy;
    double* mom;            // [N][mom_total]: see k_moments
    const double* sxx;      // k_moments: [N][W][DP][DP] parts of the interior sum of mu mu^T from the backward sweep, or null (then from part)
    int W;
    // parameters
    double *A_mean, *A_var, *C_mean, *C_var, *Q_a, *Q_b, *R_a, *R_b, *qld_A, *qld_C;
    double *lnd_A, *lnd_C;  // ln det qcov of the columns, stored beside qld_A / qld_C by the column kernels
    const double* lnd_x;    // [N][3] ln det Sigma beside qld_x
    double *resQ, *resR, *elbo;
    const double* Yent;     // k_elbo: per replicate, what the outputs that are not fully observed subtract (k_missing.hip), or null
    const double* YentX;    // k_elbo, exact bound: per replicate, the entropy of those outputs (k_missing.hip), or null
    int bound;              // k_elbo: PYVB_BOUND_REFERENCE or PYVB_BOUND_EXACT
    Priors pri;
    int N, T, D, K, noise;
    int c0, c1;             // k_cols: columns [c0, c1) are updated
    int fuse;               // k_cols: bit 0 = residuals of the noise node too, bit 1 = and its update
    const unsigned char* active;    // [N]: workgroups of switched-off replicates leave at once
    int which0;             // blockIdx.y + which0 selects the matrix / noise node (0: A, Q; 1: C, R)
    Layout L;
    const int* len;         // [N] chain length T_n of each replicate (pyvb_lds_create_lengths), or null: T.  T stays the row stride of X
    const unsigned char* first;     // k_elbo: [N] 1 = first replicate of its model (pyvb_lds_create_tied), or null: every one is
    int Lw;                 // k_moments: interior nodes per part of sxx, cut from the handle's T as k_sweep cuts them
    ColumnPrior cpA, cpC;   // k_cols, k_elbo, k_ard: the prior precisions of the columns of A and C
    int derive;             // k_ard, k_entry: 1 = qb is given (pyvb_lds_set_column_precisions, pyvb_lds_set_entry_precisions): form
                            // what follows from it, in every row
};

// layout of the per-replicate moment block written by k_moments (all row-major, no padding)
// (T: the replicate's own chain length T_n on a handle with lengths)
//   GA [D][D]  = sum_{t=0}^{T-2} <x x^T>      (children of hstack A: Mult(A, X_t))
//   GC [D][D]  = sum_{t=0}^{T-1} <x x^T>      (children of hstack C)
//   HA [D][D]  = sum_t mu_{t+1} mu_t^T        HC [K][D] = sum_t y_t mu_t^T
//   dp [D]     = diag sum_{t=1}^{T-1} <x x^T> (children of Q)
__host__ __device__ static inline size_t mom_total(int D, int K) { return (size_t)3 * D * D + (size_t)K * D + D; }
#define MOM_GA(D, K) ((size_t)0)
#define MOM_GC(D, K) ((size_t)(D) * (D))
#define MOM_HA(D, K) ((size_t)2 * (D) * (D))
#define MOM_HC(D, K) ((size_t)3 * (D) * (D))
#define MOM_DP(D, K) ((size_t)3 * (D) * (D) + (size_t)(K) * (D))

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// value of v in lane j (j wave-uniform) for every lane: two v_readlane_b32, no LDS
__device__ __forceinline__ double bcast(double v, int j) {
    const int lo = __builtin_amdgcn_readlane(__double2loint(v), j);
    const int hi = __builtin_amdgcn_readlane(__double2hiint(v), j);
    return __hiloint2double(hi, lo);
}

ParamArgs make_args(pyvb_lds* h);
