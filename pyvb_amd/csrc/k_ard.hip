// k_ard: the Gamma precision parents of the columns of A and C (automatic relevance determination).
//   column i of A (of C) is  N(pm_i, alpha_i^-1 I)  with  alpha_i ~ Gamma(a0_i, b0_i):  Gaussian(dim, pmu, pprec) with a Gamma
//   node as pprec (gaussian.py:55-61), one node per column.
//   [al.update() for al in alphas]: Gamma.update nodes_todo.py:130-138 with the column as the only child and a Constant
//   mean parent,   qb_i = b0_i + 1/2 sum_k ((M[k,i] - pm[k,i])^2 + V[i][k]);
//   qa_i = a0_i + rows / 2 is fixed by the graph (:125-128) and kept by the host.
// Known entries are stored as M = value, V = 0 (k_cols.hip), so the sum covers partly and fully known columns as it stands; a
// fully known column's alpha updates like any other (Gamma.update does not look at `observed`).
//
// One wavefront per (replicate, matrix), lane = column.  The loads of M[k][lane] and pm[k][lane] are coalesced, each lane walks its
// own contiguous V[lane][.].  The rows are summed in ascending order into one accumulator: the result depends on nothing but the
// inputs.  Beside qb the kernel leaves what k_cols and k_elbo read of the node through their strided view (params.h:
// ColumnPrior): the expectation qa / qb, and rows times ln E[alpha] (quirk Q2) and E[ln alpha] for the two bound modes.
#include "params.h"

__global__ void __launch_bounds__(64) k_ard(ParamArgs a) {
    const int WHICH = a.which0 + blockIdx.y;
    const int n = blockIdx.x, lane = threadIdx.x, D = a.D;
    if (!a.derive && !a.active[n]) return;
    if (lane >= D) return;
    const int rows = WHICH == 0 ? D : a.K;
    const size_t o = (size_t)n * D + lane;
    double* qbp = (WHICH == 0 ? a.cpA.qb : a.cpC.qb) + o;
    double qb;
    if (a.derive) {
        qb = *qbp;
    } else {
        const double* M = (WHICH == 0 ? a.A_mean : a.C_mean) + (size_t)n * rows * D + lane;
        const double* Vi = (WHICH == 0 ? a.A_var : a.C_var) + (size_t)n * D * rows + (size_t)lane * rows;
        const double* pm = (WHICH == 0 ? a.pri.A_pm : a.pri.C_pm) + lane;
        double s = 0.0;
#pragma unroll 8
        for (int k = 0; k < rows; ++k) {
            const double d = M[(size_t)k * D] - pm[(size_t)k * D];
            s += d * d + Vi[k];
        }
        qb = (WHICH == 0 ? a.cpA.b0 : a.cpC.b0)[lane] + 0.5 * s;
        *qbp = qb;
    }
    const double qa = (WHICH == 0 ? a.cpA.qa : a.cpC.qa)[lane], lb = log(qb);
    (WHICH == 0 ? a.cpA.ex : a.cpC.ex)[o] = qa / qb;                                            // Gamma.pass_down_Ex     nodes_todo.py:140-142
    (WHICH == 0 ? a.cpA.ld_ref : a.cpC.ld_ref)[o] = (double)rows * (log(qa) - lb);              // Gamma.pass_down_lndet  :144-147
    (WHICH == 0 ? a.cpA.ld_exact : a.cpC.ld_exact)[o] = (double)rows * (digamma_pos(qa) - lb);
}

// k_entry: the DiagonalGamma precision parents of the columns of A and C: a precision of its own for every entry.
//   column i of A (of C) is  N(pm_i, diag(alpha_i)^-1)  with  alpha_i[k] ~ Gamma(a0[i][k], b0[i][k]):  Gaussian(rows, pmu, pprec) with
//   a DiagonalGamma node as pprec (gaussian.py:55-61; nodes_todo.py:159-204), one node per column.
//   [dg.update() for dg in parents]: DiagonalGamma.update :187-190 with the column as the only child and a Constant mean parent,
//     qb[i][k] = b0[i][k] + 1/2 ((M[k,i] - pm[k,i])^2 + V[i][k]);    qa = a0 + 1/2 is fixed by the graph (:183-186).
// Known entries are M = value, V = 0 as for k_ard.
//
// One workgroup of four wavefronts per (replicate, matrix), lane = row k: b0, qa, V, qb and the expectations are contiguous in k, and
// a lane reads four consecutive entries of its row of M and pm per step, so four columns are in flight at once in a wavefront; the
// groups of four columns are dealt out to the wavefronts in turn, which share nothing (one wavefront per pair walked its sixteen
// groups one after the other with two wavefronts per SIMD in flight: 0.29 ms per pair of launches at the headline shape).
// Per column the kernel leaves three sums over the rows -- ln qa - ln qb (pass_down_lndet :195-197, quirk Q2, as a sum of logarithms), psi(qa) - ln qb (the exact
// bound's E[ln det]) and the nodes' own terms (log_lower_bound :199-204) -- each a butterfly over the 64 lanes, the twelve chains of
// the four columns interleaved.  The butterfly adds the same pairs in the same order whatever the data: two runs agree bitwise.
// The own term of an entry is  cst - a0 ln qb - b0 qa / qb  with cst = (a0 - qa) psi(qa) - lgamma(a0) + a0 ln b0 + lgamma(qa) + qa
// formed by the host (api.hip), which also gives ln qa and psi(qa): one logarithm per entry is left here.
#define ENTRY_COLS 4
#define ENTRY_WAVES 4
__global__ void __launch_bounds__(64 * ENTRY_WAVES) k_entry(ParamArgs a) {
    const int WHICH = a.which0 + blockIdx.y;
    const int n = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6, D = a.D;
    if (!a.derive && !a.active[n]) return;
    const int rows = WHICH == 0 ? D : a.K;
    const bool live = lane < rows;
    const int k = live ? lane : rows - 1;       // lanes past the last row load the last row's entries and store nothing
    const size_t nb = (size_t)n * D * rows;
    double* qbn = (WHICH == 0 ? a.cpA.qb : a.cpC.qb) + nb;
    double* exn = (WHICH == 0 ? a.cpA.ex : a.cpC.ex) + nb;
    const double* a0 = WHICH == 0 ? a.cpA.a0 : a.cpC.a0;
    const double* b0 = WHICH == 0 ? a.cpA.b0 : a.cpC.b0;
    const double* qa = WHICH == 0 ? a.cpA.qa : a.cpC.qa;
    const double* lnqa = WHICH == 0 ? a.cpA.lnqa : a.cpC.lnqa;
    const double* psi = WHICH == 0 ? a.cpA.psi : a.cpC.psi;
    const double* cst = WHICH == 0 ? a.cpA.cst : a.cpC.cst;
    double* ld_ref = (WHICH == 0 ? a.cpA.ld_ref : a.cpC.ld_ref) + (size_t)n * D;
    double* ld_exact = (WHICH == 0 ? a.cpA.ld_exact : a.cpC.ld_exact) + (size_t)n * D;
    double* own = (WHICH == 0 ? a.cpA.own : a.cpC.own) + (size_t)n * D;
    const double* Mk = (WHICH == 0 ? a.A_mean : a.C_mean) + (size_t)n * rows * D + (size_t)k * D;       // row k of M
    const double* pmk = (WHICH == 0 ? a.pri.A_pm : a.pri.C_pm) + (size_t)k * D;
    const double* V = (WHICH == 0 ? a.A_var : a.C_var) + nb;
    for (int i0 = wave * ENTRY_COLS; i0 < D; i0 += ENTRY_COLS * ENTRY_WAVES) {
        double sr[ENTRY_COLS], sx[ENTRY_COLS], so[ENTRY_COLS];
#pragma unroll
        for (int u = 0; u < ENTRY_COLS; ++u) {
            const bool on = live && i0 + u < D;
            const int i = i0 + u < D ? i0 + u : D - 1;
            const size_t e = (size_t)i * rows + k;
            const double b0e = b0[e], qae = qa[e];
            double qb;
            if (a.derive) {
                qb = qbn[e];
            } else {
                const double d = Mk[i] - pmk[i];
                qb = b0e + 0.5 * (d * d + V[e]);
                if (on) qbn[e] = qb;
            }
            const double lb = log(qb), ex = qae / qb;
            if (on) exn[e] = ex;                                        // DiagonalGamma.pass_down_Ex  nodes_todo.py:192-193
            sr[u] = on ? lnqa[e] - lb : 0.0;
            sx[u] = on ? psi[e] - lb : 0.0;
            so[u] = on ? cst[e] - a0[e] * lb - b0e * ex : 0.0;
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
#pragma unroll
            for (int u = 0; u < ENTRY_COLS; ++u) {
                sr[u] += __shfl_xor(sr[u], o, 64);
                sx[u] += __shfl_xor(sx[u], o, 64);
                so[u] += __shfl_xor(so[u], o, 64);
            }
        }
        if (lane == 0) {
#pragma unroll
            for (int u = 0; u < ENTRY_COLS; ++u) {
                if (i0 + u < D) { ld_ref[i0 + u] = sr[u]; ld_exact[i0 + u] = sx[u]; own[i0 + u] = so[u]; }
            }
        }
    }
}

int launch_entry(pyvb_lds* h, int which, bool derive) {
    ParamArgs a = make_args(h);
    a.which0 = which == 1 ? 1 : 0; a.derive = derive ? 1 : 0;
    TimedLaunch tl(h, PYVB_K_PARAMS);
    hipLaunchKernelGGL(k_entry, dim3(h->N, which == 2 ? 2 : 1), dim3(64 * ENTRY_WAVES), 0, h->stream, a);
    HIPCHK(hipGetLastError());
    return PYVB_OK;
}

int launch_ard(pyvb_lds* h, int which, bool derive) {
    ParamArgs a = make_args(h);
    a.which0 = which == 1 ? 1 : 0; a.derive = derive ? 1 : 0;
    TimedLaunch tl(h, PYVB_K_PARAMS);
    hipLaunchKernelGGL(k_ard, dim3(h->N, which == 2 ? 2 : 1), dim3(64), 0, h->stream, a);
    HIPCHK(hipGetLastError());
    return PYVB_OK;
}
