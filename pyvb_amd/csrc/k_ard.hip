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

int launch_ard(pyvb_lds* h, int which, bool derive) {
    ParamArgs a = make_args(h);
    a.which0 = which == 1 ? 1 : 0; a.derive = derive ? 1 : 0;
    TimedLaunch tl(h, PYVB_K_PARAMS);
    hipLaunchKernelGGL(k_ard, dim3(h->N, which == 2 ? 2 : 1), dim3(64), 0, h->stream, a);
    HIPCHK(hipGetLastError());
    return PYVB_OK;
}
