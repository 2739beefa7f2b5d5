// k_regressors: known regressors in the output equation (pyvb_lds_create_regressors),
//   Y_t = Gaussian(K, C * X_t + E * Constant(v_t), R),   E = hstack(Es),   t = 0 .. T_n - 1:
// an Addition of two Multiplications (node.py:52-129, :182-276) as the mean parent of the observed Y_t, the columns of E Gaussians
// with Constant parents updated through hstack.pass_up_m1_m2 (nodes_todo.py:43-62).  v_t = 1 is an output offset, v_t = u_t the
// direct feedthrough of an input, anything else a covariate.
//
// With f_t = <E> v_t the message of Y_t to X_t is <C>^T <R> (y_t - f_t): the posterior precisions of the states do not change, and
// the regressors are Pv more output channels with a prescribed gain, behind the 2 P of the inputs (k_inputs.hip),
//   y~_t = [y_t ; u_t ; u_{t+1} ; v_t],   G~ = [G | .. | .. | -Sigma_1 W],   W = <C>^T <R> <E>   [D x Pv],
// and the boundary nodes, which multiply <C>^T <R> y themselves, get the rows -W^T appended to Ct with ones behind the diagonal of
// <R>.  The v_t channel is live in every row t < T_n (zero in padding rows): no end-of-chain case.  k_sweep, k_step and k_stats are
// handed the wider rows and are unchanged.  On y~ the Syx block of k_stats holds Svx = sum_t v_t mu_t^T in its last Pv rows.
// Limit of this route: max(D, K + 2 P + Pv) <= 64.
//
// One wavefront or workgroup per replicate, as in k_inputs.hip:
//   k_rg_assemble  y~ from Y, U and V (when one of them is set);  k_rg_sums  Svv, Syv (when V or Y is set)
//   k_rg_gains     behind k_prep (and k_in_gains): the column group of the v_t channels on v_mfma_f64_16x16x4_f64, their rows of Ct,
//                  the ones behind <R>
//   k_rg_moments   behind k_moments: Svx out of the chunk partials, Syx aside
//   k_rg_HC        H_C = Syx - <E> Svx into the moment block: what the columns of C (k_cols) and the residual of R read
//   k_rg_colsE     [e.update() for e in Es]: G = Svv, H = Syv - <C> Svx^T, row precisions <R>
//   k_rg_resR      the terms of <E> in the residual of R;  k_rg_elbo  the columns of E into part 3 of the bound
#include "params.h"

#define MFMA(a, b, c) __builtin_amdgcn_mfma_f64_16x16x4f64((a), (b), (c), 0, 0, 0)
#define RG_PMAX 63      // Pv <= 63 channels beside K >= 1

struct RgArgs {
    const double *Y, *Uin, *Vin; double* Yt;
    double *Svv, *Syv;
    const double *C_mean, *R_a, *R_b, *Sigma1;      // Sigma1: [N][3][D][D] as k_prep has just written it; class 1 is read
    double *gains, *Ct;
    double *E_mean, *E_var, *qld_E, *lnd_E;
    const double *E_pm, *E_pp, *E_pld;
    const double* part; int nchunk;
    double *mom, *rmom, *resR, *elbo;
    const unsigned char* active;
    const int* len;
    int N, T, D, K, P, Pv, bound;
    Layout L;
};

__device__ __forceinline__ size_t rmom_total(int D, int K, int Pv) { return (size_t)Pv * D + (size_t)K * D; }
#define RMOM_SVX(D, K, Pv) ((size_t)0)
#define RMOM_SYX(D, K, Pv) ((size_t)(Pv) * (D))

// y~_t = [y_t ; u_t ; u_{t+1} ; v_t] for every row of every replicate (setters fill the rows of switched-off replicates too); the
// input channels as k_in_assemble fills them, the v_t channels live in every row of the chain, row 0 included, zero in padding rows.
__global__ void __launch_bounds__(256) k_rg_assemble(RgArgs a) {
    const int n = blockIdx.y, K = a.K, P = a.P, Pv = a.Pv, Kt = K + 2 * P + Pv, T = a.T;
    const int TL = a.len ? a.len[n] : T;
    const size_t total = (size_t)T * Kt;
    const double* Y = a.Y + (size_t)n * T * K;
    const double* U = P ? a.Uin + (size_t)n * T * P : nullptr;
    const double* V = a.Vin + (size_t)n * T * Pv;
    double* Yt = a.Yt + (size_t)n * total;
    for (size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (size_t)gridDim.x * 256) {
        const int t = (int)(idx / Kt), k = (int)(idx % Kt);
        double v;
        if (k < K) v = Y[(size_t)t * K + k];
        else if (k < K + P) v = (t >= 1 && t < TL) ? U[(size_t)t * P + (k - K)] : 0.0;
        else if (k < K + 2 * P) v = (t + 1 < TL) ? U[(size_t)(t + 1) * P + (k - K - P)] : 0.0;
        else v = t < TL ? V[(size_t)t * Pv + (k - K - 2 * P)] : 0.0;
        Yt[idx] = v;
    }
}

// Svv[p][q] = sum_{t<T_n} v_t[p] v_t[q] and Syv[k][p] = sum_{t<T_n} y_t[k] v_t[p], the rows in ascending order into one accumulator
// per entry
__global__ void __launch_bounds__(256) k_rg_sums(RgArgs a) {
    const int n = blockIdx.x, K = a.K, Pv = a.Pv, T = a.T;
    const int TL = a.len ? a.len[n] : T;
    const double* Y = a.Y + (size_t)n * T * K;
    const double* V = a.Vin + (size_t)n * T * Pv;
    for (int idx = threadIdx.x; idx < Pv * Pv + K * Pv; idx += 256) {
        const bool vv = idx < Pv * Pv;
        const int i = (vv ? idx : idx - Pv * Pv) / Pv, p = (vv ? idx : idx - Pv * Pv) % Pv;
        const double* L = vv ? V + i : Y + i;
        const int ls = vv ? Pv : K;
        double s = 0.0;
        for (int t = 0; t < TL; ++t) s += L[(size_t)t * ls] * V[(size_t)t * Pv + p];
        if (vv) a.Svv[(size_t)n * Pv * Pv + idx] = s;
        else a.Syv[(size_t)n * K * Pv + (idx - Pv * Pv)] = s;
    }
}

// Behind k_prep (and k_in_gains), one wavefront per replicate.  <R><E> [K x Pv] goes into LDS (K + Pv <= 64, so K Pv <= 1024),
// W = <C>^T (<R><E>) [D x Pv] into Ws ([DP x 64], zero padded), then Sigma_1 W, as products on the matrix cores, a 16 x 16 result
// tile at a time (once per parameter change, waiting for k_prep's stores, not for arithmetic).  The gain columns are written in
// the operand order the sweep reads (pos_perm), columns K + 2 P .. K + 2 P + Pv - 1 of the block.  k_prep has rewritten the
// diagonal of <R> (zero from K on): the ones go behind it again.  Without inputs nobody else writes Ct: its rows of <C> too.
__global__ void __launch_bounds__(64) k_rg_gains(RgArgs a) {
    __shared__ double RE[1024];
    __shared__ double Ws[64 * 65];
    const int n = blockIdx.x, lane = threadIdx.x, D = a.D, K = a.K, Pv = a.Pv, K0 = a.K + 2 * a.P, r = lane & 15, q = lane >> 4;
    if (!a.active[n]) return;
    const Layout& L = a.L;
    const int DT = L.DT, DS = L.DS, KS = L.KS, PT = (Pv + 15) >> 4;
    double* g = a.gains + (size_t)n * L.gains_total;
    const double* Cm = a.C_mean + (size_t)n * K * D;
    const double* Em = a.E_mean + (size_t)n * K * Pv;
    const double* S1 = a.Sigma1 + ((size_t)n * 3 + 1) * D * D;
    double* Ct = a.Ct + (size_t)n * (K0 + Pv) * D;
    for (int idx = lane; idx < K * Pv; idx += 64) {
        const int k = idx / Pv;
        RE[idx] = a.R_a[(size_t)n * K + k] / a.R_b[(size_t)n * K + k] * Em[idx];
    }
    __syncthreads();
    // W = <C>^T <R><E>: element (i, p) = sum_k C[k][i] RE[k][p]
    for (int m = 0; m < DT; ++m)
        for (int t = 0; t < PT; ++t) {
            d4 acc = d4{0.0, 0.0, 0.0, 0.0};
            for (int s = 0; s < (K + 3) >> 2; ++s) {
                const int k = 4 * s + q, i = 16 * m + r, p = 16 * t + r;
                const double cv = Cm[(size_t)(k < K ? k : K - 1) * D + (i < D ? i : D - 1)];
                const double ev = RE[(k < K ? k : K - 1) * Pv + (p < Pv ? p : Pv - 1)];
                acc = MFMA((k < K && i < D) ? cv : 0.0, (k < K && p < Pv) ? ev : 0.0, acc);
            }
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int i = 16 * m + 4 * e + q, p = 16 * t + r;
                Ws[i * 65 + p] = (i < D && p < Pv) ? acc[e] : 0.0;
            }
        }
    __syncthreads();
    // -Sigma_1 W: the gains of the v_t channels
    for (int m = 0; m < DT; ++m)
        for (int t = 0; t < PT; ++t) {
            d4 acc = d4{0.0, 0.0, 0.0, 0.0};
            for (int s = 0; s < DS; ++s) {
                const int i = 16 * m + r, j = 4 * s + q;
                const double sv = S1[(size_t)(i < D ? i : D - 1) * D + (j < D ? j : D - 1)];
                acc = MFMA((i < D && j < D) ? sv : 0.0, Ws[j * 65 + 16 * t + r], acc);
            }
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int i = 16 * m + 4 * e + q, c = 16 * t + r;
                if (i < D && c < Pv) g[L.oGp + pos_perm(i, K0 + c, KS)] = -acc[e];
            }
        }
    // Ct: -W^T behind the rows of <C> and of the inputs, lane = column j of a row
    if (lane < D) {
        if (!a.P)
            for (int k = 0; k < K; ++k) Ct[(size_t)k * D + lane] = Cm[(size_t)k * D + lane];
        for (int c = 0; c < Pv; ++c) Ct[(size_t)(K0 + c) * D + lane] = -Ws[lane * 65 + c];
    }
    if (lane < Pv) g[L.oqr + 64 + K0 + lane] = 1.0;
}

// Behind k_moments: the rows K + 2 P .. of the Syx partials are Svx; Syx is kept aside, because the moment block's copy is replaced
// by H_C = Syx - <E> Svx before every reader (k_rg_HC).
__global__ void __launch_bounds__(256) k_rg_moments(RgArgs a) {
    const int n = blockIdx.x, tid = threadIdx.x, D = a.D, K = a.K, Pv = a.Pv, K0 = a.K + 2 * a.P, DP = a.L.DP;
    if (!a.active[n]) return;
    const double* Pn = a.part + (size_t)n * a.nchunk * a.L.stats_total + a.L.oSyx;
    double* rm = a.rmom + (size_t)n * rmom_total(D, K, Pv);
    const double* mo = a.mom + (size_t)n * mom_total(D, K);
    for (int idx = tid; idx < Pv * D; idx += 256) {
        const int c = idx / D, j = idx % D;         // channel c of the regressors' block, state dimension j
        double s = 0.0;
        for (int ch = 0; ch < a.nchunk; ++ch) s += Pn[(size_t)ch * a.L.stats_total + (size_t)(K0 + c) * DP + j];
        rm[RMOM_SVX(D, K, Pv) + idx] = s;
    }
    for (int idx = tid; idx < K * D; idx += 256) rm[RMOM_SYX(D, K, Pv) + idx] = mo[MOM_HC(D, K) + idx];
}

__global__ void __launch_bounds__(256) k_rg_HC(RgArgs a) {
    const int n = blockIdx.x, tid = threadIdx.x, D = a.D, K = a.K, Pv = a.Pv;
    if (!a.active[n]) return;
    const double* rm = a.rmom + (size_t)n * rmom_total(D, K, Pv);
    const double* Em = a.E_mean + (size_t)n * K * Pv;
    double* HC = a.mom + (size_t)n * mom_total(D, K) + MOM_HC(D, K);
    for (int idx = tid; idx < K * D; idx += 256) {
        const int k = idx / D, j = idx % D;
        double s = 0.0;
        for (int p = 0; p < Pv; ++p) s += Em[(size_t)k * Pv + p] * rm[RMOM_SVX(D, K, Pv) + (size_t)p * D + j];
        HC[idx] = rm[RMOM_SYX(D, K, Pv) + idx] - s;
    }
}

// [e.update() for e in Es]: Gaussian.update gaussian.py:102-123 fed by hstack.pass_up_m1_m2 nodes_todo.py:43-62, as k_in_colsB does
// it for B -- lane = row k, Gauss-Seidel over the columns -- with G = Svv, H = Syv - <C> Svx^T and the row precisions <R>.
// At Pv = 63 the operands, 63 x 64 + 63 x 63 doubles, are 64 008 B of static LDS.
__global__ void __launch_bounds__(64) k_rg_colsE(RgArgs a) {
    __shared__ double Es[RG_PMAX * 64], Gs[RG_PMAX * RG_PMAX];
    const int n = blockIdx.x, lane = threadIdx.x, D = a.D, K = a.K, Pv = a.Pv;
    if (!a.active[n]) return;
    const bool live = lane < K;
    const int k = live ? lane : K - 1;
    const double* rm = a.rmom + (size_t)n * rmom_total(D, K, Pv);
    const double* Cm = a.C_mean + (size_t)n * K * D + (size_t)k * D;
    const double* Syv = a.Syv + (size_t)n * K * Pv + (size_t)k * Pv;
    double* Em = a.E_mean + (size_t)n * K * Pv + (size_t)k * Pv;
    double* Ev = a.E_var + (size_t)n * Pv * K;
    for (int idx = lane; idx < Pv * Pv; idx += 64) Gs[idx] = a.Svv[(size_t)n * Pv * Pv + idx];
    for (int p = 0; p < Pv; ++p) Es[p * 64 + lane] = live ? Em[p] : 0.0;
    const double lam = a.R_a[(size_t)n * K + k] / a.R_b[(size_t)n * K + k];
    __syncthreads();
    for (int p = 0; p < Pv; ++p) {
        // H[k][p] = Syv[k][p] - sum_j C[k][j] Svx[p][j]
        double h = 0.0;
        const double* sv = rm + RMOM_SVX(D, K, Pv) + (size_t)p * D;
#pragma unroll 8
        for (int j = 0; j < D; ++j) h += Cm[j] * sv[j];
        h = Syv[p] - h;
        double acc = 0.0;
        for (int j = 0; j < Pv; ++j) acc += (j == p ? 0.0 : Es[j * 64 + lane]) * Gs[p * Pv + j];
        const double p0 = a.E_pp[(size_t)p * K + k], m0 = a.E_pm[(size_t)k * Pv + p];
        const double prec = p0 + lam * Gs[p * Pv + p];                              // qprec  gaussian.py:117
        const double var = 1.0 / prec;                                              // qcov   gaussian.py:118-119
        const double val = (p0 * m0 + lam * h - lam * acc) * var;                   // qmu    gaussian.py:119-123
        Es[p * 64 + lane] = live ? val : 0.0;
        if (live) { Em[p] = val; Ev[(size_t)p * K + lane] = var; }
        const double lp = wave_sum(live ? log(prec) : 0.0);                         // q_ln_det gaussian.py:120 (quirk Q1)
        if (lane == 0) { a.qld_E[(size_t)n * Pv + p] = 0.5 / (0.5 * lp); a.lnd_E[(size_t)n * Pv + p] = -lp; }
    }
}

// The residual of R (k_cols, with H_C of the current <E> in the moment block) lacks the terms of <E> alone:
//   1/2 (sum_pj E[k,p] Svv[p,j] E[k,j] + sum_p var_p[k] Svv[p,p]) - sum_p Syv[k,p] E[k,p]      (node.py:121-129, :260-271)
// -- the cross term <C> Svx^T <E>^T and its transpose are what H_C's correction contributes through -diag(H_C <C>^T).
__global__ void __launch_bounds__(64) k_rg_resR(RgArgs a) {
    const int n = blockIdx.x, lane = threadIdx.x, K = a.K, Pv = a.Pv;
    if (!a.active[n] || lane >= K) return;
    const double* Em = a.E_mean + (size_t)n * K * Pv + (size_t)lane * Pv;
    const double* Ev = a.E_var + (size_t)n * Pv * K;
    const double* Syv = a.Syv + (size_t)n * K * Pv + (size_t)lane * Pv;
    const double* G = a.Svv + (size_t)n * Pv * Pv;
    double e = 0.0, hm = 0.0;
    for (int p = 0; p < Pv; ++p) {
        double s = 0.0;
        for (int j = 0; j < Pv; ++j) s += G[p * Pv + j] * Em[j];
        e += Em[p] * s + Ev[(size_t)p * K + lane] * G[p * Pv + p];
        hm += Syv[p] * Em[p];
    }
    a.resR[(size_t)n * K + lane] += 0.5 * e - hm;
}

// The columns of E against their Constant parents (gaussian.py:136-147), lane = column, added to part 3 behind k_elbo
__global__ void __launch_bounds__(64) k_rg_elbo(RgArgs a) {
    const int n = blockIdx.x, lane = threadIdx.x, K = a.K, Pv = a.Pv;
    if (!a.active[n]) return;
    double r = 0.0;
    if (lane < Pv) {
        const double* Em = a.E_mean + (size_t)n * K * Pv + lane;
        const double* Ev = a.E_var + (size_t)n * Pv * K + (size_t)lane * K;
        double tr = 0.0;
        for (int k = 0; k < K; ++k) {
            const double m = Em[(size_t)k * Pv], m0 = a.E_pm[(size_t)k * Pv + lane];
            tr += a.E_pp[(size_t)lane * K + k] * (m * m + Ev[k] + m0 * m0 - 2.0 * m * m0);
        }
        const double ent = (a.bound == PYVB_BOUND_EXACT ? a.lnd_E : a.qld_E)[(size_t)n * Pv + lane];
        r = -0.5 * K * LN2PI + 0.5 * a.E_pld[lane] - 0.5 * tr;
        r += 0.5 * K * LN2PI + 0.5 * ent + 0.5 * K;
    }
    r = wave_sum(r);
    if (lane == 0) a.elbo[(size_t)n * 6 + 3] += r;
}

static RgArgs rg_args(pyvb_lds* h) {
    RgArgs a;
    a.Y = h->Y; a.Uin = h->Uin; a.Vin = h->Vin; a.Yt = h->Yt; a.Svv = h->Svv; a.Syv = h->Syv;
    a.C_mean = h->C_mean; a.R_a = h->R_a; a.R_b = h->R_b; a.Sigma1 = h->Sigma_new;
    a.gains = h->gains; a.Ct = h->Ct;
    a.E_mean = h->E_mean; a.E_var = h->E_var; a.qld_E = h->qld_E; a.lnd_E = h->lnd_E;
    a.E_pm = h->E_pm; a.E_pp = h->E_pp; a.E_pld = h->E_pld;
    a.part = h->stats; a.nchunk = h->nchunk; a.mom = h->mom; a.rmom = h->rmom; a.resR = h->resR; a.elbo = h->elbo;
    a.active = h->active; a.len = h->len;
    a.N = h->N; a.T = h->T; a.D = h->D; a.K = h->K; a.P = h->P; a.Pv = h->Pv; a.bound = h->bound; a.L = h->L;
    return a;
}

int launch_rg_assemble(pyvb_lds* h) {
    const RgArgs a = rg_args(h);
    const size_t total = (size_t)h->T * lds_sweep_K(h), blocks = (total + 255) / 256;
    hipLaunchKernelGGL(k_rg_assemble, dim3((unsigned)(blocks < 1024 ? blocks : 1024), h->N), dim3(256), 0, h->stream, a);
    HIPCHK(hipGetLastError());
    return PYVB_OK;
}

int launch_rg_sums(pyvb_lds* h) {
    const RgArgs a = rg_args(h);
    hipLaunchKernelGGL(k_rg_sums, dim3(h->N), dim3(256), 0, h->stream, a);
    HIPCHK(hipGetLastError());
    return PYVB_OK;
}

#define RG_LAUNCH(kernel, threads, stream_) do { \
    const RgArgs a = rg_args(h); \
    TimedLaunch tl(h, PYVB_K_REGRESSORS, stream_); \
    hipLaunchKernelGGL(kernel, dim3(h->N), dim3(threads), 0, stream_, a); \
    HIPCHK(hipGetLastError()); \
    return PYVB_OK; } while (0)

int launch_rg_gains(pyvb_lds* h) { RG_LAUNCH(k_rg_gains, 64, h->stream); }
int launch_rg_moments(pyvb_lds* h) { RG_LAUNCH(k_rg_moments, 256, h->stream); }
int launch_rg_HC(pyvb_lds* h) { RG_LAUNCH(k_rg_HC, 256, h->stream); }
int launch_rg_colsE(pyvb_lds* h) { RG_LAUNCH(k_rg_colsE, 64, h->stream); }
int launch_rg_resR(pyvb_lds* h) { RG_LAUNCH(k_rg_resR, 64, h->stream); }
int launch_rg_elbo(pyvb_lds* h, hipStream_t stream) { RG_LAUNCH(k_rg_elbo, 64, stream); }
