// k_inputs: a known input that drives the states (pyvb_lds_create_inputs),
//   X_t = Gaussian(q, A * X_{t-1} + B * Constant(u_t), Q),   B = hstack(Bs),   t = 1 .. T-1:
// an Addition of two Multiplications (node.py:52-129, :182-276) as the mean parent of X_t, the columns of B Gaussians with
// Constant parents updated through hstack.pass_up_m1_m2 (nodes_todo.py:43-62).
//
// The sweeps, the single-node update and the statistics pass run unchanged: with e_t = <B> u_t the interior update is
//   mu_t <- F mu_{t-1} + B_gain mu_{t+1} + G y_t + Sigma_1 <Q> e_t - Sigma_1 <A>^T <Q> e_{t+1}  =  F mu_{t-1} + B_gain mu_{t+1} + G~ y~_t,
//   y~_t = [y_t ; u_t ; u_{t+1}],   G~ = [G | Sigma_1 <Q><B> | -Sigma_1 <A>^T<Q><B>],
// so the inputs are 2 P more output channels with a prescribed gain, and those kernels are handed y~ (Yt), K + 2 P and, for the
// two boundary nodes, which multiply <C>^T <R> y themselves, the matrix Ct = [<C> ; (<Q><B>)^T ; -(<A>^T<Q><B>)^T] with ones
// behind the diagonal of <R>: X_0 then adds -<A>^T<Q> e_1 (its u_t channel is zero) and X_{T-1} adds <Q> e_{T-1} (its u_{t+1}
// channel is zero) inside the chain, before the product with Sigma_0 / Sigma_2.  On y~ the Syx block of k_stats comes out as
// [Syx ; Sxu^T ; Su1x]: every new sum, from the present kernel, in one pass.
// Limit of this route: max(D, K + 2 P) <= 64.
//
// What is new is small and latency bound, one wavefront or workgroup per replicate as in k_ard.hip and k_tie.hip:
//   k_in_assemble  y~ from Y and U (when either is set);  k_in_suu  Suu = sum_{t>=1} u_t u_t^T (when U is set)
//   k_in_gains     behind k_prep: the two extra column groups of G~ on v_mfma_f64_16x16x4_f64, Ct, the ones behind <R>
//   k_in_moments   behind k_moments: Sxu, Su1x out of the chunk partials, Sx1x aside
//   k_in_HA        H_A = Sx1x - <B> Su1x into the moment block: what the columns of A (k_cols) and the residual of Q read
//   k_in_colsB     [b.update() for b in Bs]: G = Suu, H = Sxu - <A> Su1x^T, row precisions <Q>
//   k_in_resQ      the terms of <B> in the residual of Q;  k_in_elbo  the columns of B into part 2 of the bound
#include "params.h"

#define MFMA(a, b, c) __builtin_amdgcn_mfma_f64_16x16x4f64((a), (b), (c), 0, 0, 0)
#define IN_PMAX 31      // 2 P <= 62 extra channels beside K >= 1

struct InArgs {
    const double *Y, *Uin; double* Yt;
    double* Suu;
    const double *A_mean, *C_mean, *Q_a, *Q_b, *Sigma1;    // Sigma1: [N][3][D][D] as k_prep has just written it; class 1 is read
    double *gains, *Ct;
    double *B_mean, *B_var, *qld_B, *lnd_B;
    const double *B_pm, *B_pp, *B_pld;
    const double* part; int nchunk;
    double *mom, *imom, *resQ, *elbo;
    const unsigned char* active;
    const int* len;
    int N, T, D, K, P, bound;
    int Pv;     // the regressors' channels behind the 2 P of the inputs (k_regressors.hip): the rows of Ct they add
    Layout L;
};

__device__ __forceinline__ size_t imom_total(int D, int P) { return (size_t)2 * D * P + (size_t)D * D; }
#define IMOM_SXU(D, P) ((size_t)0)
#define IMOM_SU1X(D, P) ((size_t)(D) * (P))
#define IMOM_SX1X(D, P) ((size_t)2 * (D) * (P))

// y~_t = [y_t ; u_t ; u_{t+1}] for every row of every replicate (setters fill the rows of switched-off replicates too); the u_t
// channel is zero in row 0, the u_{t+1} channel from the chain's last row on, and padding rows carry zeros in both.
__global__ void __launch_bounds__(256) k_in_assemble(InArgs a) {
    const int n = blockIdx.y, K = a.K, P = a.P, Kt = K + 2 * P, T = a.T;
    const int TL = a.len ? a.len[n] : T;
    const size_t total = (size_t)T * Kt;
    const double* Y = a.Y + (size_t)n * T * K;
    const double* U = a.Uin + (size_t)n * T * P;
    double* Yt = a.Yt + (size_t)n * total;
    for (size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (size_t)gridDim.x * 256) {
        const int t = (int)(idx / Kt), k = (int)(idx % Kt);
        double v;
        if (k < K) v = Y[(size_t)t * K + k];
        else if (k < K + P) v = (t >= 1 && t < TL) ? U[(size_t)t * P + (k - K)] : 0.0;
        else v = (t + 1 < TL) ? U[(size_t)(t + 1) * P + (k - K - P)] : 0.0;
        Yt[idx] = v;
    }
}

// Suu[p][q] = sum_{t=1}^{T_n-1} u_t[p] u_t[q], the rows in ascending order into one accumulator per entry
__global__ void __launch_bounds__(256) k_in_suu(InArgs a) {
    const int n = blockIdx.x, P = a.P, T = a.T;
    const int TL = a.len ? a.len[n] : T;
    const double* U = a.Uin + (size_t)n * T * P;
    for (int idx = threadIdx.x; idx < P * P; idx += 256) {
        const int p = idx / P, q = idx % P;
        double s = 0.0;
        for (int t = 1; t < TL; ++t) s += U[(size_t)t * P + p] * U[(size_t)t * P + q];
        a.Suu[(size_t)n * P * P + idx] = s;
    }
}

// Behind k_prep, one wavefront per replicate.  W = <Q><B> [D x P] and V = -<A>^T W go side by side into LDS (WV, [DP x 64], zero
// padded), V and then Sigma_1 [W | V] as products on the matrix cores, a 16 x 16 result tile at a time (the operands of a
// k-step come from L2 and LDS; this runs once per parameter change and waits for k_prep's stores, not for arithmetic).
// The gain columns are written in the operand order the sweep reads (pos_perm), columns K .. K + 2 P - 1 of the block
// k_prep filled up to K.  k_prep has rewritten the diagonal of <R> (zero from K on): the ones go behind it again.
__global__ void __launch_bounds__(64) k_in_gains(InArgs a) {
    __shared__ double WV[64 * 65];
    const int n = blockIdx.x, lane = threadIdx.x, D = a.D, K = a.K, P = a.P, r = lane & 15, q = lane >> 4;
    if (!a.active[n]) return;
    const Layout& L = a.L;
    const int DT = L.DT, DS = L.DS, KS = L.KS, CT = (2 * P + 15) >> 4;
    double* g = a.gains + (size_t)n * L.gains_total;
    const double* Am = a.A_mean + (size_t)n * D * D;
    const double* Bm = a.B_mean + (size_t)n * D * P;
    const double* S1 = a.Sigma1 + ((size_t)n * 3 + 1) * D * D;
    double* Ct = a.Ct + (size_t)n * (K + 2 * P + a.Pv) * D;
    const int lc = lane < D ? lane : D - 1;
    const double qbar = lane < D ? a.Q_a[(size_t)n * D + lc] / a.Q_b[(size_t)n * D + lc] : 0.0;
    for (int c = 0; c < 64; ++c) WV[lane * 65 + c] = (lane < D && c < P) ? qbar * Bm[(size_t)lc * P + c] : 0.0;
    __syncthreads();
    // V = -<A>^T W: element (i, p) = -sum_j A[j][i] W[j][p]
    for (int m = 0; m < DT; ++m)
        for (int t = 0; t < (P + 15) >> 4; ++t) {
            d4 acc = d4{0.0, 0.0, 0.0, 0.0};
            for (int s = 0; s < DS; ++s) {
                const int j = 4 * s + q, i = 16 * m + r;
                const double av = Am[(size_t)(j < D ? j : D - 1) * D + (i < D ? i : D - 1)];
                acc = MFMA((j < D && i < D) ? av : 0.0, WV[j * 65 + 16 * t + r], acc);
            }
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int i = 16 * m + 4 * e + q, p = 16 * t + r;
                if (p < P) WV[i * 65 + P + p] = i < D ? -acc[e] : 0.0;
            }
        }
    __syncthreads();
    // Sigma_1 [W | V]: the gains of the u_t and of the u_{t+1} channels
    for (int m = 0; m < DT; ++m)
        for (int t = 0; t < CT; ++t) {
            d4 acc = d4{0.0, 0.0, 0.0, 0.0};
            for (int s = 0; s < DS; ++s) {
                const int i = 16 * m + r, j = 4 * s + q;
                const double sv = S1[(size_t)(i < D ? i : D - 1) * D + (j < D ? j : D - 1)];
                acc = MFMA((i < D && j < D) ? sv : 0.0, WV[j * 65 + 16 * t + r], acc);
            }
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int i = 16 * m + 4 * e + q, c = 16 * t + r;
                if (i < D && c < 2 * P) g[L.oGp + pos_perm(i, K + c, KS)] = acc[e];
            }
        }
    // Ct: <C>, then W^T and V^T, lane = column j of a row
    if (lane < D) {
        const double* Cm = a.C_mean + (size_t)n * K * D;
        for (int k = 0; k < K; ++k) Ct[(size_t)k * D + lane] = Cm[(size_t)k * D + lane];
        for (int c = 0; c < 2 * P; ++c) Ct[(size_t)(K + c) * D + lane] = WV[lane * 65 + c];
    }
    if (lane < 2 * P) g[L.oqr + 64 + K + lane] = 1.0;
}

// Behind k_moments: the rows K .. K + 2 P - 1 of the Syx partials are Sxu^T and Su1x; Sx1x is kept aside, because the moment
// block's copy is replaced by H_A = Sx1x - <B> Su1x before every reader (k_in_HA).
__global__ void __launch_bounds__(256) k_in_moments(InArgs a) {
    const int n = blockIdx.x, tid = threadIdx.x, D = a.D, K = a.K, P = a.P, DP = a.L.DP;
    if (!a.active[n]) return;
    const double* Pn = a.part + (size_t)n * a.nchunk * a.L.stats_total + a.L.oSyx;
    double* im = a.imom + (size_t)n * imom_total(D, P);
    const double* mo = a.mom + (size_t)n * mom_total(D, K);
    for (int idx = tid; idx < 2 * P * D; idx += 256) {
        const int c = idx / D, j = idx % D;         // channel c of the inputs' block, state dimension j
        double s = 0.0;
        for (int ch = 0; ch < a.nchunk; ++ch) s += Pn[(size_t)ch * a.L.stats_total + (size_t)(K + c) * DP + j];
        if (c < P) im[IMOM_SXU(D, P) + (size_t)j * P + c] = s;
        else im[IMOM_SU1X(D, P) + (size_t)(c - P) * D + j] = s;
    }
    for (int idx = tid; idx < D * D; idx += 256) im[IMOM_SX1X(D, P) + idx] = mo[MOM_HA(D, K) + idx];
}

__global__ void __launch_bounds__(256) k_in_HA(InArgs a) {
    const int n = blockIdx.x, tid = threadIdx.x, D = a.D, K = a.K, P = a.P;
    if (!a.active[n]) return;
    const double* im = a.imom + (size_t)n * imom_total(D, P);
    const double* Bm = a.B_mean + (size_t)n * D * P;
    double* HA = a.mom + (size_t)n * mom_total(D, K) + MOM_HA(D, K);
    for (int idx = tid; idx < D * D; idx += 256) {
        const int i = idx / D, j = idx % D;
        double s = 0.0;
        for (int p = 0; p < P; ++p) s += Bm[(size_t)i * P + p] * im[IMOM_SU1X(D, P) + (size_t)p * D + j];
        HA[idx] = im[IMOM_SX1X(D, P) + idx] - s;
    }
}

// [b.update() for b in Bs]: Gaussian.update gaussian.py:102-123 fed by hstack.pass_up_m1_m2 nodes_todo.py:43-62, as k_cols does it
// for A -- lane = row k, Gauss-Seidel over the columns -- with G = Suu, H = Sxu - <A> Su1x^T and the row precisions <Q>.  There
// are at most 31 columns, each a chain of at most 30 multiply-adds per lane behind the one before: no MFMA blocking (k_cols
// blocks 64 columns by 16 to take the products with the old columns out of the chain; here that product is the chain).
__global__ void __launch_bounds__(64) k_in_colsB(InArgs a) {
    __shared__ double Bs[IN_PMAX * 64], Gs[IN_PMAX * IN_PMAX];
    const int n = blockIdx.x, lane = threadIdx.x, D = a.D, P = a.P;
    if (!a.active[n]) return;
    const bool live = lane < D;
    const int k = live ? lane : D - 1;
    const double* im = a.imom + (size_t)n * imom_total(D, P);
    const double* Am = a.A_mean + (size_t)n * D * D + (size_t)k * D;
    double* Bm = a.B_mean + (size_t)n * D * P + (size_t)k * P;
    double* Bv = a.B_var + (size_t)n * P * D;
    for (int idx = lane; idx < P * P; idx += 64) Gs[idx] = a.Suu[(size_t)n * P * P + idx];
    for (int p = 0; p < P; ++p) Bs[p * 64 + lane] = live ? Bm[p] : 0.0;
    const double lam = a.Q_a[(size_t)n * D + k] / a.Q_b[(size_t)n * D + k];
    __syncthreads();
    for (int p = 0; p < P; ++p) {
        // H[k][p] = Sxu[k][p] - sum_j A[k][j] Su1x[p][j]
        double h = 0.0;
        const double* su = im + IMOM_SU1X(D, P) + (size_t)p * D;
#pragma unroll 8
        for (int j = 0; j < D; ++j) h += Am[j] * su[j];
        h = im[IMOM_SXU(D, P) + (size_t)k * P + p] - h;
        double acc = 0.0;
        for (int j = 0; j < P; ++j) acc += (j == p ? 0.0 : Bs[j * 64 + lane]) * Gs[p * P + j];
        const double p0 = a.B_pp[(size_t)p * D + k], m0 = a.B_pm[(size_t)k * P + p];
        const double prec = p0 + lam * Gs[p * P + p];                               // qprec  gaussian.py:117
        const double var = 1.0 / prec;                                              // qcov   gaussian.py:118-119
        const double val = (p0 * m0 + lam * h - lam * acc) * var;                   // qmu    gaussian.py:119-123
        Bs[p * 64 + lane] = live ? val : 0.0;
        if (live) { Bm[p] = val; Bv[(size_t)p * D + lane] = var; }
        const double lp = wave_sum(live ? log(prec) : 0.0);                         // q_ln_det gaussian.py:120 (quirk Q1)
        if (lane == 0) { a.qld_B[(size_t)n * P + p] = 0.5 / (0.5 * lp); a.lnd_B[(size_t)n * P + p] = -lp; }
    }
}

// The residual of Q (k_cols, with H_A of the current <B> in the moment block) lacks the terms of <B> alone:
//   1/2 (sum_pj B[k,p] Suu[p,j] B[k,j] + sum_p var_p[k] Suu[p,p]) - sum_p Sxu[k,p] B[k,p]      (node.py:121-129, :260-271)
// -- the cross term <A> Su1x^T <B>^T and its transpose are what H_A's correction contributes through -diag(H_A <A>^T).
__global__ void __launch_bounds__(64) k_in_resQ(InArgs a) {
    const int n = blockIdx.x, lane = threadIdx.x, D = a.D, P = a.P;
    if (!a.active[n] || lane >= D) return;
    const double* im = a.imom + (size_t)n * imom_total(D, P);
    const double* Bm = a.B_mean + (size_t)n * D * P + (size_t)lane * P;
    const double* Bv = a.B_var + (size_t)n * P * D;
    const double* G = a.Suu + (size_t)n * P * P;
    double e = 0.0, hm = 0.0;
    for (int p = 0; p < P; ++p) {
        double s = 0.0;
        for (int j = 0; j < P; ++j) s += G[p * P + j] * Bm[j];
        e += Bm[p] * s + Bv[(size_t)p * D + lane] * G[p * P + p];
        hm += im[IMOM_SXU(D, P) + (size_t)lane * P + p] * Bm[p];
    }
    a.resQ[(size_t)n * D + lane] += 0.5 * e - hm;
}

// The columns of B against their Constant parents (gaussian.py:136-147), lane = column, added to part 2 behind k_elbo
__global__ void __launch_bounds__(64) k_in_elbo(InArgs a) {
    const int n = blockIdx.x, lane = threadIdx.x, D = a.D, P = a.P;
    if (!a.active[n]) return;
    double r = 0.0;
    if (lane < P) {
        const double* Bm = a.B_mean + (size_t)n * D * P + lane;
        const double* Bv = a.B_var + (size_t)n * P * D + (size_t)lane * D;
        double tr = 0.0;
        for (int k = 0; k < D; ++k) {
            const double m = Bm[(size_t)k * P], m0 = a.B_pm[(size_t)k * P + lane];
            tr += a.B_pp[(size_t)lane * D + k] * (m * m + Bv[k] + m0 * m0 - 2.0 * m * m0);
        }
        const double ent = (a.bound == PYVB_BOUND_EXACT ? a.lnd_B : a.qld_B)[(size_t)n * P + lane];
        r = -0.5 * D * LN2PI + 0.5 * a.B_pld[lane] - 0.5 * tr;
        r += 0.5 * D * LN2PI + 0.5 * ent + 0.5 * D;
    }
    r = wave_sum(r);
    if (lane == 0) a.elbo[(size_t)n * 6 + 2] += r;
}

static InArgs in_args(pyvb_lds* h) {
    InArgs a;
    a.Y = h->Y; a.Uin = h->Uin; a.Yt = h->Yt; a.Suu = h->Suu;
    a.A_mean = h->A_mean; a.C_mean = h->C_mean; a.Q_a = h->Q_a; a.Q_b = h->Q_b; a.Sigma1 = h->Sigma_new;
    a.gains = h->gains; a.Ct = h->Ct;
    a.B_mean = h->B_mean; a.B_var = h->B_var; a.qld_B = h->qld_B; a.lnd_B = h->lnd_B;
    a.B_pm = h->B_pm; a.B_pp = h->B_pp; a.B_pld = h->B_pld;
    a.part = h->stats; a.nchunk = h->nchunk; a.mom = h->mom; a.imom = h->imom; a.resQ = h->resQ; a.elbo = h->elbo;
    a.active = h->active; a.len = h->len;
    a.N = h->N; a.T = h->T; a.D = h->D; a.K = h->K; a.P = h->P; a.Pv = h->Pv; a.bound = h->bound; a.L = h->L;
    return a;
}

int launch_in_assemble(pyvb_lds* h) {
    const InArgs a = in_args(h);
    const size_t total = (size_t)h->T * lds_sweep_K(h), blocks = (total + 255) / 256;
    hipLaunchKernelGGL(k_in_assemble, dim3((unsigned)(blocks < 1024 ? blocks : 1024), h->N), dim3(256), 0, h->stream, a);
    HIPCHK(hipGetLastError());
    return PYVB_OK;
}

int launch_in_suu(pyvb_lds* h) {
    const InArgs a = in_args(h);
    hipLaunchKernelGGL(k_in_suu, dim3(h->N), dim3(256), 0, h->stream, a);
    HIPCHK(hipGetLastError());
    return PYVB_OK;
}

#define IN_LAUNCH(kernel, threads, stream_, timer) do { \
    const InArgs a = in_args(h); \
    TimedLaunch tl(h, timer, stream_); \
    hipLaunchKernelGGL(kernel, dim3(h->N), dim3(threads), 0, stream_, a); \
    HIPCHK(hipGetLastError()); \
    return PYVB_OK; } while (0)

int launch_in_gains(pyvb_lds* h) { IN_LAUNCH(k_in_gains, 64, h->stream, PYVB_K_INPUTS); }
int launch_in_moments(pyvb_lds* h) { IN_LAUNCH(k_in_moments, 256, h->stream, PYVB_K_INPUTS); }
int launch_in_HA(pyvb_lds* h) { IN_LAUNCH(k_in_HA, 256, h->stream, PYVB_K_INPUTS); }
int launch_in_colsB(pyvb_lds* h) { IN_LAUNCH(k_in_colsB, 64, h->stream, PYVB_K_INPUTS); }
int launch_in_resQ(pyvb_lds* h) { IN_LAUNCH(k_in_resQ, 64, h->stream, PYVB_K_INPUTS); }
int launch_in_elbo(pyvb_lds* h, hipStream_t stream) { IN_LAUNCH(k_in_elbo, 64, stream, PYVB_K_INPUTS); }
