// k_known: known channels with an unknown gain in either equation of the model (KnownChannels, common.h).
//   side 0, pyvb_lds_create_inputs:      X_t = Gaussian(q, A * X_{t-1} + B * Constant(u_t), Q),   B = hstack(Bs),   t = 1 .. T_n - 1
//   side 1, pyvb_lds_create_regressors:  Y_t = Gaussian(K, C * X_t + E * Constant(v_t), R),       E = hstack(Es),   t = 0 .. T_n - 1
// each an Addition of two Multiplications (node.py:52-129, :182-276) as the mean parent, the columns of the gain Gaussians with
// Constant parents updated through hstack.pass_up_m1_m2 (nodes_todo.py:43-62).  v_t = 1 is an output offset, v_t = u_t the direct
// feedthrough of an input, anything else a covariate.  The two sides are one set of kernels under the substitution
//   D, P, A, B, Q, Suu, Sxu, Su1x, Sx1x, H_A, part 2   <->   K, Pv, C, E, R, Svv, Syv, Svx, Syx, H_C, part 3
// which known_args makes from the side's index: KnownArgs carries the side's record, its row count and what it is attached to.
//
// The sweeps, the single-node update and the statistics pass run unchanged.  With e_t = <B> u_t and f_t = <E> v_t the interior
// update is
//   mu_t <- F mu_{t-1} + B_gain mu_{t+1} + G (y_t - f_t) + Sigma_1 <Q> e_t - Sigma_1 <A>^T <Q> e_{t+1}  =  F mu_{t-1} + B_gain mu_{t+1} + G~ y~_t,
//   y~_t = [y_t ; u_t ; u_{t+1} ; v_t],   G~ = [G | Sigma_1 <Q><B> | -Sigma_1 <A>^T<Q><B> | -Sigma_1 <C>^T<R><E>],
// (the posterior precisions of the states do not change), so the channels are 2 P + Pv more output channels with a prescribed
// gain, and those kernels are handed y~ (Yt), K + 2 P + Pv and, for the two boundary nodes, which multiply <C>^T <R> y themselves,
// the matrix Ct = [<C> ; (<Q><B>)^T ; -(<A>^T<Q><B>)^T ; -(<C>^T<R><E>)^T] with ones behind the diagonal of <R>: X_0 then adds
// -<A>^T<Q> e_1 (its u_t channel is zero) and X_{T-1} adds <Q> e_{T-1} (its u_{t+1} channel is zero) inside the chain, before the
// product with Sigma_0 / Sigma_2.  The v_t channel is live in every row t < T_n: no end-of-chain case.  On y~ the Syx block of
// k_stats comes out as [Syx ; Sxu^T ; Su1x ; Svx]: every sum against the states, from the present kernel, in one pass.
// Limit of this route: max(D, K + 2 P + Pv) <= 64.
//
// What is here is small and latency bound, one wavefront or workgroup per replicate as in k_ard.hip and k_tie.hip:
//   k_known_assemble       y~ from Y, U and V (when one of them is set)
//   k_known_gram           Suu (when U is set) / Svv, Syv (when V or Y is set)
//   k_in_gains, k_rg_gains behind k_prep, in this order: the side's column groups of G~ on v_mfma_f64_16x16x4_f64, its rows of Ct,
//                          the ones behind <R>.  The two differ in the product that forms the block Sigma_1 multiplies.
//   k_known_moments        behind k_moments: the cross sums against the states out of the chunk partials, Sx1x / Syx aside
//   k_known_H              H_A = Sx1x - <B> Su1x / H_C = Syx - <E> Svx into the moment block: what the columns of A / C (k_cols) and
//                          the residual of Q / R read
//   k_known_cols           [b.update() for b in Bs]: G = Suu, H = Sxu - <A> Su1x^T, row precisions <Q>, and the same for Es
//   k_known_resid          the terms of the gain alone in the residual of Q / R
//   k_known_elbo           the columns of the gain into part 2 / 3 of the bound
#include "params.h"

#define MFMA(a, b, c) __builtin_amdgcn_mfma_f64_16x16x4f64((a), (b), (c), 0, 0, 0)
#define IN_PMAX 31      // 2 P <= 62 extra channels beside K >= 1
#define RG_PMAX 63      // Pv <= 63 channels beside K >= 1

struct KnownArgs {
    // the side the kernel runs for: its record (KnownChannels), and what its index attaches it to
    int side, rows, width;                      // rows: D / K
    const double* in;
    double *mean, *var, *qld, *lnd;
    const double *pm, *pp, *pld;
    double *gram, *cross_lhs, *cross_x, *saved;
    const double *M_mean, *noise_a, *noise_b;   // <A>, Q_a, Q_b / <C>, R_a, R_b
    double* res;                                // resQ / resR
    size_t mom_H;                               // MOM_HA / MOM_HC
    int part;                                   // 2 / 3
    // the handle: both sides' channels for y~, and where the side's columns stand in the gains and in Ct
    const double *Y, *Uin, *Vin; double* Yt;
    const double *C_mean, *Sigma1;              // Sigma1: [N][3][D][D] as k_prep has just written it; class 1 is read
    double *gains, *Ct;
    const double* stats; int nchunk;
    double *mom, *elbo;
    const unsigned char* active;
    const int* len;
    int N, T, D, K, P, Pv, bound;
    Layout L;
};

// y~_t = [y_t ; u_t ; u_{t+1} ; v_t] for every row of every replicate (setters fill the rows of switched-off replicates too); the
// u_t channel is zero in row 0, the u_{t+1} channel from the chain's last row on, the v_t channels are live in every row of the
// chain, row 0 included, and padding rows carry zeros in all three.
__global__ void __launch_bounds__(256) k_known_assemble(KnownArgs a) {
    const int n = blockIdx.y, K = a.K, P = a.P, Pv = a.Pv, Kt = K + 2 * P + Pv, T = a.T;
    const int TL = a.len ? a.len[n] : T;
    const size_t total = (size_t)T * Kt;
    const double* Y = a.Y + (size_t)n * T * K;
    const double* U = P ? a.Uin + (size_t)n * T * P : nullptr;
    const double* V = Pv ? a.Vin + (size_t)n * T * Pv : nullptr;
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

// gram[p][q] = sum_t w_t[p] w_t[q] over the rows the channels w act in (side 0: t = 1 .. T_n - 1, side 1: t = 0 .. T_n - 1) and, on
// side 1, Syv[k][p] = sum_t y_t[k] v_t[p] (Sxu comes from the statistics pass): the rows in ascending order into one accumulator
// per entry
__global__ void __launch_bounds__(256) k_known_gram(KnownArgs a) {
    const int n = blockIdx.x, K = a.K, W = a.width, T = a.T;
    const int TL = a.len ? a.len[n] : T;
    const double* Y = a.Y + (size_t)n * T * K;
    const double* V = a.in + (size_t)n * T * W;
    for (int idx = threadIdx.x; idx < W * W + (a.side ? K * W : 0); idx += 256) {
        const bool vv = idx < W * W;
        const int i = (vv ? idx : idx - W * W) / W, p = (vv ? idx : idx - W * W) % W;
        const double* L = vv ? V + i : Y + i;
        const int ls = vv ? W : K;
        double s = 0.0;
        for (int t = 1 - a.side; t < TL; ++t) s += L[(size_t)t * ls] * V[(size_t)t * W + p];
        if (vv) a.gram[(size_t)n * W * W + idx] = s;
        else a.cross_lhs[(size_t)n * K * W + (idx - W * W)] = s;
    }
}

// The part the two gains kernels share, one wavefront per replicate: Sigma_1 times the block in LDS (Ws, [DP x 64] at stride 65, zero
// padded, ncol real columns) as products on the matrix cores, a 16 x 16 result tile at a time, written (NEG: negated) as the gain
// columns col0 .. col0 + ncol - 1 in the operand order the sweep reads (pos_perm); the block's transpose as the rows col0 .. of Ct
// behind <C> (with_C: and the rows of <C>, which nobody else writes), lane = column j of a row; k_prep has rewritten the diagonal
// of <R> (zero from K on): the ones go behind it again.
template <bool NEG>
__device__ __forceinline__ void known_gain_columns(const KnownArgs& a, const double* Ws, int ncol, int col0, bool with_C) {
    const int n = blockIdx.x, lane = threadIdx.x, D = a.D, K = a.K, r = lane & 15, q = lane >> 4;
    const Layout& L = a.L;
    const int DT = L.DT, DS = L.DS, KS = L.KS, CT = (ncol + 15) >> 4;
    double* g = a.gains + (size_t)n * L.gains_total;
    const double* S1 = a.Sigma1 + ((size_t)n * 3 + 1) * D * D;
    double* Ct = a.Ct + (size_t)n * (K + 2 * a.P + a.Pv) * D;
    for (int m = 0; m < DT; ++m)
        for (int t = 0; t < CT; ++t) {
            d4 acc = d4{0.0, 0.0, 0.0, 0.0};
            for (int s = 0; s < DS; ++s) {
                const int i = 16 * m + r, j = 4 * s + q;
                const double sv = S1[(size_t)(i < D ? i : D - 1) * D + (j < D ? j : D - 1)];
                acc = MFMA((i < D && j < D) ? sv : 0.0, Ws[j * 65 + 16 * t + r], acc);
            }
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int i = 16 * m + 4 * e + q, c = 16 * t + r;
                if (i < D && c < ncol) g[L.oGp + pos_perm(i, col0 + c, KS)] = NEG ? -acc[e] : acc[e];
            }
        }
    if (lane < D) {
        if (with_C) {
            const double* Cm = a.C_mean + (size_t)n * K * D;
            for (int k = 0; k < K; ++k) Ct[(size_t)k * D + lane] = Cm[(size_t)k * D + lane];
        }
        for (int c = 0; c < ncol; ++c) Ct[(size_t)(col0 + c) * D + lane] = NEG ? -Ws[lane * 65 + c] : Ws[lane * 65 + c];
    }
    if (lane < ncol) g[L.oqr + 64 + col0 + lane] = 1.0;
}

// Behind k_prep.  W = <Q><B> [D x P] and V = -<A>^T W go side by side into LDS (WV, [DP x 64], zero padded), V as a product on the
// matrix cores (the operands of a k-step come from L2 and LDS; this runs once per parameter change and waits for k_prep's stores,
// not for arithmetic); Sigma_1 [W | V] are the gains of the u_t and of the u_{t+1} channels, columns K .. K + 2 P - 1 of the block
// k_prep filled up to K.
__global__ void __launch_bounds__(64) k_in_gains(KnownArgs a) {
    __shared__ double WV[64 * 65];
    const int n = blockIdx.x, lane = threadIdx.x, D = a.D, P = a.P, r = lane & 15, q = lane >> 4;
    if (!a.active[n]) return;
    const int DT = a.L.DT, DS = a.L.DS;
    const double* Am = a.M_mean + (size_t)n * D * D;
    const double* Bm = a.mean + (size_t)n * D * P;
    const int lc = lane < D ? lane : D - 1;
    const double qbar = lane < D ? a.noise_a[(size_t)n * D + lc] / a.noise_b[(size_t)n * D + lc] : 0.0;
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
    known_gain_columns<false>(a, WV, 2 * P, a.K, true);
}

// Behind k_prep (and k_in_gains).  <R><E> [K x Pv] goes into LDS (K + Pv <= 64, so K Pv <= 1024), W = <C>^T (<R><E>) [D x Pv] into
// Ws ([DP x 64], zero padded) as a product on the matrix cores; -Sigma_1 W are the gains of the v_t channels, columns
// K + 2 P .. K + 2 P + Pv - 1 of the block.  Without inputs nobody else writes Ct: its rows of <C> too.
__global__ void __launch_bounds__(64) k_rg_gains(KnownArgs a) {
    __shared__ double RE[1024];
    __shared__ double Ws[64 * 65];
    const int n = blockIdx.x, lane = threadIdx.x, D = a.D, K = a.K, Pv = a.Pv, r = lane & 15, q = lane >> 4;
    if (!a.active[n]) return;
    const int DT = a.L.DT, PT = (Pv + 15) >> 4;
    const double* Cm = a.M_mean + (size_t)n * K * D;
    const double* Em = a.mean + (size_t)n * K * Pv;
    for (int idx = lane; idx < K * Pv; idx += 64) {
        const int k = idx / Pv;
        RE[idx] = a.noise_a[(size_t)n * K + k] / a.noise_b[(size_t)n * K + k] * Em[idx];
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
    known_gain_columns<true>(a, Ws, Pv, K + 2 * a.P, !a.P);
}

// Behind k_moments: the last rows of the Syx partials are the side's sums against the states -- from K on Sxu^T and Su1x, from
// K + 2 P on Svx; Sx1x / Syx is kept aside, because the moment block's copy is replaced by H_A / H_C before every reader (k_known_H).
__global__ void __launch_bounds__(256) k_known_moments(KnownArgs a) {
    const int n = blockIdx.x, tid = threadIdx.x, D = a.D, K = a.K, P = a.P, W = a.width, DP = a.L.DP;
    if (!a.active[n]) return;
    const double* Pn = a.stats + (size_t)n * a.nchunk * a.L.stats_total + a.L.oSyx;
    const int c0 = K + (a.side ? 2 * P : P);        // the first row of u_{t+1} / v_t
    double* cx = a.cross_x + (size_t)n * W * D;
    for (int idx = tid; idx < W * D; idx += 256) {
        const int c = idx / D, j = idx % D;         // channel c of the side, state dimension j
        double s = 0.0;
        for (int ch = 0; ch < a.nchunk; ++ch) s += Pn[(size_t)ch * a.L.stats_total + (size_t)(c0 + c) * DP + j];
        cx[idx] = s;
    }
    if (!a.side) {      // the rows of u_t hold Sxu^T (Syv is formed from Y and V, k_known_gram)
        double* sl = a.cross_lhs + (size_t)n * D * P;
        for (int idx = tid; idx < P * D; idx += 256) {
            const int c = idx / D, j = idx % D;
            double s = 0.0;
            for (int ch = 0; ch < a.nchunk; ++ch) s += Pn[(size_t)ch * a.L.stats_total + (size_t)(K + c) * DP + j];
            sl[(size_t)j * P + c] = s;
        }
    }
    double* sv = a.saved + (size_t)n * a.rows * D;
    const double* mo = a.mom + (size_t)n * mom_total(D, K) + a.mom_H;
    for (int idx = tid; idx < a.rows * D; idx += 256) sv[idx] = mo[idx];
}

__global__ void __launch_bounds__(256) k_known_H(KnownArgs a) {
    const int n = blockIdx.x, tid = threadIdx.x, D = a.D, R = a.rows, W = a.width;
    if (!a.active[n]) return;
    const double* cx = a.cross_x + (size_t)n * W * D;
    const double* sv = a.saved + (size_t)n * R * D;
    const double* Gm = a.mean + (size_t)n * R * W;
    double* H = a.mom + (size_t)n * mom_total(D, a.K) + a.mom_H;
    for (int idx = tid; idx < R * D; idx += 256) {
        const int i = idx / D, j = idx % D;
        double s = 0.0;
        for (int p = 0; p < W; ++p) s += Gm[(size_t)i * W + p] * cx[(size_t)p * D + j];
        H[idx] = sv[idx] - s;
    }
}

// [b.update() for b in Bs], [e.update() for e in Es]: Gaussian.update gaussian.py:102-123 fed by hstack.pass_up_m1_m2
// nodes_todo.py:43-62, as k_cols does it for A -- lane = row k, Gauss-Seidel over the columns -- with G = Suu, H = Sxu - <A> Su1x^T
// and the row precisions <Q> (G = Svv, H = Syv - <C> Svx^T, <R>).  Each column is a chain of at most PMAX - 1 multiply-adds per lane
// behind the one before: no MFMA blocking (k_cols blocks 64 columns by 16 to take the products with the old columns out of the
// chain; here that product is the chain).  The operands are static LDS, PMAX x 64 + PMAX x PMAX doubles: 23.6 KB at IN_PMAX and
// 64 008 B at RG_PMAX, which is why PMAX is the side's own and not the larger of the two.
template <int PMAX>
__global__ void __launch_bounds__(64) k_known_cols(KnownArgs a) {
    __shared__ double Bs[PMAX * 64], Gs[PMAX * PMAX];
    const int n = blockIdx.x, lane = threadIdx.x, D = a.D, R = a.rows, P = a.width;
    if (!a.active[n]) return;
    const bool live = lane < R;
    const int k = live ? lane : R - 1;
    const double* cx = a.cross_x + (size_t)n * P * D;
    const double* Mm = a.M_mean + (size_t)n * R * D + (size_t)k * D;
    const double* Sl = a.cross_lhs + (size_t)n * R * P + (size_t)k * P;
    double* Bm = a.mean + (size_t)n * R * P + (size_t)k * P;
    double* Bv = a.var + (size_t)n * P * R;
    for (int idx = lane; idx < P * P; idx += 64) Gs[idx] = a.gram[(size_t)n * P * P + idx];
    for (int p = 0; p < P; ++p) Bs[p * 64 + lane] = live ? Bm[p] : 0.0;
    const double lam = a.noise_a[(size_t)n * R + k] / a.noise_b[(size_t)n * R + k];
    __syncthreads();
    for (int p = 0; p < P; ++p) {
        // H[k][p] = Sxu[k][p] - sum_j A[k][j] Su1x[p][j]
        double h = 0.0;
        const double* su = cx + (size_t)p * D;
#pragma unroll 8
        for (int j = 0; j < D; ++j) h += Mm[j] * su[j];
        h = Sl[p] - h;
        double acc = 0.0;
        for (int j = 0; j < P; ++j) acc += (j == p ? 0.0 : Bs[j * 64 + lane]) * Gs[p * P + j];
        const double p0 = a.pp[(size_t)p * R + k], m0 = a.pm[(size_t)k * P + p];
        const double prec = p0 + lam * Gs[p * P + p];                               // qprec  gaussian.py:117
        const double var = 1.0 / prec;                                              // qcov   gaussian.py:118-119
        const double val = (p0 * m0 + lam * h - lam * acc) * var;                   // qmu    gaussian.py:119-123
        Bs[p * 64 + lane] = live ? val : 0.0;
        if (live) { Bm[p] = val; Bv[(size_t)p * R + lane] = var; }
        const double lp = wave_sum(live ? log(prec) : 0.0);                         // q_ln_det gaussian.py:120 (quirk Q1)
        if (lane == 0) { a.qld[(size_t)n * P + p] = 0.5 / (0.5 * lp); a.lnd[(size_t)n * P + p] = -lp; }
    }
}

// The residual of Q (k_cols, with H_A of the current <B> in the moment block) lacks the terms of <B> alone:
//   1/2 (sum_pj B[k,p] Suu[p,j] B[k,j] + sum_p var_p[k] Suu[p,p]) - sum_p Sxu[k,p] B[k,p]      (node.py:121-129, :260-271)
// -- the cross term <A> Su1x^T <B>^T and its transpose are what H_A's correction contributes through -diag(H_A <A>^T).  The
// residual of R, <E>, Svv, Syv and H_C likewise.
__global__ void __launch_bounds__(64) k_known_resid(KnownArgs a) {
    const int n = blockIdx.x, lane = threadIdx.x, R = a.rows, P = a.width;
    if (!a.active[n] || lane >= R) return;
    const double* Bm = a.mean + (size_t)n * R * P + (size_t)lane * P;
    const double* Bv = a.var + (size_t)n * P * R;
    const double* Sl = a.cross_lhs + (size_t)n * R * P + (size_t)lane * P;
    const double* G = a.gram + (size_t)n * P * P;
    double e = 0.0, hm = 0.0;
    for (int p = 0; p < P; ++p) {
        double s = 0.0;
        for (int j = 0; j < P; ++j) s += G[p * P + j] * Bm[j];
        e += Bm[p] * s + Bv[(size_t)p * R + lane] * G[p * P + p];
        hm += Sl[p] * Bm[p];
    }
    a.res[(size_t)n * R + lane] += 0.5 * e - hm;
}

// The columns of the gain against their Constant parents (gaussian.py:136-147), lane = column, added to the side's part behind k_elbo
__global__ void __launch_bounds__(64) k_known_elbo(KnownArgs a) {
    const int n = blockIdx.x, lane = threadIdx.x, R = a.rows, P = a.width;
    if (!a.active[n]) return;
    double r = 0.0;
    if (lane < P) {
        const double* Bm = a.mean + (size_t)n * R * P + lane;
        const double* Bv = a.var + (size_t)n * P * R + (size_t)lane * R;
        double tr = 0.0;
        for (int k = 0; k < R; ++k) {
            const double m = Bm[(size_t)k * P], m0 = a.pm[(size_t)k * P + lane];
            tr += a.pp[(size_t)lane * R + k] * (m * m + Bv[k] + m0 * m0 - 2.0 * m * m0);
        }
        const double ent = (a.bound == PYVB_BOUND_EXACT ? a.lnd : a.qld)[(size_t)n * P + lane];
        r = -0.5 * R * LN2PI + 0.5 * a.pld[lane] - 0.5 * tr;
        r += 0.5 * R * LN2PI + 0.5 * ent + 0.5 * R;
    }
    r = wave_sum(r);
    if (lane == 0) a.elbo[(size_t)n * 6 + a.part] += r;
}

// the side's record, and from its index what it is attached to
static KnownArgs known_args(pyvb_lds* h, int side) {
    const KnownChannels& k = h->known[side];
    KnownArgs a;
    a.side = side; a.rows = lds_known_rows(h, side); a.width = k.width;
    a.in = k.in; a.mean = k.mean; a.var = k.var; a.qld = k.qld; a.lnd = k.lnd; a.pm = k.pm; a.pp = k.pp; a.pld = k.pld;
    a.gram = k.gram; a.cross_lhs = k.cross_lhs; a.cross_x = k.cross_x; a.saved = k.saved;
    a.M_mean = side ? h->C_mean : h->A_mean; a.noise_a = side ? h->R_a : h->Q_a; a.noise_b = side ? h->R_b : h->Q_b;
    a.res = side ? h->resR : h->resQ; a.mom_H = side ? MOM_HC(h->D, h->K) : MOM_HA(h->D, h->K); a.part = 2 + side;
    a.Y = h->Y; a.Uin = h->known[0].in; a.Vin = h->known[1].in; a.Yt = h->Yt;
    a.C_mean = h->C_mean; a.Sigma1 = h->Sigma_new; a.gains = h->gains; a.Ct = h->Ct;
    a.stats = h->stats; a.nchunk = h->nchunk; a.mom = h->mom; a.elbo = h->elbo;
    a.active = h->active; a.len = h->len;
    a.N = h->N; a.T = h->T; a.D = h->D; a.K = h->K; a.P = h->known[0].width; a.Pv = h->known[1].width; a.bound = h->bound; a.L = h->L;
    return a;
}

int launch_known_assemble(pyvb_lds* h) {
    const KnownArgs a = known_args(h, 0);
    const size_t total = (size_t)h->T * lds_sweep_K(h), blocks = (total + 255) / 256;
    hipLaunchKernelGGL(k_known_assemble, dim3((unsigned)(blocks < 1024 ? blocks : 1024), h->N), dim3(256), 0, h->stream, a);
    HIPCHK(hipGetLastError());
    return PYVB_OK;
}

int launch_known_gram(pyvb_lds* h, int side) {
    const KnownArgs a = known_args(h, side);
    hipLaunchKernelGGL(k_known_gram, dim3(h->N), dim3(256), 0, h->stream, a);
    HIPCHK(hipGetLastError());
    return PYVB_OK;
}

#define KNOWN_LAUNCH(kernel, threads, stream_) do { \
    const KnownArgs a = known_args(h, side); \
    TimedLaunch tl(h, side ? PYVB_K_REGRESSORS : PYVB_K_INPUTS, stream_); \
    hipLaunchKernelGGL(kernel, dim3(h->N), dim3(threads), 0, stream_, a); \
    HIPCHK(hipGetLastError()); \
    return PYVB_OK; } while (0)

int launch_known_gains(pyvb_lds* h, int side) { if (side) KNOWN_LAUNCH(k_rg_gains, 64, h->stream); KNOWN_LAUNCH(k_in_gains, 64, h->stream); }
int launch_known_moments(pyvb_lds* h, int side) { KNOWN_LAUNCH(k_known_moments, 256, h->stream); }
int launch_known_H(pyvb_lds* h, int side) { KNOWN_LAUNCH(k_known_H, 256, h->stream); }
int launch_known_cols(pyvb_lds* h, int side) { if (side) KNOWN_LAUNCH(k_known_cols<RG_PMAX>, 64, h->stream); KNOWN_LAUNCH(k_known_cols<IN_PMAX>, 64, h->stream); }
int launch_known_resid(pyvb_lds* h, int side) { KNOWN_LAUNCH(k_known_resid, 64, h->stream); }
int launch_known_elbo(pyvb_lds* h, int side, hipStream_t stream) { KNOWN_LAUNCH(k_known_elbo, 64, stream); }
