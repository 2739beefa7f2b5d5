// Internal definitions shared by the translation units of libpyvb_hip.so (gfx950 only).
#pragma once
#include <cstdint>
#include "host.h"
#include "geometry.h"
#include "replicates.h"
#include "column_parents.h"

struct pyvb_comm;
typedef double d4 __attribute__((ext_vector_type(4)));
typedef double d2 __attribute__((ext_vector_type(2)));

struct Priors {          // device pointers, shared by all replicates
    double *x0_mean, *x0_prec, *A_pm, *A_pp, *C_pm, *C_pp, *Q_a0, *Q_b0, *R_a0, *R_b0;
    double *A_obs, *C_obs;   // observed entries of the matrices, [row][col], NaN = not observed
    double *Q_w0, *R_w0;     // Wishart priors w0: [D][D], [K][K] (v0 in Q_a0[0], R_a0[0]); nodes_todo.py:207-211
    double *A_pld, *C_pld;   // [D] ln det of each column's diagonal prior precision
    double x0_lndet;     // ln det of x0_prec (Constant.lndet, node.py:301-302)
    double Q_a0_host, R_a0_host, Q_w0_lndet, R_w0_lndet;    // Wishart: v0 and ln det w0 of the two priors
};

// The known channels of one equation of the model with their gain: the inputs u_t and B of the state equation, or the regressors
// v_t and E of the output equation.  `rows` below is the equation's own dimension, D or K.  Which of <A> / <C>, Q / R, resQ / resR,
// H_A / H_C and part 2 / 3 of the bound a record is attached to follows from its index on the handle (k_known.hip: known_args).
//                                   state equation (side 0)        output equation (side 1)
//   width                           P                              Pv
//   channels, gain                  u_t, B                         v_t, E
//   matrix beside the gain, noise   A, Q                           C, R
//   gram                            Suu = sum_{t>=1} u_t u_t^T     Svv = sum_t v_t v_t^T
//   cross_lhs                       Sxu = sum_{t>=1} mu_t u_t^T    Syv = sum_t y_t v_t^T
//   cross_x                         Su1x = sum u_{t+1} mu_t^T      Svx = sum_t v_t mu_t^T
//   saved                           Sx1x                           Syx
struct KnownChannels {
    int width;                      // 0: the handle has no such channels
    double *in;                     // [N][T][width] the channels as the caller gave them; row t drives x_t / enters y_t
    double *mean, *var;             // [N][rows][width] (row, col), [N][width][rows] (column i, entry k), as A_mean / A_var
    double *qld, *lnd;              // [N][width]
    double *pm, *pp, *pld;          // the Constant parents of the gain's columns: [rows][width], [width][rows], ln det of each column's precision [width]
    double *gram;                   // [N][width][width], formed when the channels are set
    double *cross_lhs;              // [N][rows][width]: side 0 out of the statistics pass (k_known_moments), side 1 when V or Y is set
    double *cross_x;                // [N][width][D] out of the statistics pass
    double *saved;                  // [N][rows][D] the moment block's Sx1x / Syx as k_moments left it: the block's copy becomes H_A / H_C
    bool set, priors_set;           // the channels / the parents of the gain have been given
};

struct EventPair;
struct KernelTimer {
    double total_ms; int launches;
};

struct pyvb_lds {
    int device, N, T, D, K, noise;
    bool big;                       // 64 < max(D, K) <= 128: the workgroup-per-replicate kernels of k_big.hip
    double* U2;                     // 128-wide class with the time axis split (W > 1): the c_t of a forward sweep (k_big.hip: BigSweepArgs.Uc)
    Layout L;
    hipStream_t stream;
    struct EventPair* pool; int pool_used;
    // state
    double *Y, *Syy;                // [N][T][K], [N][K] (sum_t y^2)
    double *X[2];                   // ping-pong [N][T][DP], rows in accumulator order (xpos); st.cur is the one that holds the states
    double *A_mean, *A_var, *C_mean, *C_var;
    double *Q_a, *Q_b, *R_a, *R_b;
    double *qld_A, *qld_C;          // [N][D]
    double *lnd_A, *lnd_C;          // [N][D] ln det qcov of the columns, written where qld_A / qld_C are (NaN before the first update)
    int bound;                      // PYVB_BOUND_REFERENCE / PYVB_BOUND_EXACT: which lower bound k_elbo / k_elbo_dense form
    Priors pri;
    double *pri_block;
    double *w0;                     // [DP] L0 m0 of the prior of X_0 (k_prep.hip: k_w0), as of the last pyvb_lds_set_priors
    ColumnParents parents[2];       // the precision parents of the columns of A ([0]) and C ([1]) (column_parents.h); Constant, no block, unless the caller asked
    // derived
    double *Sigma, *qld_x;          // as of the last X update: [N][3][D][D], [N][3]
    double *Sigma_new, *qld_x_new;  // written by k_prep for the current parameters
    double *lnd_x, *lnd_x_new;      // [N][3] ln det Sigma beside qld_x / qld_x_new (swapped with them)
    double *gains;                  // [N][L.gains_total]
    double *scratch;                // [N][2][DP][DP] (M_C, M_A + M_C)
    int *warm;                      // [N][2]
    double *zeros;                  // [64] zeros: the row that k_stats reads where there is no row
    double *trash;                  // [N][256] dump rows for masked-out stores of the sweep
    double *U;                      // [N][T][DP] c_t = F mu_{t-1} + G y_t written by the forward sweep for the backward one that follows it
    double *stats; int nchunk, chunk_len;   // [N][nchunk][L.stats_total]
    int W;                          // wavefronts per replicate in the sweeps (time split; 1 unless N is small)
    double *sxx;                    // [N][W][DP][DP] interior sum of mu mu^T from the backward sweep
    double *mom;                    // [N][3 D^2 + K D + D] second moments (k_moments)
    double *resQ, *resR;            // [N][D], [N][K]
    double *elbo, *elbo_sum;        // [N][6], [8]: the six parts, then the number of replicates still running (k_elbo_sum)
    int *status;                    // device, [N]: PYVB_FAIL_* bits of the replicates whose factorisations met a non-positive pivot
    // ---- per-replicate bookkeeping.  What replicate n is -- chain length, model, switched off, converged -- lives on the host in
    // `rep` (replicates.h); the device arrays below are what the kernels read of it.
    Replicates rep;
    unsigned char *active;          // device, [N]: 0 = switched off or converged; every update kernel leaves such a replicate's rows alone
    // ---- per-replicate convergence (pyvb_lds_iterate_until, k_converge.hip).  `active` above is the mask the update kernels run:
    // the caller's mask without the converged replicates (rep.run_mask()).  `counted` is the mask the totals count: the caller's
    // mask alone (rep.caller_mask()).  The two are equal until a replicate converges.
    unsigned char *counted;         // device, [N]
    unsigned char *conv;            // device, [N]: 1 = converged, frozen for the life of the handle (rep adopts it when iterate_until returns)
    int *conv_iters;                // device, [N]: iterations carried out under pyvb_lds_iterate_until
    double *conv_llb;               // device, [N]: the last bound the test saw (the next test's `old`); NaN before the first
    double *running_host;           // pinned, [1]: the number of running replicates (all ranks) as of the last check
    hipEvent_t ev_check;            // that copy has arrived
    // ---- per-replicate chain lengths (pyvb_lds_create_lengths): null on a handle whose chains all have T nodes
    int *len;                       // device, [N]: T_n.  T stays the row stride of every [N][T][..] buffer; rows t >= T_n are padding
    // ---- several chains, one model (pyvb_lds_create_tied, k_tie.hip): null on a handle whose models are single replicates
    int *mstart;                    // device, [rep.M() + 1]: model m is replicates mstart[m] .. mstart[m + 1] - 1
    unsigned char *first;           // device, [N]: 1 = the first replicate of its model, where k_elbo books the shared nodes' terms
    std::vector<int> status_host, reported;     // [N] staging of a read of status; [N] what the most recent failed sync reported and cleared
    LdsState st;                    // what is current on the device (host.h); written by the events of api.hip only
    DeviceBuffers mem;              // every device allocation of this handle
    bool timing; KernelTimer timers[PYVB_K_COUNT]; int timing_errors;
    pyvb_comm* comm; int rank, world;
    // ---- Wishart noise precisions (nodes_todo.py:205-234): dense expectations, dense column covariances
    bool dense;                     // noise == PYVB_NOISE_WISHART
    double *Q_w, *R_w;              // [N][D][D], [N][K][K] posterior qw as the reference stores it (qv is in Q_a / R_a)
    double *Qbar, *Rbar;            // [N][D][D], [N][K][K] E[Lambda] = qv inv(sym qw)
    double *lnd;                    // [N][4]: ln det E[Q], ln det E[R], ln det sym(Q_w), ln det sym(R_w)
    double *QA, *RC;                // [N][D][D] E[Q]<A>, [N][K][D] E[R]<C>
    double *trA, *trC;              // [N][D] tr(S_i E[Q]), tr(S'_i E[R])
    double *A_cov, *C_cov;          // [N][D][cov_stride(D)], [N][D][cov_stride(K)] column covariances, upper 8 x 8 tiles (k_wishart.hip)
    double *SyyF;                   // [N][K][K] sum_t y y^T
    double *RQ, *RR;                // [N][D][D], [N][K][K]: sum over children of 1/2<xx^T> + 1/2<mu mu^T> - <x><mu>^T
    double *ldm;                    // [N][2][D] ln det of the covariance of the unknown entries of partially known columns of A / C
    double *SG;                     // [N][2][64][64] sum_i G[i,i] S_i over the columns of A / C (k_cols_wishart)
    // ---- outputs with missing entries (k_missing.hip); allocated when set_observations sees NaN
    bool has_missing;
    double *Yobs, *Yvar, *Yqld, *Yent;      // [N][T][K] observations (NaN = missing), [N][T][K] variances, [N][T], [N]
    double *Ylnd, *YentX;                   // [N][T] ln det qcov beside Yqld; [N] the exact entropy of those rows (added, not subtracted)
    double *Yld, *YcovS;                    // Wishart noise: [N][T] ln det of each row's covariance of missing entries, [N][K][K] sum_t qcov_t
    // ---- known channels: an input u_t that drives the states, x_t = A x_{t-1} + B u_t (pyvb_lds_create_inputs), and regressors in
    // the output equation, y_t = C x_t + E v_t (pyvb_lds_create_regressors); the kernels are k_known.hip.  known[0] is the state
    // equation (B, u; width P), known[1] the output equation (E, v; width Pv): width 0 and every pointer null on a handle without.
    // The channels ride through the sweeps and the statistics pass as 2 P + Pv extra output channels: those kernels are handed Yt,
    // K + 2 P + Pv and Ct in place of Y, K and C_mean (lds_sweep_* below), and L is the layout of (D, K + 2 P + Pv); everything else
    // keeps reading Y, K and C_mean.  Yt and Ct exist when P or Pv is set.
    KnownChannels known[2];
    double *Yt;                     // [N][T][K + 2 P + Pv] rows [y_t ; u_t ; u_{t+1} ; v_t], u_t zero in row 0, u_{t+1} zero in a chain's last row
    double *Ct;                     // [N][K + 2 P + Pv][D] <C>, then the rows through which the boundary nodes add <Q><B> u, -<A>^T<Q><B> u and -<C>^T<R><E> v
    // ---- the lower bound does not feed the next iteration: inside pyvb_lds_iterate it runs on a side stream
    hipStream_t side;
    hipEvent_t ev_params, ev_elbo;  // parameters of this iteration complete (main) / lower bound of it read them (side)
    bool elbo_in_flight;            // ev_elbo has been recorded and not yet waited for by the main stream
    double* elbo_hist; int hist_count;      // [PYVB_ELBO_HISTORY][8]: parts summed over replicates (and ranks), one row per iteration
};
#define PYVB_ELBO_HISTORY 4096

// what the sweeps, the single-node update and the statistics pass are handed as outputs, their number and <C>
static inline int lds_sweep_K(const pyvb_lds* h) { return h->K + 2 * h->known[0].width + h->known[1].width; }
static inline const double* lds_sweep_Y(const pyvb_lds* h) { return h->known[0].width || h->known[1].width ? h->Yt : h->Y; }
static inline const double* lds_sweep_C(const pyvb_lds* h) { return h->known[0].width || h->known[1].width ? h->Ct : h->C_mean; }

// the rows of the gain of known[side]: the dimension of the equation it stands in
static inline int lds_known_rows(const pyvb_lds* h, int side) { return side ? h->K : h->D; }

// ---- launchers implemented in the kernel translation units ----
// k_known.hip (handles with known channels only); side: 0 = the inputs of the state equation, 1 = the regressors of the output equation
int launch_known_assemble(pyvb_lds* h);             // Yt from Y, the inputs and the regressors, every row of every replicate
int launch_known_gram(pyvb_lds* h, int side);       // Suu from the inputs / Svv and Syv from the regressors and Y
int launch_known_gains(pyvb_lds* h, int side);      // behind k_prep: the side's column groups of G, its rows of Ct, the ones behind <R>
int launch_known_moments(pyvb_lds* h, int side);    // behind k_moments: the cross sums out of the Syx block, Sx1x / Syx aside
int launch_known_H(pyvb_lds* h, int side);          // H_A = Sx1x - <B> Su1x / H_C = Syx - <E> Svx into the moment block, for the columns of A / C and the residual of Q / R
int launch_known_cols(pyvb_lds* h, int side);       // [b.update() for b in Bs] / [e.update() for e in Es]
int launch_known_resid(pyvb_lds* h, int side);      // the terms of <B> / <E> in the residual of Q / R
int launch_known_elbo(pyvb_lds* h, int side, hipStream_t stream);   // the columns of B / E into part 2 / 3, behind k_elbo on the same stream
int launch_prep(pyvb_lds* h);
int launch_w0(pyvb_lds* h);         // L0 m0 from the priors of X_0 on the device: after every change of them
// A sweep reads X[src] and writes X[1 - src]; read_cache: a backward sweep that starts from the c_t a forward one left in U.
// keep_x = false: a forward sweep whose states nobody reads (the backward one follows and reads c_t).
int launch_sweep(pyvb_lds* h, int direction, int src, bool read_cache, bool keep_x);
int launch_step(pyvb_lds* h, int t);
int launch_syy(pyvb_lds* h);
int launch_permute(pyvb_lds* h, const double* src, double* dst, int to_internal);
int launch_carry(pyvb_lds* h, const double* src, double* dst, size_t per);     // rows of switched-off replicates, per doubles each
int launch_stats(pyvb_lds* h, bool with_sxx);   // with_sxx = false: Sxx comes from the backward sweep (h->sxx)
int launch_moments(pyvb_lds* h, bool sxx_from_sweep);
int launch_observe(pyvb_lds* h);
int launch_tie(pyvb_lds* h, double* buf, size_t per);      // k_tie.hip: sum rows of [N][per] over the chains of every model, in place
int launch_cols(pyvb_lds* h, int which, int c0, int c1, int fuse = 0);   // which: 0 = A, 1 = C, 2 = both; columns [c0, c1); fuse: see k_cols.hip
int launch_resid(pyvb_lds* h, int which);     // 0 = Q, 1 = R
// k_ard.hip: [al.update() for al in alphas] of A (0), C (1) or both (2); derive: form qa / qb and the log-determinants from qb as given
int launch_ard(pyvb_lds* h, int which, bool derive);
// k_ard.hip: [dg.update() for dg in the DiagonalGamma parents] of the columns of A (0), C (1) or both (2); derive as above
int launch_entry(pyvb_lds* h, int which, bool derive);
int launch_noise(pyvb_lds* h, int which);
int launch_elbo(pyvb_lds* h, hipStream_t stream = nullptr);                           // stream: the handle's main one unless given
int launch_elbo_sum(pyvb_lds* h, double* out = nullptr, hipStream_t stream = nullptr);    // out: h->elbo_sum unless given; [7], out[6] = replicates still running
// k_converge.hip: the stopping test of network.py:53 on the bound of every model (on a handle without tied models: of every
// replicate) with the freeze of the chains it stops (first: old = -inf)
int launch_converge(pyvb_lds* h, double tol, bool first, hipStream_t stream);
// k_big.hip
int launch_prep_big(pyvb_lds* h);
int big_prepare_kernels();              // once per device, before the first launch: the dynamic-LDS limits of k_prep_big, k_cols_big
int launch_sweep_big(pyvb_lds* h, int direction, int src, bool cached);
int launch_step_big(pyvb_lds* h, int t);
int launch_stats_big(pyvb_lds* h);
int launch_cols_big(pyvb_lds* h, int which, int c0, int c1, int fuse);
// k_wishart.hip
int launch_wexpect(pyvb_lds* h);                    // Qbar, Rbar, lnd from Q_w, R_w
int launch_dense_pre(pyvb_lds* h);                  // QA, RC, trA, trC
int launch_cols_dense(pyvb_lds* h, int which, int c0, int c1);
int launch_wresid(pyvb_lds* h, int which, int update, bool use_sg);      // use_sg: SG holds the sums over the columns (LdsState.sg_valid)
int launch_syy_full(pyvb_lds* h);
int launch_elbo_dense(pyvb_lds* h, hipStream_t stream = nullptr);
int launch_colvar_to_cov(pyvb_lds* h);              // A_var/C_var (diagonals) -> A_cov/C_cov
int launch_cov_to_colvar(pyvb_lds* h);              // and back
int launch_cov_observe(pyvb_lds* h);                // zero covariance of the fully known columns
int launch_cov_convert(pyvb_lds* h, int which, double* dense, int n0, int count, int to_packed);   // dense [count][D][rows][rows] (device) <-> the tiles of replicates n0..
// k_wishart_big.hip: the same on the second shape class (64 < max(D, K) <= 128)
int launch_wexpect_big(pyvb_lds* h);
int launch_dense_pre_big(pyvb_lds* h);
int launch_cols_dense_big(pyvb_lds* h, int which, int c0, int c1);
int launch_wresid_big(pyvb_lds* h, int which, int update, bool use_sg);
int launch_syy_full_big(pyvb_lds* h);
// k_missing.hip
int launch_missing_init(pyvb_lds* h, const double* Yq0, const double* Yrowvar0);     // device pointers or null
int launch_impute(pyvb_lds* h);
int launch_syy_missing(pyvb_lds* h);
int launch_impute_dense(pyvb_lds* h);                 // Wishart noise: [y.update() for y in Ys if not y.observed]
int launch_missing_ent_dense(pyvb_lds* h, int diag_cov);

// communicators, shared by the LDS and the PCA path (api.hip): RCCL, or the caller's own host-side all-reduce
// (pyvb_*_comm_init_host: the sums travel through host memory -- a rehearsal transport for boxes where RCCL cannot run)
struct pyvb_comm {
    void* nccl;                                    // ncclComm_t, or null
    pyvb_host_allreduce_fn fn; void* user;         // host transport
    double* host; size_t cap;                      // its staging buffer
};
int pyvb_comm_create(pyvb_comm** comm, const char id[128], int rank, int world);
int pyvb_comm_create_host(pyvb_comm** comm, pyvb_host_allreduce_fn fn, void* user);
void pyvb_comm_free(pyvb_comm* comm);
int pyvb_allreduce_f64(pyvb_comm* comm, double* buf, size_t count, hipStream_t stream);

// Timed launch bracket.  When timing is on, an event pair from the handle's pool is recorded
// around the launch on the handle's stream; nothing synchronises until pyvb_lds_timing_get(),
// so timing can stay on inside a measured region.
#define PYVB_EVENT_POOL 2048
struct EventPair { hipEvent_t e0, e1; int kernel; };
struct TimedLaunch {
    pyvb_lds* h; int slot; hipStream_t s;
    TimedLaunch(pyvb_lds* h_, int k_, hipStream_t s_ = nullptr);
    ~TimedLaunch();
};
void pyvb_timing_resolve(pyvb_lds* h);
