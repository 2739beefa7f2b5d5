/*
 * pyvb_hip.h -- C ABI of libpyvb_hip.so: the MI355X (gfx950) implementation of pyvb's
 * variational update loop for the linear-dynamical-system graph, batched over N
 * independent replicates.
 *
 * The reference (jameshensman/pyvb) is pure Python and has no FFI layer; the boundary it
 * exposes is the node/network Python API (the files under src/pyvb/nodes and src/pyvb/network.py).
 * Each entry point below therefore names the reference METHODS whose work it performs for
 * every node of one class at once.  pyvb_amd/ binds these symbols with ctypes
 * (pyvb_amd/_capi.py) and re-exposes the node API on top of them; INTEGRATION.md shows
 * the stub a maintainer of the reference would add.
 *
 * Conventions
 *   - plain C, opaque handle, one handle per GPU; global state: the thread-local error string and the RCCL entry
 *     points (dlopen'ed once, under a lock, when a communicator is first asked for); thread-compatible (one host
 *     thread per handle).
 *   - every function returns 0 on success or a pyvb_status; pyvb_last_error() gives
 *     the message of the last failure on the calling thread.
 *   - all arrays are caller-owned HOST buffers of float64, C-contiguous, leading axis N
 *     (replicate); a NULL array pointer means "skip this one".  Device memory is owned
 *     by the handle.
 *   - all work is queued on the handle's HIP stream; getters synchronise.
 *
 * Array shapes (D latent dim, K observed dim, T time steps, N replicates)
 *   Y[N][T][K]  X[N][T][D]
 *   A_mean[N][D][D]  (row, col)        A_colvar[N][D][D]  (column i, entry k): diagonal of
 *   C_mean[N][K][D]  (row, col)        C_colvar[N][D][K]   the covariance of column i
 *   Q_a,Q_b[N][D]   R_a,R_b[N][K]      (PYVB_NOISE_GAMMA: all entries of a row are equal)
 *   Sigma[N][3][D][D], qld_x[N][3]     posterior covariance / q_ln_det of X_0, X_interior, X_{T-1}
 *   elbo parts [N][6] = L_X, L_Y, L_A, L_C, L_Q, L_R
 *   handles with P inputs (pyvb_lds_create_inputs): U[N][T][P], B_mean[N][D][P] (row, col), B_colvar[N][P][D] (column i, entry k)
 *   handles with Pv regressors (pyvb_lds_create_regressors): V[N][T][Pv], E_mean[N][K][Pv] (row, col), E_colvar[N][Pv][K] (column i, entry k)
 */
#ifndef PYVB_HIP_H
#define PYVB_HIP_H

#ifdef __cplusplus
extern "C" {
#endif

typedef struct pyvb_lds pyvb_lds;

typedef enum {
    PYVB_OK = 0,
    PYVB_E_ARG = 1,          /* bad argument (shape limits: 2 <= T, 1 <= D,K <= 128) */
    PYVB_E_HIP = 2,          /* HIP runtime error */
    PYVB_E_LINALG = 3,       /* a posterior precision was not positive definite (numpy LinAlgError in the reference) */
    PYVB_E_STALE = 4,        /* statistics requested while the X_t were updated under different parameters */
    PYVB_E_RCCL = 5,         /* RCCL error */
    PYVB_E_UNSUPPORTED = 6
} pyvb_status;

enum { PYVB_NOISE_DIAGONAL_GAMMA = 0,   /* nodes_todo.py:159-204 DiagonalGamma */
       PYVB_NOISE_GAMMA = 1,            /* nodes_todo.py:88-157  Gamma (isotropic) */
       PYVB_NOISE_WISHART = 2 };        /* nodes_todo.py:205-234 Wishart (dense precisions; see pyvb_lds_set_wishart_priors) */
enum { PYVB_FORWARD = 0, PYVB_BACKWARD = 1 };

/* Why a replicate failed (pyvb_lds_get_status): which family of nodes had a posterior precision that was not positive definite
 * (gaussian.py:117-119 raises numpy's LinAlgError from that node's update) */
#define PYVB_FAIL_STATES 1      /* an X_t (k_prep: the three posterior precisions of the states) */
#define PYVB_FAIL_COLUMNS 2     /* a column of A or C with dense covariance (Wishart noise) */
#define PYVB_FAIL_NOISE 4       /* the qw of a Wishart precision (nodes_todo.py:233-234 inverts it) */

/* Which lower bound the ELBO entry points form (pyvb_lds_set_bound_mode, pyvb_pca_set_bound_mode):
 *   REFERENCE  the reference's log_lower_bound, quirks Q1 / Q2 of SURVEY.md included (the default)
 *   EXACT      E_q[ln p] - E_q[ln q]: the entropies of latent Gaussians from ln det qcov, those of partially observed ones with
 *              the sign of a true entropy, E[ln det Lambda] in place of ln det E[Lambda] in the Gaussians' own terms */
#define PYVB_BOUND_REFERENCE 0
#define PYVB_BOUND_EXACT 1

/* the kind of precision parent the columns of a matrix have (pyvb_lds_get_column_parents, pyvb_pca_get_column_parents) */
#define PYVB_PARENTS_CONSTANT 0
#define PYVB_PARENTS_GAMMA 1
#define PYVB_PARENTS_DIAGONAL_GAMMA 2

/* which kernels pyvb_lds_timing_get() reports on */
enum { PYVB_K_PREP = 0, PYVB_K_SWEEP_FWD = 1, PYVB_K_STATS = 2, PYVB_K_PARAMS = 3, PYVB_K_STEP = 4,
       PYVB_K_SWEEP_BWD = 5, PYVB_K_ELBO = 6, PYVB_K_GY = 7 /* 128-wide class: G y_t ahead of a sweep */,
       PYVB_K_INPUTS = 8 /* handles with inputs: the kernels of k_known.hip */,
       PYVB_K_REGRESSORS = 9 /* handles with regressors: the kernels of k_known.hip */, PYVB_K_COUNT = 10 };

const char* pyvb_last_error(void);
int pyvb_version(void);
/* first 32 hex digits of the sha256 over the library's source files (pyvb_amd/csrc/Makefile: BUILD_ID): lets a caller check
 * that a prebuilt libpyvb_hip.so is the build of the sources beside it */
const char* pyvb_build_id(void);
int pyvb_device_count(int* count);

/* Graph construction: Linear_Dynamic_System.py:46-66 for N replicates
 * (2T Gaussian, 2 hstack of D Gaussian columns, 2 noise nodes per replicate). */
int pyvb_lds_create(pyvb_lds** out, int device, int N, int T, int D, int K, int noise_kind);
int pyvb_lds_destroy(pyvb_lds* h);

/* The same with a chain length of its own per replicate: replicate n is the graph of Linear_Dynamic_System.py:46-66 whose
 * loop (:58-66) runs over T_n = lengths[n] time steps, 2 <= T_n <= T.  lengths[N]; NULL = pyvb_lds_create.  The lengths are
 * part of graph construction and cannot change afterwards; pyvb_lds_get_lengths reads them back (all T on a plain handle).
 *   - Storage stays [N][T][..]: rows t >= T_n of replicate n are padding, not nodes.  Setters accept anything there (NaN
 *     included) and nothing derived from such a row reaches a result; getters return 0.0 in padding rows of X and of the
 *     outputs, NaN in padding entries of Yqld / Ylnd.
 *   - Q of replicate n has T_n - 1 children and R has T_n, so qa follows nodes_todo.py:125-128, 183-186 per replicate; the
 *     three posterior classes are X_0, the interior and X_{T_n - 1} (T_n = 2: no interior).
 *   - pyvb_lds_update_x(h, t) is Xs_n[t].update() for every active n with t < T_n; node T_n - 1 is the last node of its own
 *     replicate.  pyvb_lds_set_time_split's limit and the staleness check of the statistics count the handle's T.
 *   - the ELBO totals, the history and the all-reduce sum the replicates as before.
 * PYVB_E_ARG when some T_n < 2 or T_n > T (the message names the first such replicate).  Served: max(D, K) <= 64 with
 * PYVB_NOISE_DIAGONAL_GAMMA or PYVB_NOISE_GAMMA, with everything else such a handle does (known entries of A / C, both bound
 * modes, every time split, the activity mask and status, communicators).  Follow-ups, refused with PYVB_E_UNSUPPORTED when the
 * lengths are not all equal to T: Wishart noise and max(D, K) > 64 (here, before any HIP call), and NaN in a row t < T_n of Y
 * (pyvb_lds_set_observations) -- k_wishart*.hip, k_big.hip and k_missing.hip read T as the chain length throughout. */
int pyvb_lds_create_lengths(pyvb_lds** out, int device, int N, int T, int D, int K, int noise_kind, const int* lengths);
int pyvb_lds_get_lengths(pyvb_lds* h, int* lengths);

/* Several time series, one model.  A CHAIN is one replicate row (one series of T_n nodes); a MODEL is a run of consecutive
 * replicates that share the nodes As, Cs, Q, R: the graph of Linear_Dynamic_System.py with `As, A, Cs, C, Q, R` built once and
 * the loop of :58-66 run once per series, each with its own X_0.  model[N] gives the model of every replicate: it starts at 0,
 * never decreases and rises in steps of 0 or 1.  model == NULL is pyvb_lds_create_lengths (every replicate a model of its own);
 * lengths == NULL gives every chain T nodes.  pyvb_lds_get_models reads the ids back (0 .. N-1 on every other handle).
 *   - hstack, Gamma and DiagonalGamma sum over their children whoever they belong to (nodes_todo.py:43-62, :125-128,
 *     :183-186): before the columns and the noise are updated, the sufficient statistics of the chains of a model are summed
 *     (k_tie.hip).  qa counts the children of the whole model: Q has sum (T_n - 1), R has sum T_n (pyvb_lds_set_priors).
 *     Every update entry -- sweep, update_x, update_columns, update_A/C/Q/R, update_Y, iterate -- does for every model what
 *     the reference's node updates do on that graph.
 *   - Arrays stay [N][..].  X, Y, the posterior classes and the outputs are per chain.  The parameters are stored in every row
 *     of a model and are bitwise equal there, as are qld_A/C and lnd_A/C.  pyvb_lds_set_state takes A_mean, A_colvar, C_mean,
 *     C_colvar, Q_b, R_b from the row of a model's FIRST replicate and copies them to its other rows; what the caller put
 *     there is ignored.
 *   - Lower bound, both modes: the rows of pyvb_lds_get_elbo of a model add up to the six parts of its graph.  L_A, L_C, L_Q,
 *     L_R are booked on the model's first row and are 0.0 on its other rows.  L_X and L_Y of a row hold the terms of its own
 *     X_t and Y_t, except -tr(<Q> residual) and -tr(<R> residual), which are sums over the model and are booked once, on the
 *     first row; how L_X and L_Y split between the rows of a model is not contractual.  Totals, history, all-reduce: as before.
 *   - pyvb_lds_set_active: a mask that switches off part of a model is PYVB_E_ARG (the message names the model).
 *   - pyvb_lds_iterate_until, whose test is per replicate, still refuses a handle with a model of more than one chain with
 *     PYVB_E_UNSUPPORTED before any launch: convergence per model is pyvb_lds_iterate_until_model (below).
 *   - Composes with chain lengths, known entries of A / C, outputs with NaN (where all chains have T nodes), both bound modes,
 *     every time split, status, communicators (a model never spans ranks: a rank's handle holds whole models).
 * PYVB_E_ARG when model[] is not of that form (the message names the first offending replicate).  PYVB_E_UNSUPPORTED when some
 * model has more than one chain and the noise is Wishart or max(D, K) > 64.  Both before any HIP call.  A handle whose models
 * are all single replicates is bitwise a pyvb_lds_create_lengths handle. */
int pyvb_lds_create_tied(pyvb_lds** out, int device, int N, int T, int D, int K, int noise_kind,
                         const int* lengths, const int* model);
int pyvb_lds_get_models(pyvb_lds* h, int* model);

/* A known input that drives the states: replicate n is the graph of Linear_Dynamic_System.py:46-66 with
 *     X_t = Gaussian(q, A * X_{t-1} + B * Constant(u_t), Q),   B = hstack(Bs),   t = 1 .. T_n - 1
 * -- an Addition of two Multiplications as the mean parent (node.py:52-129, :182-276), u_t a known P-vector (a controlled plant, a
 * stimulus, a seasonal regressor), B [D x P] with independent Gaussian columns and Constant parents like A's
 * (hstack.pass_up_m1_m2, nodes_todo.py:43-62).  lengths[N] as pyvb_lds_create_lengths takes it, or NULL: every chain has T nodes.
 *   pyvb_lds_set_inputs        U[N][T][P]: row t drives x_t.  Row 0 and the rows t >= T_n are never read and may hold anything
 *                              finite.  Call before the first update; a later call replaces the inputs.
 *   pyvb_lds_get_inputs        U as given.
 *   pyvb_lds_set_input_priors  B_prior_mean[D][P] (row, col), B_prior_prec[P][D] (column i, diagonal entry k), positive; shared by
 *                              the replicates as A's are.
 *   pyvb_lds_set_input_state   B_mean[N][D][P] (row, col), B_colvar[N][P][D] (column i, entry k); NULL = leave.
 *   pyvb_lds_get_input_state   the same, and q_ln_det / ln det qcov of the columns, qld_B[N][P], lnd_B[N][P] (NaN before a column's
 *                              first update); NULL = skip.
 *   pyvb_lds_update_B          [b.update() for b in Bs]: G = sum_{t>=1} u_t u_t^T, H = sum_{t>=1} mu_t u_t^T - <A> sum_t mu_t u_{t+1}^T,
 *                              row precisions <Q>.
 * Everything else serves the handle as it stands, with the input's terms: pyvb_lds_sweep and pyvb_lds_update_x (mean parent
 * <A> mu_{t-1} + <B> u_t; the message of X_{t+1} is <A>^T <Q> (mu_{t+1} - <B> u_{t+1})), pyvb_lds_update_A / _columns(0, ..)
 * (H = Sx1x - <B> sum_t u_{t+1} mu_t^T), pyvb_lds_update_Q (the second moment of the mean parent, Addition.pass_down_ExxT
 * node.py:121-129), pyvb_lds_elbo in both modes (L_X with that moment; the columns of B add to part 2 what the columns of A do, so
 * parts stay [N][6]), pyvb_lds_iterate, pyvb_lds_iterate_until and pyvb_lds_iterate_until_model (forward, backward, As, Bs, Cs, Q, R,
 * bound), chain lengths, every time split, the activity mask (a switched-off replicate keeps its B), status, communicators.
 * The inputs ride through the sweeps as 2 P extra output channels (k_known.hip), hence the limit of this route:
 * max(D, K + 2 P) <= 64.
 * PYVB_E_UNSUPPORTED before any HIP call / launch, the message naming the cause: Wishart noise; max(D, K + 2 P) > 64; outputs that hold
 * NaN (pyvb_lds_set_observations); known entries of A / C (pyvb_lds_set_column_observations); Gamma / DiagonalGamma precision parents
 * (pyvb_lds_set_column_precisions, pyvb_lds_set_entry_precisions); shared models are not offered (pyvb_lds_create_tied takes no
 * inputs, and pyvb_lds_create_inputs no models).
 * PYVB_E_ARG: P < 1; NULL or non-finite U (the message names replicate, row and channel); a non-positive B_prior_prec; any of the six
 * entries on a handle created without inputs; an update before pyvb_lds_set_inputs and pyvb_lds_set_input_priors. */
int pyvb_lds_create_inputs(pyvb_lds** out, int device, int N, int T, int D, int K, int P, int noise_kind, const int* lengths);
int pyvb_lds_set_inputs(pyvb_lds* h, const double* U);
int pyvb_lds_get_inputs(pyvb_lds* h, double* U);
int pyvb_lds_set_input_priors(pyvb_lds* h, const double* B_prior_mean, const double* B_prior_prec);
int pyvb_lds_set_input_state(pyvb_lds* h, const double* B_mean, const double* B_colvar);
int pyvb_lds_get_input_state(pyvb_lds* h, double* B_mean, double* B_colvar, double* qld_B, double* lnd_B);
int pyvb_lds_update_B(pyvb_lds* h);

/* Known regressors in the output equation: replicate n is the graph of Linear_Dynamic_System.py:46-66 with
 *     Y_t = Gaussian(K, C * X_t + E * Constant(v_t), R),   E = hstack(Es),   t = 0 .. T_n - 1
 * -- an Addition of two Multiplications as the mean parent of the observed Y_t (node.py:52-129, :182-276), v_t a known Pv-vector
 * (v_t = 1: an output offset; v_t = u_t: direct feedthrough of an input; a seasonal or covariate regressor), E [K x Pv] with
 * independent Gaussian columns and Constant parents like C's (hstack.pass_up_m1_m2, nodes_todo.py:43-62).  P >= 0 are the inputs
 * that drive the states, as pyvb_lds_create_inputs takes them (0: none; the six input entries then refuse the handle); Pv >= 1.
 * lengths[N] as pyvb_lds_create_lengths takes it, or NULL: every chain has T nodes.
 *   pyvb_lds_set_regressors        V[N][T][Pv]: row t enters y_t, row 0 included.  The rows t >= T_n are never read and may hold
 *                                  anything finite.  Call before the first update; a later call replaces the regressors.
 *   pyvb_lds_get_regressors        V as given.
 *   pyvb_lds_set_regressor_priors  E_prior_mean[K][Pv] (row, col), E_prior_prec[Pv][K] (column i, diagonal entry k), positive;
 *                                  shared by the replicates as C's are.
 *   pyvb_lds_set_regressor_state   E_mean[N][K][Pv] (row, col), E_colvar[N][Pv][K] (column i, entry k); NULL = leave.
 *   pyvb_lds_get_regressor_state   the same, and q_ln_det / ln det qcov of the columns, qld_E[N][Pv], lnd_E[N][Pv] (NaN before a
 *                                  column's first update); NULL = skip.
 *   pyvb_lds_update_E              [e.update() for e in Es]: G = sum_t v_t v_t^T, H = sum_t y_t v_t^T - <C> sum_t mu_t v_t^T,
 *                                  row precisions <R>.
 * Everything else serves the handle as it stands, with the regressors' terms: pyvb_lds_sweep and pyvb_lds_update_x (the message of
 * Y_t is <C>^T <R> (y_t - <E> v_t)), pyvb_lds_update_C / _columns(1, ..) (H = Syx - <E> sum_t v_t mu_t^T), pyvb_lds_update_R (the
 * second moment of the mean parent, Addition.pass_down_ExxT node.py:121-129), pyvb_lds_elbo in both modes (L_Y with that residual;
 * the columns of E add to part 3 what the columns of C do, so parts stay [N][6]), pyvb_lds_iterate, pyvb_lds_iterate_until and
 * pyvb_lds_iterate_until_model (forward, backward, As, [Bs], Cs, Es, Q, R, bound), chain lengths, every time split, the activity
 * mask (a switched-off replicate keeps its E), status, communicators.
 * The regressors ride through the sweeps as Pv extra output channels behind the 2 P of the inputs (k_known.hip), hence the
 * limit of this route, the only cap on Pv: max(D, K + 2 P + Pv) <= 64.
 * PYVB_E_UNSUPPORTED before any HIP call / launch, the message naming the regressors and the cause: Wishart noise;
 * max(D, K + 2 P + Pv) > 64; outputs that hold NaN (pyvb_lds_set_observations); known entries of A / C
 * (pyvb_lds_set_column_observations); Gamma / DiagonalGamma precision parents (pyvb_lds_set_column_precisions,
 * pyvb_lds_set_entry_precisions); shared models are not offered (pyvb_lds_create_tied takes no regressors).
 * PYVB_E_ARG: Pv < 1; P < 0; NULL or non-finite V (the message names replicate, row and channel); a non-positive E_prior_prec; any
 * of the six entries on a handle created without regressors; an update before pyvb_lds_set_regressors and
 * pyvb_lds_set_regressor_priors. */
int pyvb_lds_create_regressors(pyvb_lds** out, int device, int N, int T, int D, int K, int P, int Pv, int noise_kind, const int* lengths);
int pyvb_lds_set_regressors(pyvb_lds* h, const double* V);
int pyvb_lds_get_regressors(pyvb_lds* h, double* V);
int pyvb_lds_set_regressor_priors(pyvb_lds* h, const double* E_prior_mean, const double* E_prior_prec);
int pyvb_lds_set_regressor_state(pyvb_lds* h, const double* E_mean, const double* E_colvar);
int pyvb_lds_get_regressor_state(pyvb_lds* h, double* E_mean, double* E_colvar, double* qld_E, double* lnd_E);
int pyvb_lds_update_E(pyvb_lds* h);

/* Constant parents (node.py:279-311), shared by all replicates:
 *   x0_mean[D], x0_prec[D][D]                     Gaussian(q, pmu, pprec) for X_0  (:58)
 *   A_prior_mean[D][D] (row,col), A_prior_prec[D][D] (column i, diagonal entry k)   (:47)
 *   C_prior_mean[K][D], C_prior_prec[D][K]                                          (:49)
 *   Q_a0,Q_b0[D], R_a0,R_b0[K]                    DiagonalGamma / Gamma priors      (:51-54)
 * Dense prior precisions for the columns are not supported (PYVB_E_UNSUPPORTED is the caller's check). */
int pyvb_lds_set_priors(pyvb_lds* h, const double* x0_mean, const double* x0_prec,
                        const double* A_prior_mean, const double* A_prior_prec,
                        const double* C_prior_mean, const double* C_prior_prec,
                        const double* Q_a0, const double* Q_b0, const double* R_a0, const double* R_b0);

/* Wishart noise precisions (Linear_Dynamic_System.py:55-56; nodes_todo.py:205-234), for handles created with
 * PYVB_NOISE_WISHART: Q = Wishart(D, Q_v0, Q_w0[D][D]), R = Wishart(K, R_v0, R_w0[K][K]); call after pyvb_lds_set_priors
 * (whose Gamma arguments may then be NULL).  State: qv (fixed by the graph, update_v :224-227) and qw ([N][D][D] /
 * [N][K][K], update :228-231); E[Lambda] = qv * inv(qw) (:233-234).  The columns of A and C then have dense posterior
 * covariances A_cov[N][D][D][D] (column i: [D][D]) and C_cov[N][D][K][K]; pyvb_lds_set_state's A_colvar / C_colvar give
 * diagonal initial ones.  Above 64 dimensions (k_wishart_big.hip) Wishart noise does not combine with known entries of A / C or
 * with outputs that hold NaN: pyvb_lds_set_column_observations / pyvb_lds_set_observations return PYVB_E_UNSUPPORTED there.
 * Deviations from the unfinished reference class (prior not mutated by update(), symmetric part
 * of qw in the expectation, a defined lower bound) are listed at the top of pyvb_amd/csrc/k_wishart.hip. */
int pyvb_lds_set_wishart_priors(pyvb_lds* h, double Q_v0, const double* Q_w0, double R_v0, const double* R_w0);
int pyvb_lds_set_wishart_state(pyvb_lds* h, const double* Q_w, const double* R_w);
int pyvb_lds_get_wishart_state(pyvb_lds* h, double* Q_v, double* Q_w, double* R_v, double* R_w);
int pyvb_lds_set_column_cov(pyvb_lds* h, const double* A_cov, const double* C_cov);
int pyvb_lds_get_column_cov(pyvb_lds* h, double* A_cov, double* C_cov);

/* Gaussian.observe for every Y_t (gaussian.py:74-100).  NaN = missing: a row with some NaN is partially observed, a row of
 * NaN is not observed at all; such Y_t are variational nodes of their own (DiagonalGamma / Gamma noise only):
 *   pyvb_lds_set_output_state  their initial posterior (mean Yq[N][T][K], isotropic variance Yrowvar[N][T]; rows without NaN
 *                              ignored) -- until its first update a partially observed node keeps the constructor's draw in
 *                              ALL its entries (observe() only records the known values); default N(0, I)
 *   pyvb_lds_update_Y          [y.update() for y in Ys if not y.observed]  (gaussian.py:102-134, parents only)
 *   pyvb_lds_get_outputs       their posterior means and variances ([N][T][K] each; fully observed rows: value, 0) and the
 *                              q_ln_det of the rows updated so far ([N][T], NaN otherwise); NULL = skip
 * The example's loop (pyvb_lds_iterate) never updates the outputs; call pyvb_lds_update_Y where the script does. */
int pyvb_lds_set_observations(pyvb_lds* h, const double* Y);
int pyvb_lds_set_output_state(pyvb_lds* h, const double* Yq, const double* Yrowvar);
int pyvb_lds_update_Y(pyvb_lds* h);
int pyvb_lds_get_outputs(pyvb_lds* h, double* Yq, double* Yvar, double* Yqld);

/* As[i].observe(v) / Cs[i].observe(v) (gaussian.py:74-100; examples/LDS_knowns_in_A.py:73-74): known entries of the
 * transition / observation matrices, A_obs[D][D] and C_obs[K][D] as (row, col), NaN = not observed; NULL = leave.
 * Call after set_state: fully known columns take their value at once, partially known ones at their next update. */
int pyvb_lds_set_column_observations(pyvb_lds* h, const double* A_obs, const double* C_obs);

/* Automatic relevance determination: Gamma precision parents for the columns of A (which = 0, rows = D) or C (which = 1,
 * rows = K).  Column i becomes Gaussian(rows, pm_i, alpha_i) with alpha_i = Gamma(rows, a0_i, b0_i) (gaussian.py:55-61;
 * nodes_todo.py:113-157) in place of its Constant precision: the prior precision of the column is qa_i / qb[n][i] in every row,
 * qa_i = a0_i + rows / 2 is fixed by the graph, and
 *   alpha_i.update():  qb[n][i] = b0_i + 1/2 sum_k ((M[k,i] - pm[k,i])^2 + V[i][k])      (known entries: M = value, V = 0).
 * The lower bound takes rows (ln qa - ln qb) (reference mode, quirk Q2) or rows (psi(qa) - ln qb) (exact mode) as the column's
 * ln det, and adds the alpha nodes' own terms to part 2 (A) and part 3 (C).
 *   a0[D], b0[D]: per column, shared by the replicates like every prior.
 *   qb[N][D]: initial state (the reference draws rand(), nodes_todo.py:119).  On a handle with tied models it is taken from
 *   each model's first row and copied to its other rows, as pyvb_lds_set_state does.
 * Call after pyvb_lds_set_priors; a later pyvb_lds_set_priors returns both matrices to Constant parents.
 * pyvb_lds_iterate, pyvb_lds_iterate_until and pyvb_lds_iterate_until_model on such a handle run forward, backward, A, C, Q, R,
 * alpha_A, alpha_C, bound.  Switched-off and converged replicates keep their qb.
 * PYVB_E_UNSUPPORTED: Wishart noise, or max(D, K) > 64.  PYVB_E_ARG: which outside {0, 1}; a non-finite or non-positive a0, b0
 * or qb (the message names the column, or the replicate and column); get / update for a matrix without hyperpriors. */
int pyvb_lds_set_column_precisions(pyvb_lds* h, int which, const double* a0, const double* b0, const double* qb);
int pyvb_lds_get_column_precisions(pyvb_lds* h, int which, double* qa, double* qb);   /* [N][D] each; NULL = skip */
int pyvb_lds_update_column_precisions(pyvb_lds* h, int which);     /* [al.update() for al in alphas of that matrix] */

/* Sparse A and C: DiagonalGamma precision parents for the columns of A (which = 0, rows = D) or C (which = 1, rows = K), a
 * precision of its own for every entry.  Column i becomes Gaussian(rows, pm_i, DiagonalGamma(rows, a0_i, b0_i)) (gaussian.py:55-61;
 * nodes_todo.py:159-204): the prior precision of the column is diag(qa[i][.] / qb[n][i][.]), qa[i][k] = a0[i][k] + 1/2 is fixed by
 * the graph, and
 *   dg_i.update():  qb[n][i][k] = b0[i][k] + 1/2 ((M[k,i] - pm[k,i])^2 + V[i][k])      (known entries: M = value, V = 0).
 * The lower bound takes sum_k (ln qa - ln qb) (reference mode, quirk Q2) or sum_k (psi(qa) - ln qb) (exact mode) as the column's
 * ln det, and adds the nodes' own terms to part 2 (A) and part 3 (C).
 *   a0[D][rows], b0[D][rows]: [column][row] as A_prior_prec is, shared by the replicates like every prior.
 *   qb[N][D][rows]: initial state.  On a handle with tied models it is taken from each model's first row and copied to its other
 *   rows, as pyvb_lds_set_column_precisions does.
 * A matrix's columns have Constant, Gamma or DiagonalGamma parents: the most recent setter for that matrix wins, A and C may have
 * different kinds, and pyvb_lds_set_priors returns both to Constant parents.  The three iterate entries run forward, backward, A,
 * C, Q, R, the precision parents of A, then of C, bound.  Switched-off and converged replicates keep their qb.
 * PYVB_E_UNSUPPORTED: Wishart noise, or max(D, K) > 64.  PYVB_E_ARG: which outside {0, 1}; a non-finite or non-positive a0, b0
 * or qb (the message names the column and row, for qb the replicate too); get / update for a matrix without DiagonalGamma parents
 * (and pyvb_lds_get_column_precisions / pyvb_lds_update_column_precisions for a matrix that has them). */
int pyvb_lds_set_entry_precisions(pyvb_lds* h, int which, const double* a0, const double* b0, const double* qb);
int pyvb_lds_get_entry_precisions(pyvb_lds* h, int which, double* qa, double* qb);   /* [N][D][rows] each; NULL = skip */
int pyvb_lds_update_entry_precisions(pyvb_lds* h, int which);      /* [dg.update() for dg in the parents of that matrix] */
/* The kind in force, PYVB_PARENTS_*, of the columns of A (kind[0]) and C (kind[1]).  Needs no device.  PYVB_E_ARG: NULL. */
int pyvb_lds_get_column_parents(pyvb_lds* h, int kind[2]);

/* Explicit posterior state instead of the constructors' random initialisation
 * (gaussian.py:70-72, nodes_todo.py:119,177). */
int pyvb_lds_set_state(pyvb_lds* h, const double* X, const double* A_mean, const double* A_colvar,
                       const double* C_mean, const double* C_colvar, const double* Q_b, const double* R_b);
int pyvb_lds_get_state(pyvb_lds* h, double* X, double* A_mean, double* A_colvar, double* C_mean, double* C_colvar,
                       double* Q_a, double* Q_b, double* R_a, double* R_b);
/* qcov / q_ln_det of the X_t as of their last update (gaussian.py:119-120); qld of the columns. */
int pyvb_lds_get_posterior_classes(pyvb_lds* h, double* Sigma, double* qld_x);
/* Initial covariances of the X_t, one per class (the reference draws an individual random one per node, gaussian.py:70-72;
 * they are overwritten by the first sweep).  Without this call, statistics / parameter updates / the lower bound return
 * PYVB_E_STALE until a complete sweep has run.  qld_x may be NULL. */
int pyvb_lds_set_posterior_classes(pyvb_lds* h, const double* Sigma, const double* qld_x);
int pyvb_lds_get_column_qld(pyvb_lds* h, double* qld_A, double* qld_C);

/* [x.update() for x in Xs] in forward or reversed order (Linear_Dynamic_System.py:70-73):
 * Gaussian.update gaussian.py:102-123 with Multiplication.pass_up_m1_m2 node.py:182-232 and
 * pass_down_Ex :235-242 for all T nodes of all replicates in one launch. */
int pyvb_lds_sweep(pyvb_lds* h, int direction);
/* Xs[t].update() alone. */
int pyvb_lds_update_x(pyvb_lds* h, int t);
/* [a.update() for a in As] / Cs: Gaussian.update + hstack.pass_up_m1_m2 nodes_todo.py:43-62 */
int pyvb_lds_update_A(pyvb_lds* h);
int pyvb_lds_update_C(pyvb_lds* h);
/* As[i].update() for i in [col_begin, col_end) in order (which = 0), or the same for Cs (which = 1) */
int pyvb_lds_update_columns(pyvb_lds* h, int which, int col_begin, int col_end);
/* Q.update() / R.update(): nodes_todo.py:130-138, :187-190 with Multiplication.pass_down_ExxT node.py:244-276 */
int pyvb_lds_update_Q(pyvb_lds* h);
int pyvb_lds_update_R(pyvb_lds* h);
/* sum of log_lower_bound() per node class (network.py:49; gaussian.py:136-151; nodes_todo.py:149-157,:199-204),
 * in the mode pyvb_lds_set_bound_mode chose (default: reference mode, quirks Q1, Q2 of SURVEY.md reproduced). Leaves the parts
 * on the device. */
int pyvb_lds_elbo(pyvb_lds* h);
int pyvb_lds_get_elbo(pyvb_lds* h, double* parts);
/* parts summed over this handle's replicates, then over all ranks if a communicator is attached
 * (one ncclAllReduce of 6 doubles). */
int pyvb_lds_elbo_total(pyvb_lds* h, double out[6]);
/* niters passes of: forward sweep, backward sweep, A, C, Q, R, ELBO (the example's loop body plus network.py:49). */
int pyvb_lds_iterate(pyvb_lds* h, int niters);
/* pyvb_lds_iterate evaluates the lower bound of every iteration on a side stream (it feeds nothing in the next one) and
 * keeps the six parts, summed over the replicates and -- with a communicator attached -- over all ranks, in a ring of the
 * last 4096 iterations.  out[count][6], oldest first; synchronises. */
int pyvb_lds_get_elbo_history(pyvb_lds* h, double* out, int max_count, int* count);
int pyvb_lds_reset_elbo_history(pyvb_lds* h);
/* The lower bound that pyvb_lds_elbo and pyvb_lds_iterate form from now on (PYVB_BOUND_*; anything else: PYVB_E_ARG).  The state
 * updates are the same in both modes.  A change of mode empties the ELBO history. */
int pyvb_lds_set_bound_mode(pyvb_lds* h, int mode);
/* ln det qcov of the X_t classes lnd_x[N][3], of the columns of A and C lnd_A[N][D], lnd_C[N][D], and of the outputs with missing
 * entries Ylnd[N][T] (of inv <R>, before the known entries are conditioned on), as their last updates left them; NaN where the
 * q_ln_det getters give NaN.  Kept in both modes; NULL = skip. */
int pyvb_lds_get_logdets(pyvb_lds* h, double* lnd_x, double* lnd_A, double* lnd_C, double* Ylnd);
/* Waits for both streams.  PYVB_E_LINALG, once, if a factorisation of an ACTIVE replicate met a non-positive pivot since the last
 * call (the flags are cleared; the message ends with the index of the first such replicate and their number): cho_factor raising
 * numpy.linalg.LinAlgError in Gaussian.update, gaussian.py:117-119. */
int pyvb_lds_sync(pyvb_lds* h);

/* Per-replicate bookkeeping.  A handle's replicates are independent graphs (Linear_Dynamic_System.py:46-66, once each); in the
 * reference each would raise, converge and be abandoned on its own.
 *   pyvb_lds_get_status  status[N]: PYVB_FAIL_* bits, the node family whose update would have raised LinAlgError
 *                        (gaussian.py:117-119; nodes_todo.py:233-234).  Waits for both streams and never fails because of a flag:
 *                        the OR of the flags pending on the device and of those the most recent failed pyvb_lds_sync reported and
 *                        cleared; the next successful pyvb_lds_sync forgets the latter.
 *   pyvb_lds_set_active  active[N], 0 = switch the replicate off: as if its nodes left every update list of the script
 *                        (Linear_Dynamic_System.py:70-79) and the node list of network.py:46-49.  No update kernel loads or stores a
 *                        row of it from then on; its state, outputs and elbo parts read back as they were; the totals
 *                        (pyvb_lds_elbo_total, the history of pyvb_lds_iterate, the all-reduce) leave it out and pyvb_lds_sync does
 *                        not fail for its flags.  Setters still copy what the caller passes into every row (what they derive from
 *                        it is update work and skips the row); getters return every row.  Stream ordered after everything queued.
 *                        The mask can only shrink: turning a replicate back on returns PYVB_E_ARG (the host-side validity tracking
 *                        is per handle).  With every replicate off the update entries return PYVB_OK without a launch.
 *   pyvb_lds_get_active  the mask as last set (all ones after pyvb_lds_create). */
int pyvb_lds_get_status(pyvb_lds* h, int* status);
int pyvb_lds_set_active(pyvb_lds* h, const unsigned char* active);
int pyvb_lds_get_active(pyvb_lds* h, unsigned char* active);

/* Converging on its own: Network.learn's stopping test (network.py:40-56, the test is on line 53) applied by every replicate to
 * itself, on the device.
 *   pyvb_lds_iterate_until   at most max_iters passes of pyvb_lds_iterate's loop body, same launches in the same order.  For every
 *                        running replicate n: old_n = -inf when the call starts; after iteration i, llb_n = the sum of its six
 *                        parts in the handle's bound mode; llb_n - old_n < tol: converged at i, otherwise old_n = llb_n.  The
 *                        first iteration of a call stops nobody, a decrease stops a replicate too (quirk Q9 of SURVEY.md), a bound
 *                        that is not finite never does (failure flags stay pyvb_lds_sync's business).  A converged replicate is
 *                        frozen from the next launch on exactly as pyvb_lds_set_active would do it -- no update kernel loads or
 *                        stores a row of it; state, classes and parts read back as iteration i left them -- for the life of the
 *                        handle: pyvb_lds_iterate, pyvb_lds_sweep and the other update entries skip it afterwards.  Unlike a
 *                        replicate the caller switched off it stays counted: pyvb_lds_get_active keeps returning the caller's
 *                        mask, and pyvb_lds_elbo_total, the history and the all-reduce sum the running replicates at their
 *                        current bound and the converged ones at their final one.  Returns when no replicate is left running or
 *                        after max_iters, both streams synchronised; *iters_run = iterations launched, one history row each.  The
 *                        host learns the number still running from an 8-byte copy to pinned memory and an event, every
 *                        check_every (>= 1) iterations: check_every affects nothing but iters_run, which may overshoot the last
 *                        stop by at most check_every - 1 idle iterations.  With a communicator the stop is collective: the rank's
 *                        running count rides as a seventh double through this entry's all-reduce and every rank stops in the
 *                        iteration where the sum is 0 (all ranks pass the same max_iters and check_every).  Inside this entry the
 *                        bound does not overlap the next iteration (the decision must precede the next k_prep).
 *                        PYVB_E_ARG before any HIP call: NULL handle, max_iters < 0, check_every < 1, NaN tol, NULL iters_run.
 *   pyvb_lds_get_convergence  iters[N]: iterations replicate n has carried out under pyvb_lds_iterate_until, summed over calls (0 for
 *                        one switched off before its first); converged[N]: 1 once it has converged; llb[N]: the last bound the
 *                        test saw for it (NaN before the first).  Any pointer may be NULL.
 * Served on every handle pyvb_lds_iterate serves.  Not built: thawing a converged replicate (the mask cannot grow), freezing
 * replicates that failed, the node front end (Network.learn over one list keeps the reference's single test on the summed
 * bound), VB-PCA (one model, nothing per replicate). */
int pyvb_lds_iterate_until(pyvb_lds* h, int max_iters, double tol, int check_every, int* iters_run);
int pyvb_lds_get_convergence(pyvb_lds* h, int* iters, unsigned char* converged, double* llb);

/* Every MODEL converging on its own: the same test applied to the bound of a model's graph (pyvb_lds_create_tied).  The chains
 * of a model share A, C, Q, R, so they stop together.
 *   pyvb_lds_iterate_until_model   pyvb_lds_iterate_until's loop, arguments, checks, return and collective stop; what differs is
 *                        the quantity tested.  For every running model m: old_m = -inf when the call starts; after iteration i,
 *                        llb_m = the sum over the model's rows of their six parts (each part summed over the rows in ascending
 *                        order, then the six added left to right); llb_m - old_m < tol and llb_m finite: converged at i, otherwise
 *                        old_m = llb_m.  The first iteration of a call stops nobody, a decrease stops a model (quirk Q9), a bound
 *                        that is not finite never does.  Every chain of a converged model is frozen exactly as
 *                        pyvb_lds_iterate_until freezes a replicate -- for the life of the handle, still counted: the totals, the
 *                        history and the all-reduce hold the model at its final bound.  The per-replicate bookkeeping holds the
 *                        model's values on every one of its chains: pyvb_lds_get_convergence returns them replicated per chain.
 *                        Served on every handle pyvb_lds_iterate_until serves, where every replicate is a model of its own and
 *                        this entry does bitwise what that one does, and on handles with tied models; composes with chain lengths,
 *                        both bound modes, the activity mask (a mask never splits a model), every time split, outputs with NaN
 *                        (equal lengths) and communicators (a model never spans ranks; the seventh double counts running chains,
 *                        0 exactly when no model runs).
 *   pyvb_lds_get_model_convergence   iters[M], converged[M], llb[M], one entry per model (read from its first row), M = the
 *                        number of models (pyvb_lds_get_models; M = N on a handle without tied models).  Any pointer may be NULL.
 * Not built: thawing a converged model, models that span ranks. */
int pyvb_lds_iterate_until_model(pyvb_lds* h, int max_iters, double tol, int check_every, int* iters_run);
int pyvb_lds_get_model_convergence(pyvb_lds* h, int* iters, unsigned char* converged, double* llb);

/* HIP-event timing of the kernels on the handle's stream (for bench.py's roofline figures). */
int pyvb_lds_timing_enable(pyvb_lds* h, int on);
int pyvb_lds_timing_reset(pyvb_lds* h);
int pyvb_lds_timing_get(pyvb_lds* h, int kernel, double* total_ms, int* launches);
/* device-side diagnostics: warm-up lengths chosen for the segmented sweeps [N][2] */
int pyvb_lds_get_warmup(pyvb_lds* h, int* warm);
/* Wavefronts per replicate in the sweeps (the time axis is dealt out to W of them when there are few replicates;
 * pyvb_lds_create picks W, = 1 from about 1024 replicates on).  The setter lets a test run the W = 1 code path
 * (the one the headline workload uses) on a handful of replicates; results do not depend on W beyond rounding. */
int pyvb_lds_get_time_split(pyvb_lds* h, int* W);
int pyvb_lds_set_time_split(pyvb_lds* h, int W);

/* Multi-GPU: replicates are sharded over ranks; the only exchange is the ELBO all-reduce. */
int pyvb_comm_unique_id(char id[128]);
int pyvb_lds_comm_init(pyvb_lds* h, const char id[128], int rank, int world);
int pyvb_lds_comm_destroy(pyvb_lds* h);
/* The same exchange through the caller's own transport instead of RCCL: fn sums buf[0..count) over all ranks in place
 * (host memory, blocking, every rank calls it in the same order) and returns 0.  A rehearsal transport -- several ranks
 * on ONE GPU, where RCCL refuses duplicate devices, or hosts without a working RCCL: every collective then costs a
 * device-host round trip and a stream synchronisation, so it is never what a scaling number should be measured with. */
typedef int (*pyvb_host_allreduce_fn)(double* buf, size_t count, void* user);
int pyvb_lds_comm_init_host(pyvb_lds* h, pyvb_host_allreduce_fn fn, void* user, int rank, int world);

/* ------------------------------------------------------------------------------------------------
 * VB-PCA with missing data: the graph of examples/PCA_missing_data.py:31-42 --
 *   W = hstack(q Gaussian columns of dim d), Mu Gaussian(d), Beta = Gamma(d), Z_n ~ N(0, I),
 *   X_n ~ N(W * Z_n + Mu, Beta), X_n.observe(row with NaN for missing entries), n = 0..N-1.
 * One handle holds N rows of one model; with several GPUs the rows are sharded (N_total rows in all,
 * this handle's first row has global index row_offset) and the sums over n are all-reduced over RCCL.
 * Arrays: X[N][d], Z[N][q], W_mean[d][q] (row, col), W_var[q][d] (column i, entry k), Z_cov[q][q],
 * Mu_mean[d], Mu_var[d], X_rowvar[N] (variance of the missing entries of row n), beta_ab[2] = (qa, qb).
 * Limits: d <= 256, q <= 32. */
typedef struct pyvb_pca pyvb_pca;
int pyvb_pca_create(pyvb_pca** out, int device, long N, int d, int q, long N_total, long row_offset);
int pyvb_pca_destroy(pyvb_pca* h);
/* Constant parents of the W columns and of Mu (diagonal precisions), Gamma hyper-parameters (PCA_missing_data.py:31-34) */
int pyvb_pca_set_priors(pyvb_pca* h, const double* W_prior_mean, const double* W_prior_prec,
                        const double* Mu_prior_mean, const double* Mu_prior_prec, double beta_a0, double beta_b0);
/* [x.observe(row) for x in Xs] (gaussian.py:74-100): NaN = missing; rows may be fully, partially or not observed */
int pyvb_pca_set_data(pyvb_pca* h, const double* X);
/* Automatic relevance determination (Bishop's VB-PCA): column i of W gets the precision parent alpha_i = Gamma(d, a0_i, b0_i) in
 * place of its Constant one -- Ws = [Gaussian(d, pmu_i, Gamma(d, a0_i, b0_i)) for i in range(q)], which gaussian.py:55-61 accepts.
 * The column then sees pprec = (qa_i / qb_i) I (gaussian.py:113, nodes_todo.py:140-142), qa_i = a0_i + d / 2 (nodes_todo.py:125-128);
 * alpha_i.update() is qb_i = b0_i + 1/2 sum_k ((<W>[k][i] - pmu[k][i])^2 + var W[k][i]) (nodes_todo.py:130-138); the column's own
 * bound term takes 1/2 d (ln qa_i - ln qb_i) (nodes_todo.py:144-147, quirk Q2; PYVB_BOUND_EXACT: 1/2 d (psi(qa_i) - ln qb_i)), and
 * each alpha_i adds Gamma.log_lower_bound (nodes_todo.py:149-157) to parts[0], the W class.
 * pyvb_pca_set_column_precisions: a0[q], b0[q] and the initial qb[q] (the reference draws it at random, nodes_todo.py:119), all
 * finite and positive; call it after pyvb_pca_set_priors, whose W_prior_prec it replaces by qa / qb -- and which, called again,
 * gives the columns their Constant parents back.  pyvb_pca_iterate then runs [al.update() for al in alphas] in every pass, where
 * fetch_network puts it (after the Z_n; it commutes with them); stage-wise callers use pyvb_pca_update_column_precisions.
 * update / get on a handle without hyperpriors, a NULL handle or array, a value that is not finite and positive: PYVB_E_ARG. */
int pyvb_pca_set_column_precisions(pyvb_pca* h, const double* a0, const double* b0, const double* qb);  /* [q] each */
int pyvb_pca_get_column_precisions(pyvb_pca* h, double* qa, double* qb);                               /* [q]; NULL = skip */
int pyvb_pca_update_column_precisions(pyvb_pca* h);            /* [al.update() for al in alphas] */
/* Sparse loadings: column i of W gets the precision parent DiagonalGamma(d, a0_i, b0_i), a Gamma per entry, in place of its Constant
 * one -- Ws = [Gaussian(d, pmu_i, DiagonalGamma(d, a0_i, b0_i)) for i in range(q)], which gaussian.py:55-61 accepts.  Arrays are
 * [column i][row k], as W_prior_prec.  The column sees pprec = diag(qa_i / qb_i) (gaussian.py:113, nodes_todo.py:192-193),
 * qa_ik = a0_ik + 1/2 (nodes_todo.py:183-186); dg_i.update() is qb_ik = b0_ik + 1/2 ((<W>[k][i] - pmu[k][i])^2 + var W[k][i])
 * (nodes_todo.py:187-190); the column's own bound term takes 1/2 sum_k (ln qa_ik - ln qb_ik) -- the reference's
 * 1/2 ln prod_k (qa_ik / qb_ik) (nodes_todo.py:195-197) as a sum of logarithms, which does not overflow where entries are pruned --
 * (PYVB_BOUND_EXACT: 1/2 sum_k (psi(qa_ik) - ln qb_ik)), and each parent adds its DiagonalGamma.log_lower_bound
 * (nodes_todo.py:199-204) to parts[0], the W class.
 * pyvb_pca_set_entry_precisions: a0, b0 and the initial qb (the reference draws it at random, nodes_todo.py:177), all finite and
 * positive; call it after pyvb_pca_set_priors, whose W_prior_prec it replaces by qa / qb -- and which, called again, gives the
 * columns their Constant parents back.  All columns of W have one kind of parent: of this setter and
 * pyvb_pca_set_column_precisions the most recent call holds, and get / update of the other kind return PYVB_E_ARG.
 * pyvb_pca_iterate then runs [dg.update() for dg in parents] in every pass, behind the W update (fetch_network has it after the
 * Z_n; it commutes with them); stage-wise callers use pyvb_pca_update_entry_precisions.
 * update / get on a handle without these parents, a NULL handle or array, a value that is not finite and positive: PYVB_E_ARG. */
int pyvb_pca_set_entry_precisions(pyvb_pca* h, const double* a0, const double* b0, const double* qb);  /* [q][d] each */
int pyvb_pca_get_entry_precisions(pyvb_pca* h, double* qa, double* qb);                                /* [q][d]; NULL = skip */
int pyvb_pca_update_entry_precisions(pyvb_pca* h);             /* [dg.update() for dg in parents] */
/* The kind in force, PYVB_PARENTS_*, of the columns of W.  Needs no device.  PYVB_E_ARG: NULL. */
int pyvb_pca_get_column_parents(pyvb_pca* h, int* kind);
/* explicit posterior state; X_missing[N][d] supplies the posterior means of the missing entries only */
int pyvb_pca_set_state(pyvb_pca* h, const double* X_missing, const double* W_mean, const double* Z, const double* Z_cov,
                       const double* Mu_mean, const double* beta_b);
/* The X_n as Gaussian.__init__ leaves them (gaussian.py:70-72; observe() with NaN changes neither qmu nor qcov, :90-96):
 * a row that is not fully observed carries the posterior mean X_full[n] at ALL its d entries and the covariance
 * row_var[n] * I, messages with them, and is conditioned on its observed entries by its first update (:125-134).
 * Call after pyvb_pca_set_data; rows without missing entries are ignored.  Without this call the observed entries of a
 * partially observed row count as pinned from the start (what pyvb_pca_set_state describes). */
int pyvb_pca_set_unpinned_rows(pyvb_pca* h, const double* X_full, const double* row_var);
/* diagonals of the initial covariances of the W columns [q][d] and of Mu [d] (either may be NULL): read only by updates that
 * come before the first update of the node itself -- Z or Beta before W, Beta before Mu; the crawl order never does that */
int pyvb_pca_set_initial_variances(pyvb_pca* h, const double* W_var, const double* Mu_var);
int pyvb_pca_get_state(pyvb_pca* h, double* X, double* X_rowvar, double* W_mean, double* W_var, double* Z, double* Z_cov,
                       double* Mu_mean, double* Mu_var, double* beta_ab);
/* q_ln_det of the nodes (gaussian.py:120, the quantity of quirk Q1 that log_lower_bound reads, gaussian.py:147), as their
 * updates on THIS handle left it; NaN for a node that has not been updated on it (the reference, too, sets it only in
 * update()).  qld_W [q]; qld_Z, qld_Mu one double each (all Z_n share one); qld_X [N]: rows without any observed entry,
 * NaN for the others.  Any pointer may be NULL. */
int pyvb_pca_get_qld(pyvb_pca* h, double* qld_W, double* qld_Z, double* qld_Mu, double* qld_X);
/* The lower bound pyvb_pca_elbo and pyvb_pca_iterate form from now on (PYVB_BOUND_*; anything else: PYVB_E_ARG); the updates do not
 * depend on it.  pyvb_pca_get_logdets: ln det qcov where pyvb_pca_get_qld gives q_ln_det, same shapes, same NaN, kept in both
 * modes; any pointer may be NULL. */
int pyvb_pca_set_bound_mode(pyvb_pca* h, int mode);
int pyvb_pca_get_logdets(pyvb_pca* h, double* lnd_W, double* lnd_Z, double* lnd_Mu, double* lnd_X);
/* [w.update() for w in Ws]; [z.update() for z in Zs]; Xs[lo:hi] updates; Mu.update(); Beta.update()
 * (gaussian.py:102-134, nodes_todo.py:130-138).  Results are what the reference's order of node updates gives, call by call; the work
 * behind pyvb_pca_update_Z is scheduled lazily: the call forms the shared posterior covariance of the Z_n, the gains and the sum of
 * the new means (which is linear in the sum of x), and the rows of Z are written by the next pass over the rows -- normally the
 * pyvb_pca_update_X that follows, which then reads X once for both updates -- or by the first call that reads or replaces Z, X or
 * the parameters (pyvb_pca_get_state, the setters). */
int pyvb_pca_update_W(pyvb_pca* h);
int pyvb_pca_update_Z(pyvb_pca* h);
int pyvb_pca_update_X(pyvb_pca* h, long lo, long hi);
/* Xs[0].update() of the GLOBAL row 0 (the crawl order updates it alone, before Mu).  With a communicator attached every update
 * call is a collective: all ranks issue the same calls in the same order, pyvb_pca_update_X with their local part of the range
 * (possibly empty).  This one is the single-row step for every rank: the owner of global row 0 updates it, all ranks exchange
 * the change of sum x.  (Without a communicator pyvb_pca_update_X(h, 0, 1) takes this shortcut by itself; with one it does not
 * -- the two are different collectives -- and runs the general row-range update, which every rank matches by calling
 * pyvb_pca_update_X with its own, possibly empty, part.) */
int pyvb_pca_update_X0(pyvb_pca* h);
int pyvb_pca_update_Mu(pyvb_pca* h);
int pyvb_pca_update_Beta(pyvb_pca* h);
/* sum of log_lower_bound() per node class: parts[5] = W columns, Z_n, X_n, Mu, Beta (NULL: leave on the device) */
int pyvb_pca_elbo(pyvb_pca* h, double parts[5]);
/* niters passes of Network.learn's loop body (network.py:46-49) in the crawl order of fetch_network:
 * W columns, Z_0.., X_0, Mu, X_1.., Beta, lower bound */
int pyvb_pca_iterate(pyvb_pca* h, int niters);
/* Which kernel serves the sweep of an iteration -- the Z update and the X update of all rows (or all but row 0) in one pass over
 * X -- where the imputed entries may be left unstored.  pyvb_pca_create picks the kind: PAIRS for d > 192 from 512 rows per
 * compute unit on, COLUMNS otherwise.  The setter lets a test or an A/B run put a chosen kernel on a small handle; it may be
 * called between any two calls and touches nothing on the device.  q > 16, rows not yet pinned, partial ranges and an incoming
 * unstored range the pass cannot take in are written back whatever the kind.  Results do not depend on the kind beyond rounding.
 * An unknown kind: PYVB_E_ARG. */
#define PYVB_PCA_SWEEP_STORE   0   /* the imputed entries are written back (k_pca_pass12) */
#define PYVB_PCA_SWEEP_COLUMNS 1   /* left unstored, column-owning sweep (k_pca_pass12<.., LAZY>) */
#define PYVB_PCA_SWEEP_PAIRS   2   /* left unstored, pair-owning sweep (k_pca_pairs) */
int pyvb_pca_get_sweep(pyvb_pca* h, int* kind);
int pyvb_pca_set_sweep(pyvb_pca* h, int kind);
int pyvb_pca_sync(pyvb_pca* h);
int pyvb_pca_comm_init(pyvb_pca* h, const char id[128], int rank, int world);
int pyvb_pca_comm_init_host(pyvb_pca* h, pyvb_host_allreduce_fn fn, void* user, int rank, int world);

/* ------------------------------------------------------------------------------------------------
 * Generic graphs, node by node (network.py:40-56 over arbitrary node lists; src/tests.py:9-202): every posterior,
 * constant, message and temporary of one graph lives in a device arena of doubles; the work of one reference method --
 *   Gaussian.update gaussian.py:102-134, Gaussian.log_lower_bound :136-151, Gaussian.pass_up_m1_m2 :179-183,
 *   Addition.pass_up_m1_m2 / pass_down_* node.py:95-129, Multiplication.* node.py:182-276, hstack.* nodes_todo.py:33-62,
 *   Gamma.* :125-157, DiagonalGamma.* :183-204, Wishart.* :224-234, Constant.* node.py:304-311
 * -- is a TAPE of small dense operations on arena offsets (records of 8 int32: opcode, dst, a, b, m, n, p, flags; the
 * opcodes are documented in pyvb_amd/csrc/k_tape.hip and mirrored by pyvb_amd/generic.py), interpreted by one workgroup
 * per launch.  Tapes are uploaded once and replayed (the graph is static).  pyvb_graph_tape_create checks every extent a
 * record touches against the arena (PYVB_E_ARG names the record); gather / scatter indices are data: the kernel skips one
 * that points outside and the next pyvb_graph_sync / pyvb_graph_read returns PYVB_E_ARG.  It also refuses, as malformed, a
 * T_COPY2D, T_FILL or T_GEMM record of more than 2^22 elements (m n; the k of a T_GEMM is not limited) and a T_DIAG with
 * flags 1 or T_CHOLINV record with m m > 2^22: up to there the interpreter's division-free row / column of an element is
 * proven exact (TAPE_MAX_ELEMS, pyvb_amd/csrc/tape.h).  Records of the other opcodes are limited by the arena alone.  A
 * T_SCATTER whose index pairs repeat leaves an unspecified one of the colliding values (with T_ACC: an unordered
 * read-modify-write that may lose terms); give it distinct pairs. */
typedef struct pyvb_graph pyvb_graph;
int pyvb_graph_create(pyvb_graph** out, int device, size_t arena_doubles);
int pyvb_graph_destroy(pyvb_graph* g);
int pyvb_graph_write(pyvb_graph* g, size_t offset, const double* src, size_t n);
int pyvb_graph_read(pyvb_graph* g, size_t offset, double* dst, size_t n);
int pyvb_graph_tape_create(pyvb_graph* g, const int* ops, int nops, int* tape_id);
/* Optional: how pyvb_graph_tape_run issues the tape -- launches[nl][2] = (first block, number of blocks), in order, and
 * blocks[nb][2] = (first record, number of records); the blocks of one launch run side by side, one workgroup each (the
 * updates of nodes none of which reads what another writes: [z.update() for z in Zs] of a PCA-like graph).  The caller
 * guarantees that independence; blocks and launches must tile the tape in order (checked).  Without a program one workgroup
 * interprets the whole tape.  What a block "writes" includes the GAPS of a strided destination: the extent of a COPY2D or FILL
 * with ld > cols is the whole span (rows - 1) * ld + cols, which a block may hold in LDS from its start and write back at its
 * end -- that span, gaps included, must be disjoint from everything any other block of the same launch writes. */
int pyvb_graph_tape_set_program(pyvb_graph* g, int tape_id, const int* blocks, int nblocks, const int* launches, int nlaunches);
int pyvb_graph_tape_run(pyvb_graph* g, int tape_id);
int pyvb_graph_tape_destroy(pyvb_graph* g, int tape_id);
int pyvb_graph_sync(pyvb_graph* g);

#ifdef __cplusplus
}
#endif
#endif
