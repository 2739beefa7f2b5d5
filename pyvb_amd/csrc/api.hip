// Host side of libpyvb_hip.so: handle lifetime, argument checks, host<->device copies, the streams of pyvb_lds_iterate, timing,
// and the RCCL all-reduce of the lower bound.  The dependency tracking that decides which kernels a node-level call needs is
// lds_flow.h (over LdsState of lds_state.h), instantiated here over the launchers.
#include "common.h"
#include "lds_flow.h"
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <cmath>
#include <vector>
#include <mutex>
#include <dlfcn.h>

static thread_local char g_err[512] = "";

void pyvb_set_error(const char* fmt, ...) {
    va_list ap; va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

int pyvb_hip_fail(hipError_t e, const char* what, const char* file, int line) {
    pyvb_set_error("HIP error %d (%s) in %s at %s:%d", (int)e, hipGetErrorString(e), what, file, line);
    return PYVB_E_HIP;
}

TimedLaunch::TimedLaunch(pyvb_lds* h_, int k_, hipStream_t s_) : h(h_), slot(-1), s(s_ ? s_ : h_->stream) {
    if (!h->timing) return;
    if (h->pool_used == PYVB_EVENT_POOL) pyvb_timing_resolve(h);     // pool exhausted: drain (synchronises)
    slot = h->pool_used++;
    h->pool[slot].kernel = k_;
    if (hipEventRecord(h->pool[slot].e0, s) != hipSuccess) { h->timing_errors += 1; h->pool[slot].kernel = -1; }
}
TimedLaunch::~TimedLaunch() {
    if (slot >= 0 && hipEventRecord(h->pool[slot].e1, s) != hipSuccess) { h->timing_errors += 1; h->pool[slot].kernel = -1; }
}

void pyvb_timing_resolve(pyvb_lds* h) {
    for (int i = 0; i < h->pool_used; ++i) {
        float ms = 0;
        if (h->pool[i].kernel < 0) continue;                          // an event of this pair was never recorded
        if (hipEventSynchronize(h->pool[i].e1) == hipSuccess && hipEventElapsedTime(&ms, h->pool[i].e0, h->pool[i].e1) == hipSuccess) {
            h->timers[h->pool[i].kernel].total_ms += ms;
            h->timers[h->pool[i].kernel].launches += 1;
        } else {
            h->timing_errors += 1;
        }
    }
    h->pool_used = 0;
}

extern "C" {

const char* pyvb_last_error(void) { return g_err; }
int pyvb_version(void) { return 111; }

int pyvb_device_count(int* count) {
    ARGCHK(count, "count is NULL");
    HIPCHK(hipGetDeviceCount(count));
    return PYVB_OK;
}

// the buffers of one side's known channels (KnownChannels, common.h); nothing on a handle without them
static int known_alloc(pyvb_lds* h, int side) {
    KnownChannels& k = h->known[side];
    if (!k.width) return PYVB_OK;
    const size_t n = h->N, D = h->D, rows = lds_known_rows(h, side), W = k.width;
    int rc;
    if ((rc = h->mem.zeros(&k.in, n * h->T * W)) || (rc = h->mem.zeros(&k.mean, n * rows * W)) || (rc = h->mem.zeros(&k.var, n * W * rows)) ||
        (rc = h->mem.alloc((void**)&k.qld, n * W * sizeof(double), 0xFF)) || (rc = h->mem.alloc((void**)&k.lnd, n * W * sizeof(double), 0xFF)) ||    // NaN
        (rc = h->mem.zeros(&k.pm, rows * W)) || (rc = h->mem.zeros(&k.pp, W * rows)) || (rc = h->mem.zeros(&k.pld, W)) ||
        (rc = h->mem.zeros(&k.gram, n * W * W)) || (rc = h->mem.zeros(&k.cross_lhs, n * rows * W)) || (rc = h->mem.zeros(&k.cross_x, n * W * D)) ||
        (rc = h->mem.zeros(&k.saved, n * rows * D))) return rc;
    return PYVB_OK;
}

// The one creation path; lengths null: every chain has T nodes, model null: every replicate is a model.  Arguments are checked
// and, where a combination is not served, refused before the first HIP call; *out is written once, when everything exists.
// P: known inputs that drive the states (pyvb_lds_create_inputs), 0: none.  Pv: known regressors in the output equation
// (pyvb_lds_create_regressors), 0: none.
static int lds_create(pyvb_lds** out, int device, int N, int T, int D, int K, int noise_kind, const int* lengths, const int* model, int P = 0, int Pv = 0) {
    ARGCHK(out, "out is NULL");
    ARGCHK(N >= 1, "N must be >= 1");
    bool ragged = false, tied = false;
    int rc = model ? Replicates::check_models(N, model, &tied) : PYVB_OK;
    if (rc) return rc;
    if (tied && noise_kind == PYVB_NOISE_WISHART) {
        pyvb_set_error("chains that share A, C, Q, R are served with DiagonalGamma and Gamma noise only, not with Wishart noise (k_wishart.hip)");
        return PYVB_E_UNSUPPORTED;
    }
    if (tied && (D > 64 || K > 64)) {
        pyvb_set_error("chains that share A, C, Q, R are served for max(D, K) <= 64 only, not in the 128-wide class (k_big.hip): D = %d, K = %d", D, K);
        return PYVB_E_UNSUPPORTED;
    }
    ARGCHK(T >= 2, "T must be >= 2 (a chain needs X_0 and X_{T-1})");
    ARGCHK(D >= 1 && D <= 128, "latent dimension D must be in 1..128");
    ARGCHK(K >= 1 && K <= 128, "observed dimension K must be in 1..128");
    ARGCHK(noise_kind == PYVB_NOISE_DIAGONAL_GAMMA || noise_kind == PYVB_NOISE_GAMMA || noise_kind == PYVB_NOISE_WISHART, "unknown noise kind");
    if (Pv && noise_kind == PYVB_NOISE_WISHART) {
        pyvb_set_error("regressors in the output equation are served with DiagonalGamma and Gamma noise only, not with Wishart noise (k_wishart.hip)");
        return PYVB_E_UNSUPPORTED;
    }
    if (Pv && (D > 64 || K + 2 * P + Pv > 64)) {
        pyvb_set_error("regressors in the output equation ride as Pv extra output channels and are served for max(D, K + 2 P + Pv) <= 64 only, "
                       "not in the 128-wide class (k_big.hip): D = %d, K = %d, P = %d, Pv = %d", D, K, P, Pv);
        return PYVB_E_UNSUPPORTED;
    }
    if (!Pv && P && noise_kind == PYVB_NOISE_WISHART) {
        pyvb_set_error("inputs that drive the states are served with DiagonalGamma and Gamma noise only, not with Wishart noise (k_wishart.hip)");
        return PYVB_E_UNSUPPORTED;
    }
    if (!Pv && P && (D > 64 || K + 2 * P > 64)) {
        pyvb_set_error("inputs that drive the states ride as 2 P extra output channels and are served for max(D, K + 2 P) <= 64 only, "
                       "not in the 128-wide class (k_big.hip): D = %d, K = %d, P = %d", D, K, P);
        return PYVB_E_UNSUPPORTED;
    }
    if (lengths && (rc = Replicates::check_lengths(N, T, lengths, &ragged))) return rc;
    if (ragged && noise_kind == PYVB_NOISE_WISHART) {
        pyvb_set_error("chains of unequal length are served with DiagonalGamma and Gamma noise only, not with Wishart noise (k_wishart.hip)");
        return PYVB_E_UNSUPPORTED;
    }
    if (ragged && (D > 64 || K > 64)) {
        pyvb_set_error("chains of unequal length are served for max(D, K) <= 64 only, not in the 128-wide class (k_big.hip): D = %d, K = %d", D, K);
        return PYVB_E_UNSUPPORTED;
    }
    int ndev = 0;
    HIPCHK(hipGetDeviceCount(&ndev));
    ARGCHK(device >= 0 && device < ndev, "no such device");
    HIPCHK(hipSetDevice(device));
    pyvb_lds* h = new pyvb_lds();       // value-initialised: every pointer null, every flag false
    h->device = device; h->N = N; h->T = T; h->D = D; h->K = K; h->noise = noise_kind; h->known[0].width = P; h->known[1].width = Pv;
    // (with inputs and regressors the gains, the statistics and the kernels that form them are those of K + 2 P + Pv outputs:
    // k_known.hip)
    const LdsGeometry g = lds_geometry(N, T, D, K + 2 * P + Pv, noise_kind);     // geometry.h: the shape class, the chunks, the time split, the extents
    h->L = g.L; h->big = g.big; h->dense = g.dense;
    h->nchunk = g.nchunk; h->chunk_len = g.chunk_len; h->W = g.W;
    // (lengths that all equal T, models of one replicate each: a plain handle, len / mstart / first stay null)
    h->rep.init(N, T, ragged ? lengths : nullptr, tied ? model : nullptr);
    const Layout& L = h->L;
#define TRY(x) CREATE_TRY(x, pyvb_lds_destroy, h)
#define TRYHIP(x) CREATE_TRYHIP(x, pyvb_lds_destroy, h)
#define dev_alloc(p, n) h->mem.zeros(p, n)
    if (h->big) TRY(big_prepare_kernels());
    TRYHIP(hipStreamCreate(&h->stream));
    TRYHIP(hipStreamCreate(&h->side));
    TRYHIP(hipEventCreateWithFlags(&h->ev_params, hipEventDisableTiming));
    TRYHIP(hipEventCreateWithFlags(&h->ev_elbo, hipEventDisableTiming));
    h->pool = (EventPair*)calloc(PYVB_EVENT_POOL, sizeof(EventPair));
    for (int i = 0; i < PYVB_EVENT_POOL; ++i) { TRYHIP(hipEventCreate(&h->pool[i].e0)); TRYHIP(hipEventCreate(&h->pool[i].e1)); }
    const size_t n = (size_t)N;
    TRY(dev_alloc(&h->Y, n * T * K));
    TRY(dev_alloc(&h->Syy, n * K));
    TRY(dev_alloc(&h->X[0], n * T * L.DP));
    TRY(dev_alloc(&h->X[1], n * T * L.DP));
    TRY(dev_alloc(&h->A_mean, n * D * D));
    TRY(dev_alloc(&h->A_var, n * D * D));
    TRY(dev_alloc(&h->C_mean, n * K * D));
    TRY(dev_alloc(&h->C_var, n * D * K));
    TRY(dev_alloc(&h->Q_a, n * D)); TRY(dev_alloc(&h->Q_b, n * D));
    TRY(dev_alloc(&h->R_a, n * K)); TRY(dev_alloc(&h->R_b, n * K));
    TRY(dev_alloc(&h->qld_A, n * D)); TRY(dev_alloc(&h->qld_C, n * D));
    TRY(dev_alloc(&h->Sigma, n * 3 * D * D)); TRY(dev_alloc(&h->Sigma_new, n * 3 * D * D));
    TRY(dev_alloc(&h->qld_x, n * 3)); TRY(dev_alloc(&h->qld_x_new, n * 3));
    TRY(dev_alloc(&h->lnd_A, n * D)); TRY(dev_alloc(&h->lnd_C, n * D));
    TRY(dev_alloc(&h->lnd_x, n * 3)); TRY(dev_alloc(&h->lnd_x_new, n * 3));
    TRY(dev_alloc(&h->gains, n * L.gains_total));
    TRY(dev_alloc(&h->scratch, g.scratch));
    TRY(dev_alloc(&h->zeros, 128));
    TRY(dev_alloc(&h->U, n * T * L.DP));                        // the c_t cache between a forward sweep and the backward one behind it
    TRY(h->mem.alloc((void**)&h->warm, n * 2 * sizeof(int)));
    TRY(dev_alloc(&h->stats, g.stats));
    TRY(dev_alloc(&h->mom, g.mom));
    TRY(dev_alloc(&h->sxx, g.sxx));
    if (g.U2) TRY(dev_alloc(&h->U2, g.U2));
    TRY(dev_alloc(&h->trash, g.trash));
    TRY(dev_alloc(&h->resQ, n * D)); TRY(dev_alloc(&h->resR, n * K));
    TRY(dev_alloc(&h->elbo, n * 6)); TRY(dev_alloc(&h->elbo_sum, 8));
    TRY(dev_alloc(&h->elbo_hist, (size_t)PYVB_ELBO_HISTORY * 8));
    TRY(h->mem.alloc((void**)&h->status, n * sizeof(int)));
    TRY(h->mem.alloc((void**)&h->active, n, 1));
    TRY(h->mem.alloc((void**)&h->counted, n, 1));
    TRY(h->mem.alloc((void**)&h->conv, n));
    TRY(h->mem.alloc((void**)&h->conv_iters, n * sizeof(int)));
    TRY(h->mem.alloc((void**)&h->conv_llb, n * sizeof(double), 0xFF));     // (all-ones bytes = NaN: no test has seen a bound yet)
    TRYHIP(hipHostMalloc((void**)&h->running_host, sizeof(double), hipHostMallocDefault));
    TRYHIP(hipEventCreateWithFlags(&h->ev_check, hipEventDisableTiming));
    if (ragged) {
        TRY(h->mem.alloc((void**)&h->len, n * sizeof(int)));
        TRYHIP(hipMemcpy(h->len, lengths, n * sizeof(int), hipMemcpyHostToDevice));
    }
    if (tied) {
        const Replicates& r = h->rep;
        TRY(h->mem.alloc((void**)&h->mstart, r.model_starts().size() * sizeof(int)));
        TRY(h->mem.alloc((void**)&h->first, n));
        TRYHIP(hipMemcpy(h->mstart, r.model_starts().data(), r.model_starts().size() * sizeof(int), hipMemcpyHostToDevice));
        TRYHIP(hipMemcpy(h->first, r.first_flags().data(), n, hipMemcpyHostToDevice));
    }
    h->status_host.assign(n, 0);
    h->reported.assign(n, 0);
    TRY(dev_alloc(&h->pri_block, g.priors));       // one block, cut below in the order LdsGeometry.priors lists
    TRY(dev_alloc(&h->w0, L.DP));
    double* p = h->pri_block;
    h->pri.x0_mean = p; p += D; h->pri.x0_prec = p; p += D * D;
    h->pri.A_pm = p; p += D * D; h->pri.A_pp = p; p += D * D;
    h->pri.C_pm = p; p += K * D; h->pri.C_pp = p; p += D * K;
    h->pri.Q_a0 = p; p += D; h->pri.Q_b0 = p; p += D; h->pri.R_a0 = p; p += K; h->pri.R_b0 = p; p += K;
    h->pri.A_obs = p; p += D * D; h->pri.C_obs = p; p += K * D;
    h->pri.A_pld = p; p += D; h->pri.C_pld = p; p += D;
    h->pri.Q_w0 = p; p += D * D; h->pri.R_w0 = p; p += K * K;
    if (h->dense) {
        TRY(dev_alloc(&h->Q_w, n * D * D)); TRY(dev_alloc(&h->R_w, n * K * K));
        TRY(dev_alloc(&h->Qbar, n * D * D)); TRY(dev_alloc(&h->Rbar, n * K * K));
        TRY(dev_alloc(&h->lnd, n * 4));
        TRY(dev_alloc(&h->QA, n * D * D)); TRY(dev_alloc(&h->RC, n * K * D));
        TRY(dev_alloc(&h->trA, n * D)); TRY(dev_alloc(&h->trC, n * D));
        TRY(dev_alloc(&h->A_cov, n * D * cov_stride(D))); TRY(dev_alloc(&h->C_cov, n * D * cov_stride(K)));
        TRY(dev_alloc(&h->SyyF, n * K * K));
        TRY(dev_alloc(&h->RQ, n * D * D)); TRY(dev_alloc(&h->RR, n * K * K));
        TRY(dev_alloc(&h->SG, g.SG));
        TRY(dev_alloc(&h->ldm, n * 2 * D));
    }
    TRYHIP(hipMemset(h->pri.A_obs, 0xFF, ((size_t)D * D + (size_t)K * D) * sizeof(double)));     // all-ones bytes = NaN = nothing observed
    if (P || Pv) { TRY(dev_alloc(&h->Yt, n * T * (K + 2 * P + Pv))); TRY(dev_alloc(&h->Ct, n * (K + 2 * P + Pv) * D)); }
    for (int side = 0; side < 2; ++side) TRY(known_alloc(h, side));
    h->st.T = T;
    h->st.fresh = (unsigned char*)calloc(T, 1);
    h->world = 1;
    // q_ln_det is undefined until a node has been updated (the reference raises AttributeError)
    {
        std::vector<double> nanv(n * (size_t)(D > 3 ? D : 3), NAN);
        TRYHIP(hipMemcpy(h->qld_x, nanv.data(), n * 3 * sizeof(double), hipMemcpyHostToDevice));
        TRYHIP(hipMemcpy(h->qld_A, nanv.data(), n * D * sizeof(double), hipMemcpyHostToDevice));
        TRYHIP(hipMemcpy(h->qld_C, nanv.data(), n * D * sizeof(double), hipMemcpyHostToDevice));
        TRYHIP(hipMemcpy(h->lnd_x, nanv.data(), n * 3 * sizeof(double), hipMemcpyHostToDevice));
        TRYHIP(hipMemcpy(h->lnd_A, nanv.data(), n * D * sizeof(double), hipMemcpyHostToDevice));
        TRYHIP(hipMemcpy(h->lnd_C, nanv.data(), n * D * sizeof(double), hipMemcpyHostToDevice));
    }
#undef dev_alloc
#undef TRY
#undef TRYHIP
    *out = h;
    return PYVB_OK;
}

int pyvb_lds_create(pyvb_lds** out, int device, int N, int T, int D, int K, int noise_kind) {
    return lds_create(out, device, N, T, D, K, noise_kind, nullptr, nullptr);
}
int pyvb_lds_create_lengths(pyvb_lds** out, int device, int N, int T, int D, int K, int noise_kind, const int* lengths) {
    return lds_create(out, device, N, T, D, K, noise_kind, lengths, nullptr);
}
int pyvb_lds_create_tied(pyvb_lds** out, int device, int N, int T, int D, int K, int noise_kind, const int* lengths, const int* model) {
    return lds_create(out, device, N, T, D, K, noise_kind, lengths, model);
}

int pyvb_lds_create_inputs(pyvb_lds** out, int device, int N, int T, int D, int K, int P, int noise_kind, const int* lengths) {
    ARGCHK(P >= 1, "P must be >= 1 (pyvb_lds_create makes a handle without inputs)");
    return lds_create(out, device, N, T, D, K, noise_kind, lengths, nullptr, P);
}

int pyvb_lds_create_regressors(pyvb_lds** out, int device, int N, int T, int D, int K, int P, int Pv, int noise_kind, const int* lengths) {
    ARGCHK(Pv >= 1, "Pv must be >= 1 (pyvb_lds_create and pyvb_lds_create_inputs make handles without regressors)");
    ARGCHK(P >= 0, "P must be >= 0");
    return lds_create(out, device, N, T, D, K, noise_kind, lengths, nullptr, P, Pv);
}

int pyvb_lds_get_models(pyvb_lds* h, int* model) {
    ARGCHK(h, "handle is NULL");
    ARGCHK(model, "model is NULL");
    for (int n = 0; n < h->N; ++n) model[n] = h->rep.model(n);
    return PYVB_OK;
}

int pyvb_lds_destroy(pyvb_lds* h) {
    if (!h) return PYVB_OK;
    (void)hipSetDevice(h->device);
    if (h->stream) (void)hipStreamSynchronize(h->stream);
    if (h->side) (void)hipStreamSynchronize(h->side);
    pyvb_lds_comm_destroy(h);
    if (h->ev_params) (void)hipEventDestroy(h->ev_params);
    if (h->ev_elbo) (void)hipEventDestroy(h->ev_elbo);
    if (h->ev_check) (void)hipEventDestroy(h->ev_check);
    if (h->running_host) (void)hipHostFree(h->running_host);
    if (h->side) (void)hipStreamDestroy(h->side);
    h->mem.release_all();
    if (h->pool) {
        for (int i = 0; i < PYVB_EVENT_POOL; ++i) { if (h->pool[i].e0) (void)hipEventDestroy(h->pool[i].e0); if (h->pool[i].e1) (void)hipEventDestroy(h->pool[i].e1); }
        free(h->pool);
    }
    if (h->stream) (void)hipStreamDestroy(h->stream);
    free(h->st.fresh);
    delete h;
    return PYVB_OK;
}

static int join_elbo(pyvb_lds* h);
// Every entry point but pyvb_lds_iterate first lets the main stream wait for a lower-bound evaluation that the last
// pyvb_lds_iterate may have left in flight on the side stream (it reads states and parameters).
#define ENTER(h) do { ENTER_DEVICE(h); if ((h)->elbo_in_flight) { int _rc = join_elbo(h); if (_rc) return _rc; } } while (0)

// ---- Which kernels a call launches, and the events it raises, is LdsFlow of lds_flow.h: one copy, compiled here over the
// launchers and in tests/c/lds_flow_driver.cpp over a recorder.  LdsDevice is what it drives here: every method is one launcher.
static int launch_parents(pyvb_lds* h, int kind, int which, bool derive);
static int form_lnd_x(pyvb_lds* h);
struct LdsDevice {
    typedef hipStream_t stream_t;
    pyvb_lds* h;
    hipStream_t main_stream() const { return h->stream; }
    int prep() { return launch_prep(h); }
    int known_gains(int side) { return launch_known_gains(h, side); }
    int wexpect() { return launch_wexpect(h); }
    int dense_pre() { return launch_dense_pre(h); }
    int sweep(int direction, int src, bool read_cache, bool keep_x) { return launch_sweep(h, direction, src, read_cache, keep_x); }
    int step(int t) { return launch_step(h, t); }
    int stats(bool with_sxx) { return launch_stats(h, with_sxx); }
    int moments(bool sxx_from_sweep) { return launch_moments(h, sxx_from_sweep); }
    int tie_moments() { return launch_tie(h, h->mom, (size_t)3 * h->D * h->D + (size_t)h->K * h->D + h->D); }
    int tie_syy() { return launch_tie(h, h->Syy, h->K); }
    int known_moments(int side) { return launch_known_moments(h, side); }
    int known_H(int side) { return launch_known_H(h, side); }
    int known_cols(int side) { return launch_known_cols(h, side); }
    int known_resid(int side) { return launch_known_resid(h, side); }
    int resid(int which) { return launch_resid(h, which); }
    int wresid(int which, int update, bool use_sg) { return launch_wresid(h, which, update, use_sg); }
    int cols(int which, int c0, int c1, int fuse = 0) { return launch_cols(h, which, c0, c1, fuse); }
    int cols_dense(int which, int c0, int c1) { return launch_cols_dense(h, which, c0, c1); }
    int noise(int which) { return launch_noise(h, which); }
    int parents(int kind, int which, bool derive) { return launch_parents(h, kind, which, derive); }
    int syy() { return launch_syy(h); }
    int syy_missing() { return launch_syy_missing(h); }
    int syy_full() { return launch_syy_full(h); }
    int missing_ent_dense(int diag_cov) { return launch_missing_ent_dense(h, diag_cov); }
    int impute() { return launch_impute(h); }
    int impute_dense() { return launch_impute_dense(h); }
    int elbo(hipStream_t stream) { return launch_elbo(h, stream); }
    int known_elbo(int side, hipStream_t stream) { return launch_known_elbo(h, side, stream); }
    int elbo_dense() { return launch_elbo_dense(h); }
    int carry_x(int src) { return launch_carry(h, h->X[src], h->X[1 - src], (size_t)h->T * h->L.DP); }
    int carry_classes() {
        int rc;
        if ((rc = launch_carry(h, h->Sigma_new, h->Sigma, (size_t)3 * h->D * h->D))) return rc;
        if ((rc = launch_carry(h, h->qld_x_new, h->qld_x, 3))) return rc;
        return launch_carry(h, h->lnd_x_new, h->lnd_x, 3);
    }
    void swap_classes() {
        double* t = h->Sigma; h->Sigma = h->Sigma_new; h->Sigma_new = t;
        t = h->qld_x; h->qld_x = h->qld_x_new; h->qld_x_new = t;
        t = h->lnd_x; h->lnd_x = h->lnd_x_new; h->lnd_x_new = t;
    }
    int join_elbo() { return ::join_elbo(h); }
    int form_lnd_x() { return ::form_lnd_x(h); }
};
static LdsFlow<LdsDevice> flow(pyvb_lds* h) {
    const KnownChannels* k = h->known;
    return {h->st, {h->T, h->N, h->D, h->dense, h->big, h->has_missing, h->bound, &h->rep, h->parents,
                    {k[0].width, k[1].width}, {k[0].set, k[1].set}, {k[0].priors_set, k[1].priors_set}}, {h}};
}
static int settle_parked(pyvb_lds* h) { return flow(h).settle_parked(); }

static int h2d(pyvb_lds* h, double* dst, const double* src, size_t n) { return to_device(h->stream, dst, src, n); }
static int d2h(pyvb_lds* h, double* dst, const double* src, size_t n) { return to_host(h->stream, dst, src, n); }

// A handle with chain lengths: rows t >= T_n of a host array [N][T][per] that a getter has just filled (after the sync) are
// padding, not nodes; they read as `value` whatever the device buffer holds there.
static void fill_padding(const pyvb_lds* h, double* a, size_t per, double value) {
    if (!h->rep.ragged() || !a) return;
    for (size_t n = 0; n < (size_t)h->N; ++n)
        for (size_t i = ((size_t)n * h->T + h->rep.length((int)n)) * per; i < (size_t)(n + 1) * h->T * per; ++i) a[i] = value;
}

// ln det of a symmetric positive definite matrix (Constant.lndet, node.py:301-302)
static int host_lndet(const double* Ain, int D, double* out) {
    std::vector<double> A(Ain, Ain + (size_t)D * D);
    double s = 0.0;
    for (int j = 0; j < D; ++j) {
        double piv = A[j * D + j];
        for (int k = 0; k < j; ++k) piv -= A[j * D + k] * A[j * D + k];
        if (!(piv > 0.0)) return PYVB_E_LINALG;
        double d = sqrt(piv);
        A[j * D + j] = d; s += log(d);
        for (int i = j + 1; i < D; ++i) {
            double v = A[i * D + j];
            for (int k = 0; k < j; ++k) v -= A[i * D + k] * A[j * D + k];
            A[i * D + j] = v / d;
        }
    }
    *out = 2.0 * s;
    return PYVB_OK;
}

int pyvb_lds_set_priors(pyvb_lds* h, const double* x0_mean, const double* x0_prec,
                        const double* A_pm, const double* A_pp, const double* C_pm, const double* C_pp,
                        const double* Q_a0, const double* Q_b0, const double* R_a0, const double* R_b0) {
    ENTER(h);
    ARGCHK(x0_mean && x0_prec && A_pm && A_pp && C_pm && C_pp, "the priors of X_0 and of the columns are required");
    ARGCHK(h->dense || (Q_a0 && Q_b0 && R_a0 && R_b0), "the Gamma priors of Q and R are required");
    const int D = h->D, K = h->K, N = h->N;
    for (int i = 0; i < D * D; ++i) ARGCHK(A_pp[i] > 0.0, "A_prior_prec must be positive");
    for (int i = 0; i < D * K; ++i) ARGCHK(C_pp[i] > 0.0, "C_prior_prec must be positive");
    if (host_lndet(x0_prec, D, &h->pri.x0_lndet) != PYVB_OK) { pyvb_set_error("x0_prec is not positive definite"); return PYVB_E_LINALG; }
    int rc;
    if ((rc = h2d(h, h->pri.x0_mean, x0_mean, D))) return rc;
    if ((rc = h2d(h, h->pri.x0_prec, x0_prec, (size_t)D * D))) return rc;
    if (!h->big && (rc = launch_w0(h))) return rc;         // (the 128-wide class forms L0 m0 in k_prep_big)
    if ((rc = h2d(h, h->pri.A_pm, A_pm, (size_t)D * D))) return rc;
    if ((rc = h2d(h, h->pri.A_pp, A_pp, (size_t)D * D))) return rc;
    if ((rc = h2d(h, h->pri.C_pm, C_pm, (size_t)K * D))) return rc;
    if ((rc = h2d(h, h->pri.C_pp, C_pp, (size_t)D * K))) return rc;
    {   // ln det of the diagonal prior precision of every column (Constant.lndet of the parents, node.py:301-302)
        std::vector<double> ld(2 * (size_t)D, 0.0);
        for (int i = 0; i < D; ++i) {
            for (int k = 0; k < D; ++k) ld[i] += log(A_pp[(size_t)i * D + k]);
            for (int k = 0; k < K; ++k) ld[D + i] += log(C_pp[(size_t)i * K + k]);
        }
        HIPCHK(hipMemcpyAsync(h->pri.A_pld, ld.data(), 2 * (size_t)D * sizeof(double), hipMemcpyHostToDevice, h->stream));
        HIPCHK(hipStreamSynchronize(h->stream));
    }
    if (!h->dense) {        // (the Wishart priors come through pyvb_lds_set_wishart_priors)
        if ((rc = h2d(h, h->pri.Q_a0, Q_a0, D))) return rc;
        if ((rc = h2d(h, h->pri.Q_b0, Q_b0, D))) return rc;
        if ((rc = h2d(h, h->pri.R_a0, R_a0, K))) return rc;
        if ((rc = h2d(h, h->pri.R_b0, R_b0, K))) return rc;
        // qa is fixed by the graph: update_a, nodes_todo.py:125-128 (Gamma: +0.5*child.shape[0] per child)
        // and :183-186 (DiagonalGamma: +0.5 per child); Q has T-1 children X_1.., R has T children Y_t
        std::vector<double> qa((size_t)N * D), ra((size_t)N * K);
        // the children of replicate n's Q and R: its own chain's, or those of every chain of its model (pyvb_lds_create_tied)
        std::vector<long> cq, cr;
        h->rep.children(cq, cr);
        for (int n = 0; n < N; ++n) {
            const long nq = cq[n], nr = cr[n];
            for (int k = 0; k < D; ++k)
                qa[(size_t)n * D + k] = (h->noise == PYVB_NOISE_GAMMA) ? Q_a0[0] + 0.5 * D * nq : Q_a0[k] + 0.5 * nq;
            for (int k = 0; k < K; ++k)
                ra[(size_t)n * K + k] = (h->noise == PYVB_NOISE_GAMMA) ? R_a0[0] + 0.5 * K * nr : R_a0[k] + 0.5 * nr;
        }
        if ((rc = h2d(h, h->Q_a, qa.data(), qa.size()))) return rc;
        if ((rc = h2d(h, h->R_a, ra.data(), ra.size()))) return rc;
        HIPCHK(hipStreamSynchronize(h->stream));       // qa, ra are about to go out of scope
    }
    h->parents[0].clear(); h->parents[1].clear();      // the columns have Constant parents again (the setters of others come after)
    h->st.parameters_changed();
    return PYVB_OK;
}

// ---- The precision parents of the columns of A / C: a Gamma per column (automatic relevance determination, k_ard.hip: k_ard) or a
// DiagonalGamma per column, a precision of its own for every entry (k_ard.hip: k_entry).  Which kind a matrix has, the checks and
// the staging are column_parents.h; a setter is gate, check, stage, upload, launch, commit.
static ParentWords lds_words(int which) { return {which == 0 ? "A" : "C", false}; }

// need: the kind a getter or an update serves; 0: a setter, which any matrix admits
static int parents_gate(const pyvb_lds* h, int which, int need) {
    ARGCHK(h, "handle is NULL");
    ARGCHK(which == 0 || which == 1, "which must be 0 (A) or 1 (C)");
    return need ? h->parents[which].require(need, lds_words(which)) : PYVB_OK;
}

static int launch_parents(pyvb_lds* h, int kind, int which, bool derive) {
    return kind == PARENTS_GAMMA ? launch_ard(h, which, derive) : launch_entry(h, which, derive);
}

// extent of a0 / b0 / a replicate's qb, and the rows per column of those arrays (0: one value per column)
static size_t parents_per(const pyvb_lds* h, int which, int kind, size_t* rows) {
    *rows = kind == PARENTS_GAMMA ? 0 : (size_t)(which == 0 ? h->D : h->K);
    return kind == PARENTS_GAMMA ? (size_t)h->D : (size_t)h->D * *rows;
}

static int set_parents(pyvb_lds* h, int which, int kind, const double* a0, const double* b0, const double* qb) {
    int rc = parents_gate(h, which, 0);
    if (rc) return rc;
    const char* name = kind == PARENTS_GAMMA ? "Gamma" : "DiagonalGamma";
    if (h->known[1].width) {
        pyvb_set_error("%s precision parents of the columns are not served on a handle with regressors (pyvb_lds_create_regressors, k_known.hip)", name);
        return PYVB_E_UNSUPPORTED;
    }
    if (h->known[0].width) {
        pyvb_set_error("%s precision parents of the columns are not served on a handle with inputs (pyvb_lds_create_inputs, k_known.hip)", name);
        return PYVB_E_UNSUPPORTED;
    }
    if (h->dense) {
        pyvb_set_error("%s precision parents of the columns are served with DiagonalGamma and Gamma noise only, not with Wishart noise (k_wishart.hip)", name);
        return PYVB_E_UNSUPPORTED;
    }
    if (h->big) {
        pyvb_set_error("%s precision parents of the columns are served for max(D, K) <= 64 only, not in the 128-wide class (k_big.hip): D = %d, K = %d", name, h->D, h->K);
        return PYVB_E_UNSUPPORTED;
    }
    ARGCHK(a0 && b0 && qb, "a0, b0 and qb are required");
    size_t rows;
    const size_t N = h->N, per = parents_per(h, which, kind, &rows);
    const ParentWords w = lds_words(which);
    std::vector<double> head, rowsqb;
    if ((rc = check_positive(a0, per, rows, "a0", w)) || (rc = check_positive(b0, per, rows, "b0", w)) ||
        (rc = broadcast_qb(h->rep, qb, per, rows, w, rowsqb))) return rc;
    if (kind == PARENTS_GAMMA) stage_gamma(head, a0, b0, per, which == 0 ? h->D : h->K);
    else stage_diagonal_gamma(head, a0, b0, per);
    ENTER(h);
    ColumnParents& p = h->parents[which];
    const LdsParentBlock o = lds_parent_block(kind, N, h->D, per);
    if (!p.block[kind] && (rc = h->mem.zeros(&p.block[kind], o.total))) return rc;
    if ((rc = h2d(h, p.block[kind], head.data(), o.head)) || (rc = h2d(h, p.block[kind] + o.qb, rowsqb.data(), N * per))) return rc;
    p.begin(kind);          // one kind of parent per matrix: the most recent setter's, unless its launch fails
    // qa / qb and the per-column sums of every row, from qb as given
    if ((rc = p.commit(launch_parents(h, kind, which, true)))) return rc;
    HIPCHK(hipStreamSynchronize(h->stream));               // the staging vectors are about to go out of scope
    // (nothing on the host depends on the column priors: gains, statistics and residuals read the columns, not their parents)
    return PYVB_OK;
}

static int get_parents(pyvb_lds* h, int which, int kind, double* qa, double* qb) {
    int rc = parents_gate(h, which, kind);
    if (rc) return rc;
    ENTER(h);
    size_t rows;
    const size_t N = h->N, per = parents_per(h, which, kind, &rows);
    const double* blk = h->parents[which].current();
    std::vector<double> a(qa ? per : 0);
    if (qa && (rc = d2h(h, a.data(), blk + 2 * per, per))) return rc;
    if ((rc = d2h(h, qb, blk + lds_parent_block(kind, N, h->D, per).qb, N * per))) return rc;
    if ((rc = pyvb_lds_sync(h))) return rc;
    for (size_t n = 0; qa && n < N; ++n) memcpy(qa + n * per, a.data(), per * sizeof(double));
    return PYVB_OK;
}

static int update_parents(pyvb_lds* h, int which, int kind) {
    int rc = parents_gate(h, which, kind);
    if (rc) return rc;
    ENTER(h);
    return flow(h).update_parents(which, kind);
}

int pyvb_lds_set_column_precisions(pyvb_lds* h, int which, const double* a0, const double* b0, const double* qb) {
    return set_parents(h, which, PARENTS_GAMMA, a0, b0, qb);
}
int pyvb_lds_get_column_precisions(pyvb_lds* h, int which, double* qa, double* qb) { return get_parents(h, which, PARENTS_GAMMA, qa, qb); }
int pyvb_lds_update_column_precisions(pyvb_lds* h, int which) { return update_parents(h, which, PARENTS_GAMMA); }
int pyvb_lds_set_entry_precisions(pyvb_lds* h, int which, const double* a0, const double* b0, const double* qb) {
    return set_parents(h, which, PARENTS_DIAGONAL_GAMMA, a0, b0, qb);
}
int pyvb_lds_get_entry_precisions(pyvb_lds* h, int which, double* qa, double* qb) { return get_parents(h, which, PARENTS_DIAGONAL_GAMMA, qa, qb); }
int pyvb_lds_update_entry_precisions(pyvb_lds* h, int which) { return update_parents(h, which, PARENTS_DIAGONAL_GAMMA); }

int pyvb_lds_get_column_parents(pyvb_lds* h, int kind[2]) {
    ARGCHK(h, "handle is NULL");
    ARGCHK(kind, "kind is NULL");
    kind[0] = h->parents[0].kind; kind[1] = h->parents[1].kind;
    return PYVB_OK;
}

int pyvb_lds_set_wishart_priors(pyvb_lds* h, double Q_v0, const double* Q_w0, double R_v0, const double* R_w0) {
    ENTER(h);
    ARGCHK(h->dense, "the handle was not created with PYVB_NOISE_WISHART");
    ARGCHK(Q_w0 && R_w0, "Q_w0 and R_w0 are required");
    const int D = h->D, K = h->K, T = h->T, N = h->N;
    if (host_lndet(Q_w0, D, &h->pri.Q_w0_lndet) != PYVB_OK || host_lndet(R_w0, K, &h->pri.R_w0_lndet) != PYVB_OK) {
        pyvb_set_error("a Wishart prior w0 is not symmetric positive definite");
        return PYVB_E_LINALG;
    }
    h->pri.Q_a0_host = Q_v0; h->pri.R_a0_host = R_v0;
    int rc;
    if ((rc = h2d(h, h->pri.Q_w0, Q_w0, (size_t)D * D))) return rc;
    if ((rc = h2d(h, h->pri.R_w0, R_w0, (size_t)K * K))) return rc;
    // qv is fixed by the graph: update_v, nodes_todo.py:224-227 (+0.5 per child); Q has T-1 children, R has T
    std::vector<double> qa((size_t)N * D, Q_v0 + 0.5 * (T - 1)), ra((size_t)N * K, R_v0 + 0.5 * T);
    if ((rc = h2d(h, h->Q_a, qa.data(), qa.size()))) return rc;
    if ((rc = h2d(h, h->R_a, ra.data(), ra.size()))) return rc;
    HIPCHK(hipStreamSynchronize(h->stream));
    h->st.noise_changed();
    h->st.parameters_changed();
    return PYVB_OK;
}

int pyvb_lds_set_wishart_state(pyvb_lds* h, const double* Q_w, const double* R_w) {
    ENTER(h);
    ARGCHK(h->dense, "the handle was not created with PYVB_NOISE_WISHART");
    int rc;
    if ((rc = h2d(h, h->Q_w, Q_w, (size_t)h->N * h->D * h->D))) return rc;
    if ((rc = h2d(h, h->R_w, R_w, (size_t)h->N * h->K * h->K))) return rc;
    HIPCHK(hipStreamSynchronize(h->stream));
    h->st.noise_changed();
    return PYVB_OK;
}

int pyvb_lds_get_wishart_state(pyvb_lds* h, double* Q_v, double* Q_w, double* R_v, double* R_w) {
    ENTER(h);
    ARGCHK(h->dense, "the handle was not created with PYVB_NOISE_WISHART");
    const size_t N = h->N, D = h->D, K = h->K;
    int rc;
    std::vector<double> qa(Q_v ? N * D : 0), ra(R_v ? N * K : 0);       // qv is stored once per dimension, like the Gamma kinds' qa
    if (Q_v && (rc = d2h(h, qa.data(), h->Q_a, N * D))) return rc;
    if (R_v && (rc = d2h(h, ra.data(), h->R_a, N * K))) return rc;
    if ((rc = d2h(h, Q_w, h->Q_w, N * D * D))) return rc;
    if ((rc = d2h(h, R_w, h->R_w, N * K * K))) return rc;
    if ((rc = pyvb_lds_sync(h))) return rc;
    for (size_t n = 0; Q_v && n < N; ++n) Q_v[n] = qa[n * D];
    for (size_t n = 0; R_v && n < N; ++n) R_v[n] = ra[n * K];
    return PYVB_OK;
}

// dense [N][D][rows][rows] on the host <-> the tiled device storage, through a device staging buffer of at most 64 MB
static int column_cov_io(pyvb_lds* h, int which, double* host, bool to_device) {
    if (!host) return PYVB_OK;
    const size_t D = h->D, rows = which == 0 ? h->D : h->K, per = D * rows * rows;
    size_t slice = ((size_t)8 << 20) / per;                 // replicates per slice
    if (slice < 1) slice = 1;
    if (slice > (size_t)h->N) slice = h->N;
    double* stage = nullptr;
    HIPCHK(hipMalloc((void**)&stage, slice * per * sizeof(double)));
    int rc = PYVB_OK;
    for (size_t n0 = 0; n0 < (size_t)h->N && rc == PYVB_OK; n0 += slice) {
        const size_t cnt = (n0 + slice <= (size_t)h->N) ? slice : (size_t)h->N - n0;
        hipError_t e = hipSuccess;
        if (to_device) {
            e = hipMemcpyAsync(stage, host + n0 * per, cnt * per * sizeof(double), hipMemcpyHostToDevice, h->stream);
            if (e == hipSuccess) rc = launch_cov_convert(h, which, stage, (int)n0, (int)cnt, 1);
        } else {
            rc = launch_cov_convert(h, which, stage, (int)n0, (int)cnt, 0);
            if (rc == PYVB_OK) e = hipMemcpyAsync(host + n0 * per, stage, cnt * per * sizeof(double), hipMemcpyDeviceToHost, h->stream);
        }
        if (e == hipSuccess) e = hipStreamSynchronize(h->stream);       // the staging buffer is reused by the next slice
        if (e != hipSuccess && rc == PYVB_OK) rc = pyvb_hip_fail(e, "column covariance transfer", __FILE__, __LINE__);
    }
    (void)hipFree(stage);
    return rc;
}

int pyvb_lds_set_column_cov(pyvb_lds* h, const double* A_cov, const double* C_cov) {
    ENTER(h);
    ARGCHK(h->dense, "dense column covariances exist with PYVB_NOISE_WISHART only");
    int rc;
    if ((rc = column_cov_io(h, 0, const_cast<double*>(A_cov), true))) return rc;
    if ((rc = column_cov_io(h, 1, const_cast<double*>(C_cov), true))) return rc;
    if ((A_cov || C_cov) && (rc = launch_cov_to_colvar(h))) return rc;      // the diagonals (what the lower bound reads) follow
    HIPCHK(hipStreamSynchronize(h->stream));
    h->st.columns_changed();
    return PYVB_OK;
}

int pyvb_lds_get_column_cov(pyvb_lds* h, double* A_cov, double* C_cov) {
    ENTER(h);
    ARGCHK(h->dense, "dense column covariances exist with PYVB_NOISE_WISHART only");
    int rc;
    if ((rc = column_cov_io(h, 0, A_cov, false))) return rc;
    if ((rc = column_cov_io(h, 1, C_cov, false))) return rc;
    return pyvb_lds_sync(h);
}

int pyvb_lds_set_column_observations(pyvb_lds* h, const double* A_obs, const double* C_obs) {
    ENTER(h);
    if (h->known[0].width || h->known[1].width) {
        bool known = false;
        for (size_t i = 0; A_obs && i < (size_t)h->D * h->D && !known; ++i) known = A_obs[i] == A_obs[i];
        for (size_t i = 0; C_obs && i < (size_t)h->K * h->D && !known; ++i) known = C_obs[i] == C_obs[i];
        if (known && h->known[1].width) {
            pyvb_set_error("known entries of A / C are not served on a handle with regressors (pyvb_lds_create_regressors, k_known.hip)");
            return PYVB_E_UNSUPPORTED;
        }
        if (known) {
            pyvb_set_error("known entries of A / C are not served on a handle with inputs (pyvb_lds_create_inputs, k_known.hip)");
            return PYVB_E_UNSUPPORTED;
        }
    }
    if (h->dense && h->big) {
        pyvb_set_error("with Wishart noise, known entries of A / C are served for D, K <= 64 only (k_wishart_big.hip)");
        return PYVB_E_UNSUPPORTED;
    }
    int rc;
    if ((rc = h2d(h, h->pri.A_obs, A_obs, (size_t)h->D * h->D))) return rc;
    if ((rc = h2d(h, h->pri.C_obs, C_obs, (size_t)h->K * h->D))) return rc;
    if ((rc = launch_observe(h))) return rc;
    if (h->dense && (rc = launch_cov_observe(h))) return rc;
    HIPCHK(hipStreamSynchronize(h->stream));
    h->st.columns_changed();
    return PYVB_OK;
}

int pyvb_lds_set_observations(pyvb_lds* h, const double* Y) {
    ENTER(h);
    ARGCHK(Y, "Y is NULL");
    const size_t n = (size_t)h->N * h->T * h->K;
    bool missing = false;
    if (h->rep.ragged()) {      // padding rows may hold anything, NaN included: they are not outputs of any graph
        for (int r = 0; r < h->N; ++r) {
            const double* Yr = Y + (size_t)r * h->T * h->K;
            for (size_t i = 0; i < (size_t)h->rep.length(r) * h->K; ++i)
                if (Yr[i] != Yr[i]) {
                    if (h->known[1].width) { missing = true; break; }       // (refused below, naming the regressors)
                    pyvb_set_error("outputs that hold NaN are not served together with chains of unequal length (k_missing.hip): "
                                   "replicate %d, t = %d of its %d nodes", r, (int)(i / h->K), h->rep.length(r));
                    return PYVB_E_UNSUPPORTED;
                }
        }
    } else
        for (size_t i = 0; i < n && !missing; ++i) missing = Y[i] != Y[i];
    int rc;
    if (missing && h->known[1].width) {
        pyvb_set_error("outputs that hold NaN are not served on a handle with regressors (pyvb_lds_create_regressors, k_missing.hip): "
                       "sum_t y_t v_t^T and the imputation would both change");
        return PYVB_E_UNSUPPORTED;
    }
    if (missing && h->known[0].width) {
        pyvb_set_error("outputs that hold NaN are not served on a handle with inputs (pyvb_lds_create_inputs, k_missing.hip)");
        return PYVB_E_UNSUPPORTED;
    }
    if (missing && h->dense && h->big) {
        pyvb_set_error("with Wishart noise, outputs that hold NaN are served for D, K <= 64 only (k_wishart_big.hip)");
        return PYVB_E_UNSUPPORTED;
    }
    if (missing) {
        if (!h->Yobs) {
            if ((rc = h->mem.zeros(&h->Yobs, n))) return rc;
            if ((rc = h->mem.zeros(&h->Yvar, n))) return rc;
            if ((rc = h->mem.zeros(&h->Yqld, (size_t)h->N * h->T))) return rc;
            if ((rc = h->mem.zeros(&h->Yent, h->N))) return rc;
            if ((rc = h->mem.zeros(&h->Ylnd, (size_t)h->N * h->T))) return rc;
            if ((rc = h->mem.zeros(&h->YentX, h->N))) return rc;
            if (h->dense) {
                if ((rc = h->mem.zeros(&h->Yld, (size_t)h->N * h->T))) return rc;
                if ((rc = h->mem.zeros(&h->YcovS, (size_t)h->N * h->K * h->K))) return rc;
            }
        }
        if ((rc = h2d(h, h->Yobs, Y, n))) return rc;
        h->has_missing = true;
        // rows with NaN start as N(0, I) until pyvb_lds_set_output_state says otherwise
        if ((rc = launch_missing_init(h, nullptr, nullptr))) return rc;
        if ((rc = h->dense ? flow(h).outputs_changed_dense(1) : flow(h).syy_missing())) return rc;
    } else {
        h->has_missing = false;
        if ((rc = h2d(h, h->Y, Y, n))) return rc;
        if ((rc = flow(h).syy())) return rc;
        if ((h->known[0].width || h->known[1].width) && (rc = launch_known_assemble(h))) return rc;      // the rows [y_t ; u_t ; u_{t+1} ; v_t] the sweeps read
        if (h->known[1].width && (rc = launch_known_gram(h, 1))) return rc;      // Syv
        if (h->dense && (rc = launch_syy_full(h))) return rc;
    }
    HIPCHK(hipStreamSynchronize(h->stream));
    h->st.outputs_changed();
    return PYVB_OK;
}

int pyvb_lds_set_output_state(pyvb_lds* h, const double* Yq, const double* Yrowvar) {
    ENTER(h);
    ARGCHK(h->has_missing, "the observations hold no NaN: every output is observed");
    ARGCHK(Yq && Yrowvar, "Yq and Yrowvar are required");
    const size_t n = (size_t)h->N * h->T * h->K;
    { int rc0 = settle_parked(h); if (rc0) return rc0; }
    // staged through buffers that are free until the next sweep / statistics pass
    double* dq = h->U;                  // [N][T][DP] >= [N][T][K]?  not for K > DP: use a temporary then
    double* tmp = nullptr;
    if ((size_t)h->K > (size_t)h->L.DP) { HIPCHK(hipMalloc((void**)&tmp, n * sizeof(double))); dq = tmp; }
    double* dv = h->X[1 - h->st.cur];      // [N][T][DP] >= [N][T]
    int rc;
    if ((rc = h2d(h, dq, Yq, n)) || (rc = h2d(h, dv, Yrowvar, (size_t)h->N * h->T)) ||
        (rc = launch_missing_init(h, dq, dv)) || (rc = h->dense ? flow(h).outputs_changed_dense(1) : flow(h).syy_missing())) {
        if (tmp) { (void)hipStreamSynchronize(h->stream); (void)hipFree(tmp); }
        return rc;
    }
    const hipError_t se = hipStreamSynchronize(h->stream);
    if (tmp) (void)hipFree(tmp);
    HIPCHK(se);
    h->st.outputs_changed();
    return PYVB_OK;
}

int pyvb_lds_get_outputs(pyvb_lds* h, double* Yq, double* Yvar, double* Yqld) {
    ENTER(h);
    const size_t n = (size_t)h->N * h->T * h->K;
    int rc;
    if ((rc = d2h(h, Yq, h->Y, n))) return rc;
    if (Yvar) {
        if (h->has_missing) { if ((rc = d2h(h, Yvar, h->Yvar, n))) return rc; }
        else memset(Yvar, 0, n * sizeof(double));
    }
    if (Yqld) {
        if (h->has_missing) { if ((rc = d2h(h, Yqld, h->Yqld, (size_t)h->N * h->T))) return rc; }
        else for (size_t i = 0; i < (size_t)h->N * h->T; ++i) Yqld[i] = NAN;
    }
    if ((rc = pyvb_lds_sync(h))) return rc;
    fill_padding(h, Yq, h->K, 0.0);
    return PYVB_OK;
}

int pyvb_lds_update_Y(pyvb_lds* h) {
    ENTER(h);
    return flow(h).update_Y();
}

// ---- Known channels: an input that drives the states (side 0, pyvb_lds_create_inputs) and regressors in the output equation
// (side 1, pyvb_lds_create_regressors); KnownChannels of common.h, the kernels are k_known.hip.  One copy of every entry, with
// the side's words in the messages.
static const struct { const char *what, *chan, *gain; } known_words[2] = {{"inputs", "U", "B"}, {"regressors", "V", "E"}};

static int known_gate(const pyvb_lds* h, int side) {
    ARGCHK(h, "handle is NULL");
    if (h->known[side].width <= 0) {
        pyvb_set_error("the handle was created without %s (pyvb_lds_create_%s makes one with)", known_words[side].what, known_words[side].what);
        return PYVB_E_ARG;
    }
    return PYVB_OK;
}

static int known_set_channels(pyvb_lds* h, int side, const double* U) {
    int rc = known_gate(h, side);
    if (rc) return rc;
    const char* name = known_words[side].chan;
    if (!U) { pyvb_set_error("%s is NULL", name); return PYVB_E_ARG; }
    KnownChannels& k = h->known[side];
    const size_t T = h->T, P = k.width;
    for (int n = 0; n < h->N; ++n)
        for (size_t i = 0; i < T * P; ++i)
            if (!std::isfinite(U[(size_t)n * T * P + i])) {
                pyvb_set_error("%s is not finite: replicate %d, row %d, channel %d", name, n, (int)(i / P), (int)(i % P));
                return PYVB_E_ARG;
            }
    ENTER(h);
    if ((rc = h2d(h, k.in, U, (size_t)h->N * T * P))) return rc;
    if ((rc = launch_known_assemble(h)) || (rc = launch_known_gram(h, side))) return rc;
    HIPCHK(hipStreamSynchronize(h->stream));
    k.set = true;
    h->st.outputs_changed();        // what the sweeps read as outputs has changed: c_t and every sum over t with it
    return PYVB_OK;
}

static int known_get_channels(pyvb_lds* h, int side, double* U) {
    int rc = known_gate(h, side);
    if (rc) return rc;
    if (!U) { pyvb_set_error("%s is NULL", known_words[side].chan); return PYVB_E_ARG; }
    ENTER(h);
    if ((rc = d2h(h, U, h->known[side].in, (size_t)h->N * h->T * h->known[side].width))) return rc;
    return pyvb_lds_sync(h);
}

static int known_set_priors(pyvb_lds* h, int side, const double* pm, const double* pp) {
    int rc = known_gate(h, side);
    if (rc) return rc;
    const char* g = known_words[side].gain;
    if (!(pm && pp)) { pyvb_set_error("%s_prior_mean and %s_prior_prec are required", g, g); return PYVB_E_ARG; }
    KnownChannels& k = h->known[side];
    const int D = lds_known_rows(h, side), P = k.width;
    for (int i = 0; i < P * D; ++i)
        if (!(pp[i] > 0.0 && std::isfinite(pp[i]) && std::isfinite(pm[i]))) {
            pyvb_set_error("%s_prior_prec must be positive and %s_prior_mean finite", g, g);
            return PYVB_E_ARG;
        }
    std::vector<double> ld((size_t)P, 0.0);     // ln det of the diagonal prior precision of every column (node.py:301-302)
    for (int i = 0; i < P; ++i)
        for (int r = 0; r < D; ++r) ld[i] += log(pp[(size_t)i * D + r]);
    ENTER(h);
    if ((rc = h2d(h, k.pm, pm, (size_t)D * P)) || (rc = h2d(h, k.pp, pp, (size_t)P * D)) || (rc = h2d(h, k.pld, ld.data(), P))) return rc;
    HIPCHK(hipStreamSynchronize(h->stream));    // ld is about to go out of scope
    k.priors_set = true;
    h->st.parameters_changed();
    return PYVB_OK;
}

static int known_set_state(pyvb_lds* h, int side, const double* mean, const double* colvar) {
    int rc = known_gate(h, side);
    if (rc) return rc;
    ENTER(h);
    const size_t n = (size_t)h->N * lds_known_rows(h, side) * h->known[side].width;
    if ((rc = h2d(h, h->known[side].mean, mean, n)) || (rc = h2d(h, h->known[side].var, colvar, n))) return rc;
    HIPCHK(hipStreamSynchronize(h->stream));
    if (mean || colvar) h->st.parameters_changed();
    return PYVB_OK;
}

static int known_get_state(pyvb_lds* h, int side, double* mean, double* colvar, double* qld, double* lnd) {
    int rc = known_gate(h, side);
    if (rc) return rc;
    ENTER(h);
    const KnownChannels& k = h->known[side];
    const size_t N = h->N, D = lds_known_rows(h, side), P = k.width;
    if ((rc = d2h(h, mean, k.mean, N * D * P)) || (rc = d2h(h, colvar, k.var, N * P * D)) ||
        (rc = d2h(h, qld, k.qld, N * P)) || (rc = d2h(h, lnd, k.lnd, N * P))) return rc;
    return pyvb_lds_sync(h);
}

static int known_update_gain(pyvb_lds* h, int side) {
    int rc = known_gate(h, side);
    if (rc) return rc;
    ENTER(h);
    return flow(h).update_gain(side);
}

int pyvb_lds_set_inputs(pyvb_lds* h, const double* U) { return known_set_channels(h, 0, U); }
int pyvb_lds_get_inputs(pyvb_lds* h, double* U) { return known_get_channels(h, 0, U); }
int pyvb_lds_set_input_priors(pyvb_lds* h, const double* B_pm, const double* B_pp) { return known_set_priors(h, 0, B_pm, B_pp); }
int pyvb_lds_set_input_state(pyvb_lds* h, const double* B_mean, const double* B_colvar) { return known_set_state(h, 0, B_mean, B_colvar); }
int pyvb_lds_get_input_state(pyvb_lds* h, double* B_mean, double* B_colvar, double* qld_B, double* lnd_B) { return known_get_state(h, 0, B_mean, B_colvar, qld_B, lnd_B); }
int pyvb_lds_update_B(pyvb_lds* h) { return known_update_gain(h, 0); }
int pyvb_lds_set_regressors(pyvb_lds* h, const double* V) { return known_set_channels(h, 1, V); }
int pyvb_lds_get_regressors(pyvb_lds* h, double* V) { return known_get_channels(h, 1, V); }
int pyvb_lds_set_regressor_priors(pyvb_lds* h, const double* E_pm, const double* E_pp) { return known_set_priors(h, 1, E_pm, E_pp); }
int pyvb_lds_set_regressor_state(pyvb_lds* h, const double* E_mean, const double* E_colvar) { return known_set_state(h, 1, E_mean, E_colvar); }
int pyvb_lds_get_regressor_state(pyvb_lds* h, double* E_mean, double* E_colvar, double* qld_E, double* lnd_E) { return known_get_state(h, 1, E_mean, E_colvar, qld_E, lnd_E); }
int pyvb_lds_update_E(pyvb_lds* h) { return known_update_gain(h, 1); }

int pyvb_lds_set_state(pyvb_lds* h, const double* X, const double* A_mean, const double* A_colvar,
                       const double* C_mean, const double* C_colvar, const double* Q_b, const double* R_b) {
    ENTER(h);
    const size_t N = h->N, T = h->T, D = h->D, K = h->K;
    int rc;
    if ((rc = settle_parked(h))) return rc;
    if (X) {    // the other buffer is free between sweeps: stage the API layout there, then permute
        if ((rc = h2d(h, h->X[1 - h->st.cur], X, N * T * D))) return rc;
        if ((rc = launch_permute(h, h->X[1 - h->st.cur], h->X[h->st.cur], 1))) return rc;
    }
    // Chains that share A, C, Q, R: the row of a model's first replicate is the model's state and goes to all its rows
    std::vector<double> tied[6];        // (staging; alive until the synchronisation below)
    auto model_rows = [&](int slot, const double* src, size_t per) -> const double* {
        if (!src || !h->rep.tied()) return src;
        std::vector<double>& v = tied[slot];
        v.resize(N * per);
        for (size_t n = 0; n < N; ++n) memcpy(v.data() + n * per, src + (size_t)h->rep.first_of((int)n) * per, per * sizeof(double));
        return v.data();
    };
    if ((rc = h2d(h, h->A_mean, model_rows(0, A_mean, D * D), N * D * D))) return rc;
    if ((rc = h2d(h, h->A_var, model_rows(1, A_colvar, D * D), N * D * D))) return rc;
    if ((rc = h2d(h, h->C_mean, model_rows(2, C_mean, K * D), N * K * D))) return rc;
    if ((rc = h2d(h, h->C_var, model_rows(3, C_colvar, D * K), N * D * K))) return rc;
    if ((rc = h2d(h, h->Q_b, model_rows(4, Q_b, D), N * D))) return rc;
    if ((rc = h2d(h, h->R_b, model_rows(5, R_b, K), N * K))) return rc;
    const bool covs = h->dense && (A_colvar || C_colvar);       // diagonal initial covariances
    if (covs && (rc = launch_colvar_to_cov(h))) return rc;
    HIPCHK(hipStreamSynchronize(h->stream));
    flow(h).state_given(X, covs, A_mean || A_colvar || C_mean || C_colvar || Q_b || R_b);
    return PYVB_OK;
}

int pyvb_lds_get_state(pyvb_lds* h, double* X, double* A_mean, double* A_colvar, double* C_mean, double* C_colvar,
                       double* Q_a, double* Q_b, double* R_a, double* R_b) {
    ENTER(h);
    const size_t N = h->N, T = h->T, D = h->D, K = h->K;
    int rc;
    if ((rc = settle_parked(h))) return rc;
    if (X) {
        if ((rc = launch_permute(h, h->X[h->st.cur], h->X[1 - h->st.cur], 0))) return rc;
        if ((rc = d2h(h, X, h->X[1 - h->st.cur], N * T * D))) return rc;
    }
    if ((rc = d2h(h, A_mean, h->A_mean, N * D * D))) return rc;
    if ((rc = d2h(h, A_colvar, h->A_var, N * D * D))) return rc;
    if ((rc = d2h(h, C_mean, h->C_mean, N * K * D))) return rc;
    if ((rc = d2h(h, C_colvar, h->C_var, N * D * K))) return rc;
    if ((rc = d2h(h, Q_a, h->Q_a, N * D))) return rc;
    if ((rc = d2h(h, Q_b, h->Q_b, N * D))) return rc;
    if ((rc = d2h(h, R_a, h->R_a, N * K))) return rc;
    if ((rc = d2h(h, R_b, h->R_b, N * K))) return rc;
    if ((rc = pyvb_lds_sync(h))) return rc;
    fill_padding(h, X, D, 0.0);
    return PYVB_OK;
}

int pyvb_lds_get_posterior_classes(pyvb_lds* h, double* Sigma, double* qld_x) {
    ENTER(h);
    const size_t N = h->N, D = h->D;
    int rc;
    if ((rc = settle_parked(h))) return rc;
    if ((rc = d2h(h, Sigma, h->Sigma, N * 3 * D * D))) return rc;
    if ((rc = d2h(h, qld_x, h->qld_x, N * 3))) return rc;
    return pyvb_lds_sync(h);
}

int pyvb_lds_set_posterior_classes(pyvb_lds* h, const double* Sigma, const double* qld_x) {
    ENTER(h);
    ARGCHK(Sigma, "Sigma is NULL");
    const size_t N = h->N, D = h->D;
    int rc;
    if ((rc = settle_parked(h))) return rc;
    if ((rc = h2d(h, h->Sigma, Sigma, N * 3 * D * D))) return rc;
    if ((rc = h2d(h, h->qld_x, qld_x, N * 3))) return rc;
    HIPCHK(hipStreamSynchronize(h->stream));
    h->st.classes_set();
    return PYVB_OK;
}

int pyvb_lds_get_column_qld(pyvb_lds* h, double* qld_A, double* qld_C) {
    ENTER(h);
    int rc;
    if ((rc = d2h(h, qld_A, h->qld_A, (size_t)h->N * h->D))) return rc;
    if ((rc = d2h(h, qld_C, h->qld_C, (size_t)h->N * h->D))) return rc;
    return pyvb_lds_sync(h);
}

int pyvb_lds_get_lengths(pyvb_lds* h, int* lengths) {
    ARGCHK(h, "handle is NULL");
    ARGCHK(lengths, "lengths is NULL");
    for (int n = 0; n < h->N; ++n) lengths[n] = h->rep.length(n);
    return PYVB_OK;
}

int pyvb_lds_get_time_split(pyvb_lds* h, int* W) {
    ENTER(h);
    ARGCHK(W, "W is NULL");
    *W = h->W;
    return PYVB_OK;
}

int pyvb_lds_set_time_split(pyvb_lds* h, int W) {
    ENTER(h);
    int rc = check_time_split(h->T, W);
    if (rc) return rc;
    HIPCHK(hipStreamSynchronize(h->stream));
    if (W != h->W) {
        const LdsGeometry g = lds_geometry(h->N, h->T, h->D, lds_sweep_K(h), h->noise).with_time_split(W);
        double* p = nullptr;
        rc = h->mem.zeros(&p, g.sxx);
        if (rc) { h->mem.release(p); return rc; }
        if (g.U2 && !h->U2 && (rc = h->mem.zeros(&h->U2, g.U2))) { h->mem.release(p); return rc; }
        if (h->big) {       // (elsewhere trash does not depend on W)
            double* tr = nullptr;
            if ((rc = h->mem.zeros(&tr, g.trash))) { h->mem.release(tr); h->mem.release(p); return rc; }
            h->mem.release(h->trash);
            h->trash = tr;
        }
        h->mem.release(h->sxx);
        h->sxx = p; h->W = W;
        h->st.x_changed();
    }
    return PYVB_OK;
}

int pyvb_lds_get_warmup(pyvb_lds* h, int* warm) {
    ENTER(h);
    ARGCHK(warm, "warm is NULL");
    HIPCHK(hipMemcpyAsync(warm, h->warm, (size_t)h->N * 2 * sizeof(int), hipMemcpyDeviceToHost, h->stream));
    return pyvb_lds_sync(h);
}

// ln det of every class of Sigma (Cholesky on the host, NaN where one is not positive definite) into lnd_x: what
// LdsFlow::ensure_lnd_x has carried out when Sigma came from the caller
static int form_lnd_x(pyvb_lds* h) {
    const size_t N = h->N, D = h->D;
    std::vector<double> S(N * 3 * D * D), lnd(N * 3), L(D * D);
    HIPCHK(hipMemcpyAsync(S.data(), h->Sigma, S.size() * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    for (size_t m = 0; m < N * 3; ++m) {
        const double* Sm = S.data() + m * D * D;
        double s = 0.0;
        for (size_t j = 0; j < D && s == s; ++j) {
            for (size_t i = j; i < D; ++i) {
                double v = Sm[i * D + j];
                for (size_t k = 0; k < j; ++k) v -= L[i * D + k] * L[j * D + k];
                if (i == j) {
                    if (!(v > 0.0)) { s = NAN; break; }
                    L[j * D + j] = sqrt(v);
                    s += log(v);
                } else L[i * D + j] = v / L[j * D + j];
            }
        }
        lnd[m] = s;
    }
    HIPCHK(hipMemcpyAsync(h->lnd_x, lnd.data(), lnd.size() * sizeof(double), hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    return PYVB_OK;
}

int pyvb_lds_sweep(pyvb_lds* h, int direction) {
    ENTER(h);
    ARGCHK(direction == PYVB_FORWARD || direction == PYVB_BACKWARD, "direction must be PYVB_FORWARD or PYVB_BACKWARD");
    return flow(h).update_sweep(direction);
}

int pyvb_lds_update_x(pyvb_lds* h, int t) {
    ENTER(h);
    ARGCHK(t >= 0 && t < h->T, "t out of range");
    return flow(h).update_x(t);
}

int pyvb_lds_update_columns(pyvb_lds* h, int which, int col_begin, int col_end) {
    ENTER(h);
    ARGCHK(which == 0 || which == 1, "which must be 0 (A) or 1 (C)");
    ARGCHK(col_begin >= 0 && col_begin < col_end && col_end <= h->D, "bad column range");
    return flow(h).update_columns(which, col_begin, col_end);
}

int pyvb_lds_update_A(pyvb_lds* h) { ARGCHK(h, "handle is NULL"); return pyvb_lds_update_columns(h, 0, 0, h->D); }
int pyvb_lds_update_C(pyvb_lds* h) { ARGCHK(h, "handle is NULL"); return pyvb_lds_update_columns(h, 1, 0, h->D); }

int pyvb_lds_update_Q(pyvb_lds* h) { ENTER(h); return flow(h).update_noise(0); }
int pyvb_lds_update_R(pyvb_lds* h) { ENTER(h); return flow(h).update_noise(1); }

int pyvb_lds_elbo(pyvb_lds* h) {
    ENTER(h);
    return flow(h).elbo();
}

int pyvb_lds_get_elbo(pyvb_lds* h, double* parts) {
    ENTER(h);
    ARGCHK(parts, "parts is NULL");
    int rc = d2h(h, parts, h->elbo, (size_t)h->N * 6);
    if (rc) return rc;
    return pyvb_lds_sync(h);
}

// The main stream may not overwrite what a lower-bound evaluation still in flight on the side stream reads
// (the states: next backward sweep; the parameters: next column update).
static int join_elbo(pyvb_lds* h) {
    if (h->elbo_in_flight) {
        HIPCHK(hipStreamWaitEvent(h->stream, h->ev_elbo, 0));
        h->elbo_in_flight = false;
    }
    return PYVB_OK;
}

int pyvb_lds_iterate(pyvb_lds* h, int niters) {
    ENTER_DEVICE(h);
    ARGCHK(niters >= 0, "niters must be >= 0");
    int rc;
    // Every replicate switched off: no update is launched, but the (empty) sums still go into the history and through the
    // all-reduce, which the other ranks are waiting in.
    LdsFlow<LdsDevice> f = flow(h);
    const bool idle = f.idle();
    for (int it = 0; it < niters; ++it) {
        if ((rc = idle ? join_elbo(h) : f.iterate_updates())) return rc;
        // The lower bound (network.py:49) feeds nothing in the next iteration: it is evaluated on the side stream while
        // the main one goes on with k_prep and the forward sweep.  Its per-iteration totals (summed over the replicates,
        // and over the ranks when a communicator is attached) go into a history ring (pyvb_lds_get_elbo_history).
        HIPCHK(hipEventRecord(h->ev_params, h->stream));
        HIPCHK(hipStreamWaitEvent(h->side, h->ev_params, 0));
        if (!idle && (rc = h->dense ? launch_elbo_dense(h, h->side) : f.lds_bound(h->side))) return rc;
        double* slot = h->elbo_hist + (size_t)(h->hist_count % PYVB_ELBO_HISTORY) * 8;
        if ((rc = launch_elbo_sum(h, slot, h->side))) return rc;
        if (h->comm && (rc = pyvb_allreduce_f64(h->comm, slot, 6, h->side))) return rc;
        h->hist_count += 1;
        HIPCHK(hipEventRecord(h->ev_elbo, h->side));
        h->elbo_in_flight = true;
    }
    // the last lower bound may still be in flight: the next pyvb_lds_iterate overlaps it with its k_prep and forward
    // sweep, any other entry point joins it first (ENTER), pyvb_lds_sync waits for both streams
    return PYVB_OK;
}

// pyvb_lds_iterate with the stopping test of network.py:53 applied by every replicate to itself or, per_model, by
// every model to the bound of its graph (k_converge.hip serves both).  The decision of iteration i must be in force before the k_prep of
// i + 1 reads the mask, so here the bound, the test and the totals run on the main stream, in order, and nothing overlaps the next
// iteration (has what that costs; section 20 the per-model test).
static int iterate_until(pyvb_lds* h, int max_iters, double tol, int check_every, int* iters_run, bool per_model) {
    ARGCHK(h, "handle is NULL");
    ARGCHK(max_iters >= 0, "max_iters must be >= 0");
    ARGCHK(check_every >= 1, "check_every must be >= 1");
    ARGCHK(tol == tol, "tol is NaN");
    ARGCHK(iters_run, "iters_run is NULL");
    if (!per_model && h->rep.tied()) {
        pyvb_set_error("pyvb_lds_iterate_until is not served on a handle with a model of more than one chain (pyvb_lds_create_tied): "
                       "the stopping test is per replicate, convergence per model is pyvb_lds_iterate_until_model");
        return PYVB_E_UNSUPPORTED;
    }
    ENTER(h);
    *iters_run = 0;
    int rc, it = 0;
    // Nothing to run on this rank: no update is launched, but with a communicator the totals and the running count (0 here)
    // still go through the all-reduce the other ranks are waiting in, until every rank has stopped.
    LdsFlow<LdsDevice> f = flow(h);
    const bool idle = f.idle();
    bool done = idle && !h->comm;
    while (!done && it < max_iters) {
        if (!idle) {
            if ((rc = f.iterate_updates())) return rc;
            if ((rc = h->dense ? launch_elbo_dense(h, h->stream) : f.lds_bound(h->stream))) return rc;
            if ((rc = launch_converge(h, tol, it == 0, h->stream))) return rc;
        }
        double* slot = h->elbo_hist + (size_t)(h->hist_count % PYVB_ELBO_HISTORY) * 8;
        if ((rc = launch_elbo_sum(h, slot, h->stream))) return rc;
        if (h->comm && (rc = pyvb_allreduce_f64(h->comm, slot, 7, h->stream))) return rc;
        h->hist_count += 1;
        it += 1;
        if (it % check_every == 0 && it < max_iters) {
            // how many replicates (of all ranks) are still running: a small copy to pinned memory and an event, not a spin
            HIPCHK(hipMemcpyAsync(h->running_host, slot + 6, sizeof(double), hipMemcpyDeviceToHost, h->stream));
            HIPCHK(hipEventRecord(h->ev_check, h->stream));
            HIPCHK(hipEventSynchronize(h->ev_check));
            done = *h->running_host == 0.0;
        }
    }
    *iters_run = it;
    HIPCHK(hipStreamSynchronize(h->stream));
    HIPCHK(hipStreamSynchronize(h->side));
    // the host record: which replicates the test has frozen, and with that how many are left for idle(), settle_parked and
    // adopt_classes.  The rows frozen in this call are identical in both X buffers and both class sets, so x_park /
    // cls_parked_other are right for them whatever they say.
    std::vector<unsigned char> conv((size_t)h->N);
    HIPCHK(hipMemcpy(conv.data(), h->conv, conv.size(), hipMemcpyDeviceToHost));
    h->rep.adopt_conv(conv.data());
    return PYVB_OK;
}

int pyvb_lds_iterate_until(pyvb_lds* h, int max_iters, double tol, int check_every, int* iters_run) {
    return iterate_until(h, max_iters, tol, check_every, iters_run, false);
}

int pyvb_lds_iterate_until_model(pyvb_lds* h, int max_iters, double tol, int check_every, int* iters_run) {
    return iterate_until(h, max_iters, tol, check_every, iters_run, true);
}

int pyvb_lds_get_convergence(pyvb_lds* h, int* iters, unsigned char* converged, double* llb) {
    ENTER(h);
    HIPCHK(hipStreamSynchronize(h->stream));
    HIPCHK(hipStreamSynchronize(h->side));
    if (iters) HIPCHK(hipMemcpy(iters, h->conv_iters, (size_t)h->N * sizeof(int), hipMemcpyDeviceToHost));
    if (converged) HIPCHK(hipMemcpy(converged, h->conv, (size_t)h->N, hipMemcpyDeviceToHost));
    if (llb) HIPCHK(hipMemcpy(llb, h->conv_llb, (size_t)h->N * sizeof(double), hipMemcpyDeviceToHost));
    return PYVB_OK;
}

// One entry per model, read from the row of its first replicate: every chain of a model holds the model's values.
int pyvb_lds_get_model_convergence(pyvb_lds* h, int* iters, unsigned char* converged, double* llb) {
    ARGCHK(h, "handle is NULL");
    if (!h->rep.tied()) return pyvb_lds_get_convergence(h, iters, converged, llb);      // M = N
    const size_t N = (size_t)h->N;
    std::vector<int> it(N);
    std::vector<unsigned char> cv(N);
    std::vector<double> lb(N);
    int rc = pyvb_lds_get_convergence(h, it.data(), cv.data(), lb.data());
    if (rc) return rc;
    for (int n = 0; n < h->N; ++n) {
        if (h->rep.first_of(n) != n) continue;
        const int m = h->rep.model(n);
        if (iters) iters[m] = it[n];
        if (converged) converged[m] = cv[n];
        if (llb) llb[m] = lb[n];
    }
    return PYVB_OK;
}

int pyvb_lds_get_elbo_history(pyvb_lds* h, double* out, int max_count, int* count) {
    ENTER(h);
    ARGCHK(out && count && max_count >= 0, "bad arguments");
    int n = h->hist_count < PYVB_ELBO_HISTORY ? h->hist_count : PYVB_ELBO_HISTORY;
    if (n > max_count) n = max_count;
    HIPCHK(hipStreamSynchronize(h->stream));
    HIPCHK(hipStreamSynchronize(h->side));
    std::vector<double> tmp((size_t)n * 8);
    for (int i = 0; i < n; ++i) {            // the most recent n rows, oldest first
        const size_t row = (size_t)((h->hist_count - n + i) % PYVB_ELBO_HISTORY);
        HIPCHK(hipMemcpy(tmp.data() + (size_t)i * 8, h->elbo_hist + row * 8, 6 * sizeof(double), hipMemcpyDeviceToHost));
        for (int p = 0; p < 6; ++p) out[(size_t)i * 6 + p] = tmp[(size_t)i * 8 + p];
    }
    *count = n;
    return pyvb_lds_sync(h);
}

int pyvb_lds_reset_elbo_history(pyvb_lds* h) { ENTER(h); HIPCHK(hipStreamSynchronize(h->side)); h->hist_count = 0; return PYVB_OK; }

int pyvb_lds_set_bound_mode(pyvb_lds* h, int mode) {
    ENTER(h);
    ARGCHK(mode == PYVB_BOUND_REFERENCE || mode == PYVB_BOUND_EXACT, "mode must be PYVB_BOUND_REFERENCE or PYVB_BOUND_EXACT");
    HIPCHK(hipStreamSynchronize(h->side));
    h->bound = mode;
    h->hist_count = 0;              // the history holds bounds of one mode only
    return PYVB_OK;
}

int pyvb_lds_get_logdets(pyvb_lds* h, double* lnd_x, double* lnd_A, double* lnd_C, double* Ylnd) {
    ENTER(h);
    int rc;
    if ((rc = settle_parked(h))) return rc;
    if (lnd_x && (rc = flow(h).ensure_lnd_x())) return rc;
    if ((rc = d2h(h, lnd_x, h->lnd_x, (size_t)h->N * 3))) return rc;
    if ((rc = d2h(h, lnd_A, h->lnd_A, (size_t)h->N * h->D))) return rc;
    if ((rc = d2h(h, lnd_C, h->lnd_C, (size_t)h->N * h->D))) return rc;
    if (Ylnd) {
        if (h->has_missing) { if ((rc = d2h(h, Ylnd, h->Ylnd, (size_t)h->N * h->T))) return rc; }
        else for (size_t i = 0; i < (size_t)h->N * h->T; ++i) Ylnd[i] = NAN;
    }
    return pyvb_lds_sync(h);
}

int pyvb_lds_sync(pyvb_lds* h) {
    ENTER(h);
    HIPCHK(hipStreamSynchronize(h->stream));
    HIPCHK(hipStreamSynchronize(h->side));
    HIPCHK(hipMemcpy(h->status_host.data(), h->status, (size_t)h->N * sizeof(int), hipMemcpyDeviceToHost));
    int first = -1, failed = 0;
    for (int n = 0; n < h->N; ++n)      // the flags of a replicate that was switched off (because it failed) do not raise again
        if (h->status_host[n] && h->rep.active(n)) { if (first < 0) first = n; ++failed; }
    if (failed) {
        h->reported = h->status_host;
        pyvb_set_error("a posterior precision was not positive definite (numpy.linalg.LinAlgError in the reference): "
                       "first in replicate %d, %d of %d replicates failed (pyvb_lds_get_status)", first, failed, h->N);
        HIPCHK(hipMemset(h->status, 0, (size_t)h->N * sizeof(int)));
        return PYVB_E_LINALG;
    }
    h->reported.assign((size_t)h->N, 0);
    return PYVB_OK;
}

int pyvb_lds_get_status(pyvb_lds* h, int* status) {
    ARGCHK(h, "handle is NULL");
    ARGCHK(status, "status is NULL");
    ENTER(h);
    HIPCHK(hipStreamSynchronize(h->stream));
    HIPCHK(hipStreamSynchronize(h->side));
    HIPCHK(hipMemcpy(h->status_host.data(), h->status, (size_t)h->N * sizeof(int), hipMemcpyDeviceToHost));
    for (int n = 0; n < h->N; ++n) status[n] = h->status_host[n] | h->reported[n];
    return PYVB_OK;
}

// The two device masks from the host record: what the totals count is the caller's mask, what the update kernels run is that
// without the converged replicates (the same bytes until pyvb_lds_iterate_until has stopped one).
static int upload_masks(pyvb_lds* h) {
    const std::vector<unsigned char> run = h->rep.run_mask();
    HIPCHK(hipMemcpyAsync(h->counted, h->rep.caller_mask(), (size_t)h->N, hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipMemcpyAsync(h->active, run.data(), (size_t)h->N, hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));       // `run` is about to go out of scope
    return PYVB_OK;
}

int pyvb_lds_set_active(pyvb_lds* h, const unsigned char* active) {
    ARGCHK(h, "handle is NULL");
    ARGCHK(active, "active is NULL");
    int rc = h->rep.check_mask(active);
    if (rc) return rc;
    ENTER(h);
    if (!h->rep.mask_differs(active)) return PYVB_OK;
    // rows switched off earlier move to where the rows switched off now are: the current buffers
    if ((rc = settle_parked(h))) return rc;
    h->rep.adopt_mask(active);
    h->st.parked_here();
    return upload_masks(h);
}

int pyvb_lds_get_active(pyvb_lds* h, unsigned char* active) {
    ARGCHK(h, "handle is NULL");
    ARGCHK(active, "active is NULL");
    memcpy(active, h->rep.caller_mask(), (size_t)h->N);
    return PYVB_OK;
}

int pyvb_lds_timing_enable(pyvb_lds* h, int on) { ENTER(h); h->timing = on != 0; return PYVB_OK; }
int pyvb_lds_timing_reset(pyvb_lds* h) { ENTER(h); pyvb_timing_resolve(h); memset(h->timers, 0, sizeof(h->timers)); return PYVB_OK; }
int pyvb_lds_timing_get(pyvb_lds* h, int kernel, double* total_ms, int* launches) {
    ENTER(h);
    ARGCHK(kernel >= 0 && kernel < PYVB_K_COUNT, "no such kernel id");
    pyvb_timing_resolve(h);
    if (h->timing_errors) { pyvb_set_error("%d timing events could not be recorded or resolved", h->timing_errors); h->timing_errors = 0; return PYVB_E_HIP; }
    if (total_ms) *total_ms = h->timers[kernel].total_ms;
    if (launches) *launches = h->timers[kernel].launches;
    return PYVB_OK;
}

// ---- RCCL (loaded on demand so that single-GPU use does not depend on it) -------------------
typedef struct { char internal[128]; } nccl_uid;
typedef int (*fn_getuid)(nccl_uid*);
typedef int (*fn_initrank)(void**, int, nccl_uid, int);
typedef int (*fn_allreduce)(const void*, void*, size_t, int, int, void*, hipStream_t);
typedef int (*fn_destroy)(void*);
typedef const char* (*fn_errstr)(int);
static struct { void* lib; fn_getuid getuid; fn_initrank initrank; fn_allreduce allreduce; fn_destroy destroy; fn_errstr errstr; } g_nccl;

// The only process-wide state of the library: the dlopen'ed RCCL entry points, set once under a lock.
static std::mutex g_nccl_lock;
static int load_rccl() {
    std::lock_guard<std::mutex> guard(g_nccl_lock);
    if (g_nccl.lib) return PYVB_OK;
    void* lib = dlopen("librccl.so.1", RTLD_NOW | RTLD_LOCAL);
    if (!lib) lib = dlopen("librccl.so", RTLD_NOW | RTLD_LOCAL);
    if (!lib) { pyvb_set_error("cannot load librccl: %s", dlerror()); return PYVB_E_RCCL; }
    g_nccl.getuid = (fn_getuid)dlsym(lib, "ncclGetUniqueId");
    g_nccl.initrank = (fn_initrank)dlsym(lib, "ncclCommInitRank");
    g_nccl.allreduce = (fn_allreduce)dlsym(lib, "ncclAllReduce");
    g_nccl.destroy = (fn_destroy)dlsym(lib, "ncclCommDestroy");
    g_nccl.errstr = (fn_errstr)dlsym(lib, "ncclGetErrorString");
    if (!g_nccl.getuid || !g_nccl.initrank || !g_nccl.allreduce || !g_nccl.destroy) { pyvb_set_error("librccl lacks a required symbol"); return PYVB_E_RCCL; }
    g_nccl.lib = lib;
    return PYVB_OK;
}
#define NCCLCHK(x) do { int _r = (x); if (_r != 0) { pyvb_set_error("RCCL error %d (%s) in %s", _r, g_nccl.errstr ? g_nccl.errstr(_r) : "?", #x); return PYVB_E_RCCL; } } while (0)

int pyvb_comm_unique_id(char id[128]) {
    ARGCHK(id, "id is NULL");
    int rc = load_rccl();
    if (rc) return rc;
    nccl_uid u;
    NCCLCHK(g_nccl.getuid(&u));
    memcpy(id, u.internal, 128);
    return PYVB_OK;
}

}  // extern "C"

// shared with the PCA path (api_pca.hip)
int pyvb_comm_create(pyvb_comm** comm, const char id[128], int rank, int world) {
    ARGCHK(comm && id && world >= 1 && rank >= 0 && rank < world, "bad communicator arguments");
    ARGCHK(!*comm, "a communicator is attached already");
    int rc = load_rccl();
    if (rc) return rc;
    nccl_uid u;
    memcpy(u.internal, id, 128);
    void* nc = nullptr;
    NCCLCHK(g_nccl.initrank(&nc, world, u, rank));
    pyvb_comm* c = new pyvb_comm();
    c->nccl = nc; c->fn = nullptr; c->user = nullptr; c->host = nullptr; c->cap = 0;
    *comm = c;
    return PYVB_OK;
}
int pyvb_comm_create_host(pyvb_comm** comm, pyvb_host_allreduce_fn fn, void* user) {
    ARGCHK(comm && fn, "bad communicator arguments");
    pyvb_comm* c = new pyvb_comm();
    c->nccl = nullptr; c->fn = fn; c->user = user; c->host = nullptr; c->cap = 0;
    *comm = c;
    return PYVB_OK;
}
void pyvb_comm_free(pyvb_comm* c) {
    if (!c) return;
    if (c->nccl && g_nccl.destroy) g_nccl.destroy(c->nccl);
    if (c->host) (void)hipHostFree(c->host);
    delete c;
}
int pyvb_allreduce_f64(pyvb_comm* c, double* buf, size_t count, hipStream_t stream) {
    if (c->nccl) {
        NCCLCHK(g_nccl.allreduce(buf, buf, count, 8, 0, c->nccl, stream));     // ncclDouble = 8, ncclSum = 0
        return PYVB_OK;
    }
    // host transport: device -> pinned host, the caller's all-reduce (blocking, in place), back.  The stream waits for it.
    if (c->cap < count) {
        if (c->host) (void)hipHostFree(c->host);
        c->host = nullptr; c->cap = 0;
        HIPCHK(hipHostMalloc((void**)&c->host, count * sizeof(double), hipHostMallocDefault));
        c->cap = count;
    }
    HIPCHK(hipMemcpyAsync(c->host, buf, count * sizeof(double), hipMemcpyDeviceToHost, stream));
    HIPCHK(hipStreamSynchronize(stream));
    const int r = c->fn(c->host, count, c->user);
    if (r != 0) { pyvb_set_error("the host all-reduce callback failed (%d)", r); return PYVB_E_RCCL; }
    HIPCHK(hipMemcpyAsync(buf, c->host, count * sizeof(double), hipMemcpyHostToDevice, stream));
    HIPCHK(hipStreamSynchronize(stream));          // the staging buffer is reused by the next call
    return PYVB_OK;
}

extern "C" {

int pyvb_lds_comm_init(pyvb_lds* h, const char id[128], int rank, int world) {
    ENTER(h);
    int rc = pyvb_comm_create(&h->comm, id, rank, world);
    if (rc) return rc;
    h->rank = rank; h->world = world;
    return PYVB_OK;
}

int pyvb_lds_comm_init_host(pyvb_lds* h, pyvb_host_allreduce_fn fn, void* user, int rank, int world) {
    ENTER(h);
    ARGCHK(fn && world >= 1 && rank >= 0 && rank < world, "bad communicator arguments");
    ARGCHK(!h->comm, "a communicator is attached already");
    int rc = pyvb_comm_create_host(&h->comm, fn, user);
    if (rc) return rc;
    h->rank = rank; h->world = world;
    return PYVB_OK;
}

int pyvb_lds_comm_destroy(pyvb_lds* h) {
    if (h && h->comm) { pyvb_comm_free(h->comm); h->comm = nullptr; h->world = 1; }
    return PYVB_OK;
}

int pyvb_lds_elbo_total(pyvb_lds* h, double out[6]) {
    ENTER(h);
    ARGCHK(out, "out is NULL");
    int rc = launch_elbo_sum(h);
    if (rc) return rc;
    if (h->comm && (rc = pyvb_allreduce_f64(h->comm, h->elbo_sum, 6, h->stream))) return rc;
    if ((rc = d2h(h, out, h->elbo_sum, 6))) return rc;
    return pyvb_lds_sync(h);
}

}  // extern "C"
