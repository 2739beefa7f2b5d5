/* A host program in plain C for the regressor entries of include/pyvb_hip.h: pyvb_lds_create_regressors, pyvb_lds_set_regressors,
 * pyvb_lds_get_regressors, pyvb_lds_set_regressor_priors, pyvb_lds_set_regressor_state, pyvb_lds_get_regressor_state and
 * pyvb_lds_update_E.  Builds like tests/c/abi_smoke.c.  The file it reads starts with N, T, D, K, Pv (as doubles), then Y, V, X, A_mean,
 * A_colvar, C_mean, C_colvar, Q_b, R_b, E_mean, E_colvar.  It creates a handle with Pv regressors and no input, iterates, calls
 * pyvb_lds_update_E once more, reads E and the lower bound back and prints them; tests/test_regressors_c_abi_gpu.py compares them
 * with the Python front end on the same inputs. */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "pyvb_hip.h"

#define CHECK(call) do { int rc_ = (call); if (rc_ != PYVB_OK) { fprintf(stderr, "%s failed: %d %s\n", #call, rc_, pyvb_last_error()); return 1; } } while (0)
#define EXPECT(call, want) do { int rc_ = (call); if (rc_ != (want)) { fprintf(stderr, "%s gave %d, expected %d (%s)\n", #call, rc_, (want), pyvb_last_error()); return 1; } } while (0)
#define NAMES(word) do { if (!strstr(pyvb_last_error(), word)) { fprintf(stderr, "the message does not name %s: %s\n", word, pyvb_last_error()); return 4; } } while (0)

static double* rd(FILE* f, size_t n) {
    double* p = (double*)malloc(n * sizeof(double));
    if (!p || fread(p, sizeof(double), n, f) != n) { fprintf(stderr, "short read\n"); exit(2); }
    return p;
}

int main(int argc, char** argv) {
    /* the argument checks and the refusals need no device */
    pyvb_lds* h = NULL;
    double one[4] = {1.0, 1.0, 1.0, 1.0};
    EXPECT(pyvb_lds_create_regressors(&h, 0, 2, 5, 3, 3, 0, 0, PYVB_NOISE_DIAGONAL_GAMMA, NULL), PYVB_E_ARG);
    NAMES("Pv must be >= 1");
    EXPECT(pyvb_lds_create_regressors(&h, 0, 2, 5, 3, 3, -1, 1, PYVB_NOISE_DIAGONAL_GAMMA, NULL), PYVB_E_ARG);
    NAMES("P must be >= 0");
    EXPECT(pyvb_lds_create_regressors(&h, 0, 2, 5, 3, 3, 0, 2, PYVB_NOISE_WISHART, NULL), PYVB_E_UNSUPPORTED);
    NAMES("regressors"); NAMES("Wishart");
    EXPECT(pyvb_lds_create_regressors(&h, 0, 2, 5, 3, 1, 0, 64, PYVB_NOISE_GAMMA, NULL), PYVB_E_UNSUPPORTED);
    NAMES("regressors"); NAMES("max(D, K + 2 P + Pv) <= 64");
    EXPECT(pyvb_lds_create_regressors(&h, 0, 2, 5, 3, 20, 20, 5, PYVB_NOISE_GAMMA, NULL), PYVB_E_UNSUPPORTED);
    if (h) { fprintf(stderr, "a refused create returned a handle\n"); return 4; }
    EXPECT(pyvb_lds_set_regressors(NULL, one), PYVB_E_ARG);
    EXPECT(pyvb_lds_get_regressors(NULL, one), PYVB_E_ARG);
    EXPECT(pyvb_lds_set_regressor_priors(NULL, one, one), PYVB_E_ARG);
    EXPECT(pyvb_lds_set_regressor_state(NULL, one, one), PYVB_E_ARG);
    EXPECT(pyvb_lds_get_regressor_state(NULL, one, one, one, one), PYVB_E_ARG);
    EXPECT(pyvb_lds_update_E(NULL), PYVB_E_ARG);
    if (pyvb_version() < 111) { fprintf(stderr, "pyvb_version %d\n", pyvb_version()); return 4; }
    if (argc < 3) { printf("argument checks ok\n"); return 0; }

    FILE* f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    const int niters = atoi(argv[2]);
    double* hdr = rd(f, 5);
    const int N = (int)hdr[0], T = (int)hdr[1], D = (int)hdr[2], K = (int)hdr[3], Pv = (int)hdr[4];
    double* Y = rd(f, (size_t)N * T * K);
    double* V = rd(f, (size_t)N * T * Pv);
    double* X = rd(f, (size_t)N * T * D);
    double* A_mean = rd(f, (size_t)N * D * D); double* A_var = rd(f, (size_t)N * D * D);
    double* C_mean = rd(f, (size_t)N * K * D); double* C_var = rd(f, (size_t)N * D * K);
    double* Q_b = rd(f, (size_t)N * D); double* R_b = rd(f, (size_t)N * K);
    double* E_mean = rd(f, (size_t)N * K * Pv); double* E_var = rd(f, (size_t)N * Pv * K);
    fclose(f);

    double* x0_mean = (double*)calloc(D, sizeof(double));
    double* x0_prec = (double*)calloc((size_t)D * D, sizeof(double));
    double* A_pm = (double*)calloc((size_t)D * D, sizeof(double)); double* A_pp = (double*)malloc((size_t)D * D * sizeof(double));
    double* C_pm = (double*)calloc((size_t)K * D, sizeof(double)); double* C_pp = (double*)malloc((size_t)D * K * sizeof(double));
    double* E_pm = (double*)calloc((size_t)K * Pv, sizeof(double)); double* E_pp = (double*)malloc((size_t)Pv * K * sizeof(double));
    double* qa0 = (double*)malloc(D * sizeof(double)); double* ra0 = (double*)malloc(K * sizeof(double));
    for (int i = 0; i < D; ++i) { x0_prec[i * D + i] = 1.0; qa0[i] = 1e-3; }
    for (int i = 0; i < D * D; ++i) A_pp[i] = 1e-3;
    for (int i = 0; i < D * K; ++i) C_pp[i] = 1e-3;
    for (int i = 0; i < Pv * K; ++i) E_pp[i] = 1e-3;
    for (int i = 0; i < K; ++i) ra0[i] = 1e-3;

    CHECK(pyvb_lds_create_regressors(&h, 0, N, T, D, K, 0, Pv, PYVB_NOISE_DIAGONAL_GAMMA, NULL));
    CHECK(pyvb_lds_set_priors(h, x0_mean, x0_prec, A_pm, A_pp, C_pm, C_pp, qa0, qa0, ra0, ra0));
    CHECK(pyvb_lds_set_observations(h, Y));
    CHECK(pyvb_lds_set_state(h, X, A_mean, A_var, C_mean, C_var, Q_b, R_b));
    /* an update before the regressors and their priors are there; the entries of a handle with inputs on this one */
    EXPECT(pyvb_lds_iterate(h, 1), PYVB_E_ARG);
    NAMES("pyvb_lds_set_regressors");
    EXPECT(pyvb_lds_update_B(h), PYVB_E_ARG);
    EXPECT(pyvb_lds_set_regressors(h, NULL), PYVB_E_ARG);
    E_pp[Pv * K - 1] = 0.0;
    EXPECT(pyvb_lds_set_regressor_priors(h, E_pm, E_pp), PYVB_E_ARG);
    E_pp[Pv * K - 1] = 1e-3;
    CHECK(pyvb_lds_set_regressors(h, V));
    EXPECT(pyvb_lds_iterate(h, 1), PYVB_E_ARG);
    NAMES("pyvb_lds_set_regressor_priors");
    CHECK(pyvb_lds_set_regressor_priors(h, E_pm, E_pp));
    CHECK(pyvb_lds_set_regressor_state(h, E_mean, E_var));
    double* Vb = (double*)malloc((size_t)N * T * Pv * sizeof(double));
    CHECK(pyvb_lds_get_regressors(h, Vb));
    if (memcmp(Vb, V, (size_t)N * T * Pv * sizeof(double))) { fprintf(stderr, "V does not read back\n"); return 4; }
    double* qld = (double*)malloc((size_t)N * Pv * sizeof(double));
    CHECK(pyvb_lds_get_regressor_state(h, NULL, NULL, qld, NULL));
    if (qld[0] == qld[0]) { fprintf(stderr, "qld_E is %.17g before the first update\n", qld[0]); return 4; }
    CHECK(pyvb_lds_iterate(h, niters));
    CHECK(pyvb_lds_update_E(h));
    CHECK(pyvb_lds_elbo(h));
    double* parts = (double*)malloc((size_t)N * 6 * sizeof(double));
    CHECK(pyvb_lds_get_elbo(h, parts));
    double* Em = (double*)malloc((size_t)N * K * Pv * sizeof(double));
    double* lnd = (double*)malloc((size_t)N * Pv * sizeof(double));
    CHECK(pyvb_lds_get_regressor_state(h, Em, NULL, qld, lnd));
    for (int n = 0; n < N; ++n) {
        double tot = 0.0;
        for (int p = 0; p < 6; ++p) tot += parts[n * 6 + p];
        printf("replicate %d lower bound %.17g\n", n, tot);
    }
    for (size_t i = 0; i < (size_t)N * K * Pv; ++i) printf("E %.17g\n", Em[i]);
    for (size_t i = 0; i < (size_t)N * Pv; ++i)
        if (!isfinite(qld[i]) || !isfinite(lnd[i])) { fprintf(stderr, "qld_E / lnd_E of column %d is not finite after an update\n", (int)i); return 4; }
    CHECK(pyvb_lds_destroy(h));
    printf("done\n");
    return 0;
}
