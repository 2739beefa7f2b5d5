/* A host program in plain C for the per-model convergence entries of include/pyvb_hip.h: pyvb_lds_iterate_until_model and
 * pyvb_lds_get_model_convergence.  Builds like tests/c/abi_smoke.c; the file it reads has tests/c/abi_tied.c's format (N, T, D, K,
 * the N lengths and the N model ids as doubles, then the arrays).  It creates the tied handle, checks that the per-replicate
 * entry still refuses it, runs every model to its own stop and prints per model the iterations, whether it converged and the
 * last bound; tests/test_model_converge_c_abi_gpu.py compares them with the Python front end and the comparator. */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "pyvb_hip.h"

#define CHECK(call) do { int rc_ = (call); if (rc_ != PYVB_OK) { fprintf(stderr, "%s failed: %d %s\n", #call, rc_, pyvb_last_error()); return 1; } } while (0)
#define EXPECT(call, want) do { int rc_ = (call); if (rc_ != (want)) { fprintf(stderr, "%s gave %d, expected %d (%s)\n", #call, rc_, (want), pyvb_last_error()); return 1; } } while (0)
#define NAMES(what) do { if (!strstr(pyvb_last_error(), what)) { fprintf(stderr, "the message does not name %s: %s\n", what, pyvb_last_error()); return 4; } } while (0)

static double* rd(FILE* f, size_t n) {
    double* p = (double*)malloc(n * sizeof(double));
    if (!p || fread(p, sizeof(double), n, f) != n) { fprintf(stderr, "short read\n"); exit(2); }
    return p;
}

int main(int argc, char** argv) {
    /* the argument checks need no device: they come before the handle is looked into */
    static double not_a_handle[16];
    pyvb_lds* fake = (pyvb_lds*)not_a_handle;
    int iters_run = -1;
    EXPECT(pyvb_lds_iterate_until_model(NULL, 3, 1e-3, 1, &iters_run), PYVB_E_ARG);
    NAMES("handle is NULL");
    EXPECT(pyvb_lds_get_model_convergence(NULL, NULL, NULL, NULL), PYVB_E_ARG);
    NAMES("handle is NULL");
    EXPECT(pyvb_lds_iterate_until_model(fake, -1, 1e-3, 1, &iters_run), PYVB_E_ARG);
    NAMES("max_iters");
    EXPECT(pyvb_lds_iterate_until_model(fake, 3, 1e-3, 0, &iters_run), PYVB_E_ARG);
    NAMES("check_every");
    EXPECT(pyvb_lds_iterate_until_model(fake, 3, NAN, 1, &iters_run), PYVB_E_ARG);
    NAMES("NaN");
    EXPECT(pyvb_lds_iterate_until_model(fake, 3, 1e-3, 1, NULL), PYVB_E_ARG);
    NAMES("iters_run");
    if (pyvb_version() < 104) { fprintf(stderr, "pyvb_version() = %d\n", pyvb_version()); return 4; }
    if (argc < 4) { printf("argument checks ok\n"); return 0; }

    FILE* f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    const int max_iters = atoi(argv[2]);
    const double tol = strtod(argv[3], NULL);
    double* hdr = rd(f, 4);
    const int N = (int)hdr[0], T = (int)hdr[1], D = (int)hdr[2], K = (int)hdr[3];
    double* lend = rd(f, (size_t)N);
    double* modd = rd(f, (size_t)N);
    int* lengths = (int*)malloc(N * sizeof(int));
    int* model = (int*)malloc(N * sizeof(int));
    for (int n = 0; n < N; ++n) { lengths[n] = (int)lend[n]; model[n] = (int)modd[n]; }
    const int M = model[N - 1] + 1;
    double* Y = rd(f, (size_t)N * T * K);
    double* X = rd(f, (size_t)N * T * D);
    double* A_mean = rd(f, (size_t)N * D * D); double* A_var = rd(f, (size_t)N * D * D);
    double* C_mean = rd(f, (size_t)N * K * D); double* C_var = rd(f, (size_t)N * D * K);
    double* Q_b = rd(f, (size_t)N * D); double* R_b = rd(f, (size_t)N * K);
    fclose(f);

    double* x0_mean = (double*)calloc(D, sizeof(double));
    double* x0_prec = (double*)calloc((size_t)D * D, sizeof(double));
    double* A_pm = (double*)calloc((size_t)D * D, sizeof(double)); double* A_pp = (double*)malloc((size_t)D * D * sizeof(double));
    double* C_pm = (double*)calloc((size_t)K * D, sizeof(double)); double* C_pp = (double*)malloc((size_t)D * K * sizeof(double));
    double* qa0 = (double*)malloc(D * sizeof(double)); double* ra0 = (double*)malloc(K * sizeof(double));
    for (int i = 0; i < D; ++i) { x0_prec[i * D + i] = 1.0; qa0[i] = 1e-3; }
    for (int i = 0; i < D * D; ++i) A_pp[i] = 1e-3;
    for (int i = 0; i < D * K; ++i) C_pp[i] = 1e-3;
    for (int i = 0; i < K; ++i) ra0[i] = 1e-3;

    pyvb_lds* h = NULL;
    CHECK(pyvb_lds_create_tied(&h, 0, N, T, D, K, PYVB_NOISE_DIAGONAL_GAMMA, lengths, model));
    CHECK(pyvb_lds_set_priors(h, x0_mean, x0_prec, A_pm, A_pp, C_pm, C_pp, qa0, qa0, ra0, ra0));
    CHECK(pyvb_lds_set_observations(h, Y));
    CHECK(pyvb_lds_set_state(h, X, A_mean, A_var, C_mean, C_var, Q_b, R_b));
    /* the per-replicate entry still refuses a handle with tied models, and says where to go */
    EXPECT(pyvb_lds_iterate_until(h, 3, 1e-3, 1, &iters_run), PYVB_E_UNSUPPORTED);
    NAMES("per model");
    NAMES("pyvb_lds_iterate_until_model");
    EXPECT(pyvb_lds_iterate_until_model(h, -1, tol, 1, &iters_run), PYVB_E_ARG);
    EXPECT(pyvb_lds_iterate_until_model(h, max_iters, tol, 0, &iters_run), PYVB_E_ARG);

    int* mit = (int*)malloc(M * sizeof(int)); unsigned char* mcv = (unsigned char*)malloc(M); double* mlb = (double*)malloc(M * sizeof(double));
    int* it = (int*)malloc(N * sizeof(int)); unsigned char* cv = (unsigned char*)malloc(N); double* lb = (double*)malloc(N * sizeof(double));
    CHECK(pyvb_lds_get_model_convergence(h, mit, mcv, mlb));
    for (int m = 0; m < M; ++m)
        if (mit[m] != 0 || mcv[m] != 0 || mlb[m] == mlb[m]) { fprintf(stderr, "model %d before the first call: %d %d %g\n", m, mit[m], mcv[m], mlb[m]); return 4; }

    CHECK(pyvb_lds_iterate_until_model(h, max_iters, tol, 1, &iters_run));
    printf("iterations launched %d\n", iters_run);
    CHECK(pyvb_lds_get_model_convergence(h, mit, mcv, mlb));
    CHECK(pyvb_lds_get_model_convergence(h, NULL, NULL, NULL));
    CHECK(pyvb_lds_get_convergence(h, it, cv, lb));
    double* parts = (double*)malloc((size_t)N * 6 * sizeof(double));
    CHECK(pyvb_lds_get_elbo(h, parts));
    int last = 0;
    for (int n = 0; n < N; ++n) {       /* every chain holds its model's values */
        const int m = model[n];
        if (it[n] != mit[m] || cv[n] != mcv[m] || lb[n] != mlb[m]) {
            fprintf(stderr, "replicate %d of model %d: %d %d %.17g, the model has %d %d %.17g\n", n, m, it[n], cv[n], lb[n], mit[m], mcv[m], mlb[m]);
            return 4;
        }
    }
    for (int n0 = 0; n0 < N;) {         /* the bound the test saw is the sum of the model's rows, part by part, then left to right */
        int n1 = n0 + 1;
        while (n1 < N && model[n1] == model[n0]) ++n1;
        double s[6];
        for (int p = 0; p < 6; ++p) { s[p] = parts[n0 * 6 + p]; for (int n = n0 + 1; n < n1; ++n) s[p] += parts[n * 6 + p]; }
        const double llb = ((((s[0] + s[1]) + s[2]) + s[3]) + s[4]) + s[5];
        const int m = model[n0];
        if (llb != mlb[m]) { fprintf(stderr, "model %d: llb %.17g, its rows add up to %.17g\n", m, mlb[m], llb); return 5; }
        printf("model %d: %d iterations, %s, lower bound %.17g\n", m, mit[m], mcv[m] ? "converged" : "still running", mlb[m]);
        if (mit[m] > last) last = mit[m];
        n0 = n1;
    }
    if (iters_run != last && iters_run != max_iters) { fprintf(stderr, "%d iterations launched, the last stop was at %d\n", iters_run, last); return 5; }
    /* everybody converged: nothing is launched */
    int all = 1;
    for (int m = 0; m < M; ++m) all = all && mcv[m];
    if (all) {
        CHECK(pyvb_lds_iterate_until_model(h, 5, tol, 1, &iters_run));
        if (iters_run != 0) { fprintf(stderr, "a call with every model converged launched %d iterations\n", iters_run); return 5; }
    }
    CHECK(pyvb_lds_destroy(h));
    printf("done\n");
    return 0;
}
