/* A host program in plain C for the shared-parameter entries of include/pyvb_hip.h: pyvb_lds_create_tied and
 * pyvb_lds_get_models.  Builds like tests/c/abi_smoke.c.  The file it reads starts with N, T, D, K, then the N lengths and the N
 * model ids (as doubles), then the arrays of tests/c/abi_lengths.c's format.  It creates the handle, iterates, reads models,
 * parameters and the lower bound back and prints the total of every model; tests/test_tied_c_abi_gpu.py passes the expected
 * totals of two models on the command line (from the Python front end on the same inputs) and this program compares them. */
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
    /* the argument checks and the refusals need no device */
    pyvb_lds* h = NULL;
    int len3[3] = {5, 4, 2}, from1[3] = {1, 1, 2}, down[3] = {0, 1, 0}, gap[3] = {0, 0, 2}, ok[3] = {0, 1, 1};
    EXPECT(pyvb_lds_get_models(NULL, ok), PYVB_E_ARG);
    EXPECT(pyvb_lds_create_tied(&h, 0, 3, 5, 3, 3, PYVB_NOISE_DIAGONAL_GAMMA, len3, from1), PYVB_E_ARG);
    NAMES("replicate 0 ");
    EXPECT(pyvb_lds_create_tied(&h, 0, 3, 5, 3, 3, PYVB_NOISE_DIAGONAL_GAMMA, len3, down), PYVB_E_ARG);
    NAMES("replicate 2 ");
    EXPECT(pyvb_lds_create_tied(&h, 0, 3, 5, 3, 3, PYVB_NOISE_GAMMA, NULL, gap), PYVB_E_ARG);
    NAMES("replicate 2 ");
    EXPECT(pyvb_lds_create_tied(&h, 0, 3, 5, 3, 3, PYVB_NOISE_WISHART, NULL, ok), PYVB_E_UNSUPPORTED);
    EXPECT(pyvb_lds_create_tied(&h, 0, 3, 5, 65, 3, PYVB_NOISE_GAMMA, NULL, ok), PYVB_E_UNSUPPORTED);
    EXPECT(pyvb_lds_create_tied(&h, 0, 3, 5, 3, 65, PYVB_NOISE_DIAGONAL_GAMMA, len3, ok), PYVB_E_UNSUPPORTED);
    if (h) { fprintf(stderr, "a refused create returned a handle\n"); return 4; }
    if (argc < 7) { printf("argument checks ok\n"); return 0; }

    FILE* f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    const int niters = atoi(argv[2]);
    const int ma = atoi(argv[3]), mb = atoi(argv[5]);
    const double want_a = strtod(argv[4], NULL), want_b = strtod(argv[6], NULL);
    double* hdr = rd(f, 4);
    const int N = (int)hdr[0], T = (int)hdr[1], D = (int)hdr[2], K = (int)hdr[3];
    double* lend = rd(f, (size_t)N);
    double* modd = rd(f, (size_t)N);
    int* lengths = (int*)malloc(N * sizeof(int));
    int* model = (int*)malloc(N * sizeof(int));
    for (int n = 0; n < N; ++n) { lengths[n] = (int)lend[n]; model[n] = (int)modd[n]; }
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

    CHECK(pyvb_lds_create_tied(&h, 0, N, T, D, K, PYVB_NOISE_DIAGONAL_GAMMA, lengths, model));
    EXPECT(pyvb_lds_get_models(h, NULL), PYVB_E_ARG);
    int* back = (int*)malloc(N * sizeof(int));
    CHECK(pyvb_lds_get_models(h, back));
    printf("models");
    for (int n = 0; n < N; ++n) {
        printf(" %d", back[n]);
        if (back[n] != model[n]) { fprintf(stderr, "model %d reads back as %d, not %d\n", n, back[n], model[n]); return 4; }
    }
    printf("\n");
    CHECK(pyvb_lds_get_lengths(h, back));
    for (int n = 0; n < N; ++n)
        if (back[n] != lengths[n]) { fprintf(stderr, "length %d reads back as %d, not %d\n", n, back[n], lengths[n]); return 4; }
    CHECK(pyvb_lds_set_priors(h, x0_mean, x0_prec, A_pm, A_pp, C_pm, C_pp, qa0, qa0, ra0, ra0));
    CHECK(pyvb_lds_set_observations(h, Y));
    CHECK(pyvb_lds_set_state(h, X, A_mean, A_var, C_mean, C_var, Q_b, R_b));
    int iters_run = -1;
    EXPECT(pyvb_lds_iterate_until(h, 3, 1e-3, 1, &iters_run), PYVB_E_UNSUPPORTED);
    CHECK(pyvb_lds_iterate(h, niters));
    CHECK(pyvb_lds_elbo(h));
    double* parts = (double*)malloc((size_t)N * 6 * sizeof(double));
    CHECK(pyvb_lds_get_elbo(h, parts));
    double* Q_a = (double*)malloc((size_t)N * D * sizeof(double));
    double* R_a = (double*)malloc((size_t)N * K * sizeof(double));
    double* Am = (double*)malloc((size_t)N * D * D * sizeof(double));
    CHECK(pyvb_lds_get_state(h, NULL, Am, NULL, NULL, NULL, Q_a, NULL, R_a, NULL));
    for (int n0 = 0; n0 < N;) {
        int n1 = n0 + 1;
        long nq = lengths[n0] - 1, nr = lengths[n0];
        while (n1 < N && model[n1] == model[n0]) { nq += lengths[n1] - 1; nr += lengths[n1]; ++n1; }
        double tot = 0.0;
        for (int n = n0; n < n1; ++n) {
            for (int p = 0; p < 6; ++p) tot += parts[n * 6 + p];
            /* Q has the children of every chain of the model (nodes_todo.py:183-186), R likewise */
            if (Q_a[(size_t)n * D] != 1e-3 + 0.5 * nq || R_a[(size_t)n * K] != 1e-3 + 0.5 * nr) {
                fprintf(stderr, "replicate %d: Q_a %.17g, R_a %.17g\n", n, Q_a[(size_t)n * D], R_a[(size_t)n * K]);
                return 4;
            }
            if (memcmp(Am + (size_t)n * D * D, Am + (size_t)n0 * D * D, (size_t)D * D * sizeof(double))) {
                fprintf(stderr, "A_mean of replicates %d and %d of model %d differ\n", n0, n, model[n0]);
                return 4;
            }
            for (int p = 2; p < 6; ++p)
                if (n > n0 && parts[n * 6 + p] != 0.0) { fprintf(stderr, "part %d of replicate %d is %.17g, not 0\n", p, n, parts[n * 6 + p]); return 4; }
        }
        printf("model %d lower bound %.17g\n", model[n0], tot);
        const double want = model[n0] == ma ? want_a : want_b;
        if ((model[n0] == ma || model[n0] == mb) && !(fabs(tot - want) <= 1e-12 * fabs(want))) {
            fprintf(stderr, "model %d: lower bound %.17g, expected %.17g\n", model[n0], tot, want);
            return 5;
        }
        n0 = n1;
    }
    /* a mask may not split a model */
    unsigned char* mask = (unsigned char*)malloc(N);
    memset(mask, 1, N);
    for (int n = 1; n < N; ++n)
        if (model[n] == model[n - 1]) { mask[n] = 0; break; }
    EXPECT(pyvb_lds_set_active(h, mask), PYVB_E_ARG);
    NAMES("model ");
    double hist[6];
    int count = 0;
    CHECK(pyvb_lds_get_elbo_history(h, hist, 1, &count));
    double all = 0.0;
    for (int p = 0; p < 6; ++p) all += hist[p];
    printf("history %.17g\n", all);
    CHECK(pyvb_lds_destroy(h));
    printf("compared models %d and %d\n", ma, mb);
    return 0;
}
