/* A host program in plain C for the chain-length entries of include/pyvb_hip.h: pyvb_lds_create_lengths and
 * pyvb_lds_get_lengths.  Builds like tests/c/abi_smoke.c.  The file it reads starts with N, T, D, K and the N lengths (as
 * doubles), then the arrays of tests/c/abi_status.c's format.  It creates the handle with lengths, iterates, reads the lengths
 * and the lower bound back and prints them; tests/test_lengths_c_abi_gpu.py passes the expected totals of two replicates on
 * the command line (from the Python front end on the same inputs) and this program compares them itself. */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "pyvb_hip.h"

#define CHECK(call) do { int rc_ = (call); if (rc_ != PYVB_OK) { fprintf(stderr, "%s failed: %d %s\n", #call, rc_, pyvb_last_error()); return 1; } } while (0)
#define EXPECT(call, want) do { int rc_ = (call); if (rc_ != (want)) { fprintf(stderr, "%s gave %d, expected %d (%s)\n", #call, rc_, (want), pyvb_last_error()); return 1; } } while (0)

static double* rd(FILE* f, size_t n) {
    double* p = (double*)malloc(n * sizeof(double));
    if (!p || fread(p, sizeof(double), n, f) != n) { fprintf(stderr, "short read\n"); exit(2); }
    return p;
}

int main(int argc, char** argv) {
    /* the argument checks and the refusals need no device */
    pyvb_lds* h = NULL;
    int two[2] = {5, 1}, len2[2] = {5, 4};
    EXPECT(pyvb_lds_get_lengths(NULL, two), PYVB_E_ARG);
    EXPECT(pyvb_lds_create_lengths(&h, 0, 2, 5, 3, 3, PYVB_NOISE_DIAGONAL_GAMMA, two), PYVB_E_ARG);
    if (!strstr(pyvb_last_error(), "replicate 1")) { fprintf(stderr, "the message does not name replicate 1: %s\n", pyvb_last_error()); return 4; }
    EXPECT(pyvb_lds_create_lengths(&h, 0, 2, 5, 3, 3, PYVB_NOISE_WISHART, len2), PYVB_E_UNSUPPORTED);
    EXPECT(pyvb_lds_create_lengths(&h, 0, 2, 5, 65, 3, PYVB_NOISE_GAMMA, len2), PYVB_E_UNSUPPORTED);
    if (h) { fprintf(stderr, "a refused create returned a handle\n"); return 4; }
    if (argc < 7) { printf("argument checks ok\n"); return 0; }

    FILE* f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    const int niters = atoi(argv[2]);
    const int ra = atoi(argv[3]), rb = atoi(argv[5]);
    const double want_a = strtod(argv[4], NULL), want_b = strtod(argv[6], NULL);
    double* hdr = rd(f, 4);
    const int N = (int)hdr[0], T = (int)hdr[1], D = (int)hdr[2], K = (int)hdr[3];
    double* lend = rd(f, (size_t)N);
    int* lengths = (int*)malloc(N * sizeof(int));
    for (int n = 0; n < N; ++n) lengths[n] = (int)lend[n];
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

    CHECK(pyvb_lds_create_lengths(&h, 0, N, T, D, K, PYVB_NOISE_DIAGONAL_GAMMA, lengths));
    EXPECT(pyvb_lds_get_lengths(h, NULL), PYVB_E_ARG);
    int* back = (int*)malloc(N * sizeof(int));
    CHECK(pyvb_lds_get_lengths(h, back));
    printf("lengths");
    for (int n = 0; n < N; ++n) {
        printf(" %d", back[n]);
        if (back[n] != lengths[n]) { fprintf(stderr, "length %d reads back as %d, not %d\n", n, back[n], lengths[n]); return 4; }
    }
    printf("\n");
    CHECK(pyvb_lds_set_priors(h, x0_mean, x0_prec, A_pm, A_pp, C_pm, C_pp, qa0, qa0, ra0, ra0));
    CHECK(pyvb_lds_set_observations(h, Y));
    CHECK(pyvb_lds_set_state(h, X, A_mean, A_var, C_mean, C_var, Q_b, R_b));
    CHECK(pyvb_lds_iterate(h, niters));
    CHECK(pyvb_lds_elbo(h));
    double* parts = (double*)malloc((size_t)N * 6 * sizeof(double));
    CHECK(pyvb_lds_get_elbo(h, parts));
    double* Q_a = (double*)malloc((size_t)N * D * sizeof(double));
    double* Xo = (double*)malloc((size_t)N * T * D * sizeof(double));
    CHECK(pyvb_lds_get_state(h, Xo, NULL, NULL, NULL, NULL, Q_a, NULL, NULL, NULL));
    for (int n = 0; n < N; ++n) {
        double tot = 0.0;
        for (int p = 0; p < 6; ++p) tot += parts[n * 6 + p];
        printf("replicate %d lower bound %.17g\n", n, tot);
        /* Q of replicate n has T_n - 1 children (nodes_todo.py:183-186) */
        if (Q_a[(size_t)n * D] != 1e-3 + 0.5 * (lengths[n] - 1)) { fprintf(stderr, "Q_a of replicate %d is %.17g\n", n, Q_a[(size_t)n * D]); return 4; }
        for (size_t i = ((size_t)n * T + lengths[n]) * D; i < (size_t)(n + 1) * T * D; ++i)
            if (Xo[i] != 0.0) { fprintf(stderr, "a padding row of X of replicate %d reads %.17g\n", n, Xo[i]); return 4; }
        const double want = n == ra ? want_a : want_b;
        if ((n == ra || n == rb) && !(fabs(tot - want) <= 1e-12 * fabs(want))) {
            fprintf(stderr, "replicate %d: lower bound %.17g, expected %.17g\n", n, tot, want);
            return 5;
        }
    }
    double hist[6];
    int count = 0;
    CHECK(pyvb_lds_get_elbo_history(h, hist, 1, &count));
    double all = 0.0;
    for (int p = 0; p < 6; ++p) all += hist[p];
    printf("history %.17g\n", all);
    CHECK(pyvb_lds_destroy(h));
    printf("compared replicates %d and %d\n", ra, rb);
    return 0;
}
