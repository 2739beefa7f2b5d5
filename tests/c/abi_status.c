/* A host program in plain C for the per-replicate entries of include/pyvb_hip.h: pyvb_lds_get_status, pyvb_lds_set_active,
 * pyvb_lds_get_active.  Builds like tests/c/abi_smoke.c and reads the same file format; replicate `bad` (second argument) has
 * been given a negative Q_b by the test that writes the file.  Prints what tests/test_status_c_abi_gpu.py compares with the
 * Python front end: the status word of every replicate after the failing sync, the mask, and the lower bound of two
 * iterations with the failed replicate switched off. */
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
    /* the argument checks need no device */
    int one = 0; unsigned char byte = 1;
    EXPECT(pyvb_lds_get_status(NULL, &one), PYVB_E_ARG);
    EXPECT(pyvb_lds_set_active(NULL, &byte), PYVB_E_ARG);
    EXPECT(pyvb_lds_get_active(NULL, &byte), PYVB_E_ARG);
    if (argc < 3) { printf("argument checks ok\n"); return 0; }
    FILE* f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    const int bad = atoi(argv[2]);
    double* hdr = rd(f, 4);
    const int N = (int)hdr[0], T = (int)hdr[1], D = (int)hdr[2], K = (int)hdr[3];
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
    CHECK(pyvb_lds_create(&h, 0, N, T, D, K, PYVB_NOISE_DIAGONAL_GAMMA));
    EXPECT(pyvb_lds_get_status(h, NULL), PYVB_E_ARG);
    EXPECT(pyvb_lds_set_active(h, NULL), PYVB_E_ARG);
    EXPECT(pyvb_lds_get_active(h, NULL), PYVB_E_ARG);
    CHECK(pyvb_lds_set_priors(h, x0_mean, x0_prec, A_pm, A_pp, C_pm, C_pp, qa0, qa0, ra0, ra0));
    CHECK(pyvb_lds_set_observations(h, Y));
    CHECK(pyvb_lds_set_state(h, X, A_mean, A_var, C_mean, C_var, Q_b, R_b));
    int* status = (int*)malloc(N * sizeof(int));
    unsigned char* mask = (unsigned char*)malloc(N);
    CHECK(pyvb_lds_get_active(h, mask));
    for (int n = 0; n < N; ++n) if (mask[n] != 1) { fprintf(stderr, "replicate %d starts switched off\n", n); return 4; }
    CHECK(pyvb_lds_sweep(h, PYVB_FORWARD));
    EXPECT(pyvb_lds_sync(h), PYVB_E_LINALG);
    printf("sync: %s\n", pyvb_last_error());
    CHECK(pyvb_lds_get_status(h, status));
    printf("status");
    for (int n = 0; n < N; ++n) printf(" %d", status[n]);
    printf("\n");
    if (!(status[bad] & PYVB_FAIL_STATES)) { fprintf(stderr, "replicate %d carries no PYVB_FAIL_STATES\n", bad); return 4; }
    mask[bad] = 0;
    CHECK(pyvb_lds_set_active(h, mask));
    CHECK(pyvb_lds_iterate(h, 2));
    CHECK(pyvb_lds_sync(h));                    /* the switched-off replicate does not fail the handle again */
    CHECK(pyvb_lds_get_status(h, status));
    for (int n = 0; n < N; ++n) if (status[n]) { fprintf(stderr, "status[%d] = %d after a successful sync\n", n, status[n]); return 4; }
    memset(mask, 1, N);
    EXPECT(pyvb_lds_set_active(h, mask), PYVB_E_ARG);       /* the mask can only shrink */
    CHECK(pyvb_lds_get_active(h, mask));
    printf("active");
    for (int n = 0; n < N; ++n) printf(" %d", (int)mask[n]);
    printf("\n");
    double hist[2 * 6];
    int count = 0;
    CHECK(pyvb_lds_get_elbo_history(h, hist, 2, &count));
    for (int it = 0; it < count; ++it) {
        double tot = 0.0;
        for (int p = 0; p < 6; ++p) tot += hist[it * 6 + p];
        printf("iteration %d lower bound %.17g\n", it + 1, tot);
    }
    CHECK(pyvb_lds_destroy(h));
    return 0;
}
