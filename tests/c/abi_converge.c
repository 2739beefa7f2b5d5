/* A host program in plain C for the convergence entries of include/pyvb_hip.h: pyvb_lds_iterate_until and
 * pyvb_lds_get_convergence.  Builds like tests/c/abi_smoke.c.  Without arguments it checks the arguments of both entries,
 * which needs no device.  With a problem file (N, T, D, K as doubles, then the arrays of tests/c/abi_status.c's format), max_iters,
 * tol and check_every it runs every replicate to its own stop and prints the per-replicate iteration counts, which
 * tests/test_converge_c_abi_gpu.py compares with those of the Python front end on the same inputs. */
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
    /* the argument checks need no device: they come before any HIP call, a handle that is not one is never looked into */
    int ran = -1;
    double not_a_handle[64];
    pyvb_lds* fake = (pyvb_lds*)not_a_handle;
    memset(not_a_handle, 0, sizeof(not_a_handle));
    EXPECT(pyvb_lds_iterate_until(NULL, 10, 1e-3, 8, &ran), PYVB_E_ARG);
    EXPECT(pyvb_lds_get_convergence(NULL, NULL, NULL, NULL), PYVB_E_ARG);
    EXPECT(pyvb_lds_iterate_until(fake, -1, 1e-3, 8, &ran), PYVB_E_ARG);
    EXPECT(pyvb_lds_iterate_until(fake, 10, 1e-3, 0, &ran), PYVB_E_ARG);
    if (!strstr(pyvb_last_error(), "check_every")) { fprintf(stderr, "the message does not name check_every: %s\n", pyvb_last_error()); return 4; }
    EXPECT(pyvb_lds_iterate_until(fake, 10, NAN, 8, &ran), PYVB_E_ARG);
    EXPECT(pyvb_lds_iterate_until(fake, 10, 1e-3, 8, NULL), PYVB_E_ARG);
    if (ran != -1) { fprintf(stderr, "a refused call wrote iters_run\n"); return 4; }
    if (argc < 5) { printf("argument checks ok\n"); return 0; }

    FILE* f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    const int max_iters = atoi(argv[2]), check_every = atoi(argv[4]);
    const double tol = strtod(argv[3], NULL);
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
    CHECK(pyvb_lds_set_priors(h, x0_mean, x0_prec, A_pm, A_pp, C_pm, C_pp, qa0, qa0, ra0, ra0));
    CHECK(pyvb_lds_set_observations(h, Y));
    CHECK(pyvb_lds_set_state(h, X, A_mean, A_var, C_mean, C_var, Q_b, R_b));
    CHECK(pyvb_lds_iterate_until(h, max_iters, tol, check_every, &ran));
    int* iters = (int*)malloc(N * sizeof(int));
    unsigned char* conv = (unsigned char*)malloc(N);
    double* llb = (double*)malloc(N * sizeof(double));
    CHECK(pyvb_lds_get_convergence(h, NULL, NULL, NULL));       /* any pointer may be NULL */
    CHECK(pyvb_lds_get_convergence(h, iters, conv, llb));
    printf("iters_run %d\n", ran);
    for (int n = 0; n < N; ++n) printf("replicate %d iters %d converged %d llb %.17g\n", n, iters[n], (int)conv[n], llb[n]);
    unsigned char* mask = (unsigned char*)malloc(N);
    CHECK(pyvb_lds_get_active(h, mask));
    for (int n = 0; n < N; ++n)
        if (!mask[n]) { fprintf(stderr, "replicate %d left the caller's mask\n", n); return 4; }
    CHECK(pyvb_lds_destroy(h));
    return 0;
}
