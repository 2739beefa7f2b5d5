/* A host program in plain C for the per-entry precision entries of include/pyvb_hip.h: pyvb_lds_set_entry_precisions,
 * pyvb_lds_get_entry_precisions, pyvb_lds_update_entry_precisions.  Builds like tests/c/abi_smoke.c.  The file it reads starts with
 * N, T, D, K, then the arrays of tests/c/abi_lengths.c's format, then a0[D][D], b0[D][D] and qb[N][D][D] for A and a0[D][K], b0[D][K]
 * and qb[N][D][K] for C.  It creates the handle, gives both matrices DiagonalGamma parents, iterates, reads qa / qb and the lower
 * bound back and prints them; tests/test_entry_c_abi_gpu.py compares them with the Python front end on the same inputs. */
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
    /* a NULL handle needs no device */
    double one[4] = {1.0, 1.0, 1.0, 1.0};
    EXPECT(pyvb_lds_set_entry_precisions(NULL, 0, one, one, one), PYVB_E_ARG);
    NAMES("handle is NULL");
    EXPECT(pyvb_lds_get_entry_precisions(NULL, 1, one, one), PYVB_E_ARG);
    EXPECT(pyvb_lds_update_entry_precisions(NULL, 0), PYVB_E_ARG);
    if (argc < 3) { printf("argument checks ok\n"); return 0; }

    FILE* f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    const int niters = atoi(argv[2]);
    double* hdr = rd(f, 4);
    const int N = (int)hdr[0], T = (int)hdr[1], D = (int)hdr[2], K = (int)hdr[3];
    double* Y = rd(f, (size_t)N * T * K);
    double* X = rd(f, (size_t)N * T * D);
    double* A_mean = rd(f, (size_t)N * D * D); double* A_var = rd(f, (size_t)N * D * D);
    double* C_mean = rd(f, (size_t)N * K * D); double* C_var = rd(f, (size_t)N * D * K);
    double* Q_b = rd(f, (size_t)N * D); double* R_b = rd(f, (size_t)N * K);
    double *a0[2], *b0[2], *qb0[2];
    size_t per[2];
    per[0] = (size_t)D * D; per[1] = (size_t)D * K;
    for (int w = 0; w < 2; ++w) { a0[w] = rd(f, per[w]); b0[w] = rd(f, per[w]); qb0[w] = rd(f, (size_t)N * per[w]); }
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
    double* qa = (double*)malloc((size_t)N * per[1] * sizeof(double));
    double* qb = (double*)malloc((size_t)N * per[1] * sizeof(double));
    EXPECT(pyvb_lds_get_entry_precisions(h, 0, qa, qb), PYVB_E_ARG);        /* Constant parents so far */
    NAMES("no DiagonalGamma precision parents");
    EXPECT(pyvb_lds_update_entry_precisions(h, 1), PYVB_E_ARG);
    EXPECT(pyvb_lds_set_entry_precisions(h, 2, a0[0], b0[0], qb0[0]), PYVB_E_ARG);
    NAMES("which");
    for (int w = 0; w < 2; ++w) CHECK(pyvb_lds_set_entry_precisions(h, w, a0[w], b0[w], qb0[w]));
    EXPECT(pyvb_lds_get_column_precisions(h, 1, qa, qb), PYVB_E_ARG);       /* the Gamma entries do not serve these parents */
    NAMES("DiagonalGamma precision parents");
    CHECK(pyvb_lds_get_entry_precisions(h, 1, qa, qb));
    for (size_t i = 0; i < (size_t)N * per[1]; ++i)
        if (qb[i] != qb0[1][i] || qa[i] != a0[1][i % per[1]] + 0.5) { fprintf(stderr, "entry %d of C: qa %.17g qb %.17g\n", (int)i, qa[i], qb[i]); return 4; }
    CHECK(pyvb_lds_iterate(h, niters));
    CHECK(pyvb_lds_elbo(h));
    double* parts = (double*)malloc((size_t)N * 6 * sizeof(double));
    CHECK(pyvb_lds_get_elbo(h, parts));
    for (int n = 0; n < N; ++n) {
        double tot = 0.0;
        for (int p = 0; p < 6; ++p) tot += parts[n * 6 + p];
        printf("replicate %d lower bound %.17g\n", n, tot);
    }
    for (int w = 0; w < 2; ++w) {
        CHECK(pyvb_lds_get_entry_precisions(h, w, NULL, qb));        /* NULL = skip */
        printf("qb %c", w == 0 ? 'A' : 'C');
        for (size_t i = 0; i < (size_t)N * per[w]; ++i) printf(" %.17g", qb[i]);
        printf("\n");
    }
    /* the explicit entry: the columns have not changed since iterate's own precision update, so qb comes out the same */
    double* again = (double*)malloc((size_t)N * per[1] * sizeof(double));
    CHECK(pyvb_lds_update_entry_precisions(h, 1));
    CHECK(pyvb_lds_get_entry_precisions(h, 1, NULL, again));
    if (memcmp(again, qb, (size_t)N * per[1] * sizeof(double))) { fprintf(stderr, "a second precision update of C changed qb\n"); return 4; }
    /* back to Constant parents */
    CHECK(pyvb_lds_set_priors(h, x0_mean, x0_prec, A_pm, A_pp, C_pm, C_pp, qa0, qa0, ra0, ra0));
    EXPECT(pyvb_lds_get_entry_precisions(h, 0, qa, qb), PYVB_E_ARG);
    CHECK(pyvb_lds_destroy(h));
    printf("done\n");
    return 0;
}
