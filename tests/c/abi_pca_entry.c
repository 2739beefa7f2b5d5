/* A host program in plain C for the sparse-loadings entries of the VB-PCA path of include/pyvb_hip.h:
 * pyvb_pca_set_entry_precisions, pyvb_pca_get_entry_precisions, pyvb_pca_update_entry_precisions.  Builds like
 * tests/c/abi_pca_ard.c.  The file it reads starts with N, d, q, then X[N][d] (NaN = missing), X_missing[N][d], W_mean[d][q], Z[N][q],
 * Z_cov[q][q], Mu_mean[d], beta_b, W_prior_mean[d][q], a0[q][d], b0[q][d], qb[q][d].  It creates the handle, gives the columns of W
 * DiagonalGamma parents, iterates, reads qa / qb and the lower bound back and prints them; tests/test_pca_entry_c_abi_gpu.py compares them with the
 * Python front end on the same inputs. */
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
    EXPECT(pyvb_pca_set_entry_precisions(NULL, one, one, one), PYVB_E_ARG);
    NAMES("handle is NULL");
    EXPECT(pyvb_pca_get_entry_precisions(NULL, one, one), PYVB_E_ARG);
    EXPECT(pyvb_pca_update_entry_precisions(NULL), PYVB_E_ARG);
    if (argc < 3) { printf("argument checks ok\n"); return 0; }

    FILE* f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    const int niters = atoi(argv[2]);
    double* hdr = rd(f, 3);
    const long N = (long)hdr[0]; const int d = (int)hdr[1], q = (int)hdr[2];
    double* X = rd(f, (size_t)N * d); double* Xm = rd(f, (size_t)N * d);
    double* W_mean = rd(f, (size_t)d * q); double* Z = rd(f, (size_t)N * q); double* Z_cov = rd(f, (size_t)q * q);
    double* Mu_mean = rd(f, (size_t)d); double* beta_b = rd(f, 1);
    double* W_pm = rd(f, (size_t)d * q);
    const size_t qd = (size_t)q * d;
    double* a0 = rd(f, qd); double* b0 = rd(f, qd); double* qb0 = rd(f, qd);
    fclose(f);

    double* W_pp = (double*)malloc((size_t)q * d * sizeof(double));
    double* Mu_pm = (double*)calloc((size_t)d, sizeof(double)); double* Mu_pp = (double*)malloc((size_t)d * sizeof(double));
    for (int i = 0; i < q * d; ++i) W_pp[i] = 1.0;
    for (int i = 0; i < d; ++i) Mu_pp[i] = 1e-3;

    pyvb_pca* h = NULL;
    CHECK(pyvb_pca_create(&h, 0, N, d, q, N, 0));
    CHECK(pyvb_pca_set_priors(h, W_pm, W_pp, Mu_pm, Mu_pp, 1e-3, 1e-3));
    CHECK(pyvb_pca_set_data(h, X));
    CHECK(pyvb_pca_set_state(h, Xm, W_mean, Z, Z_cov, Mu_mean, beta_b));
    double* qa = (double*)malloc(qd * sizeof(double));
    double* qb = (double*)malloc(qd * sizeof(double));
    EXPECT(pyvb_pca_get_entry_precisions(h, qa, qb), PYVB_E_ARG);          /* Constant parents so far */
    NAMES("no DiagonalGamma precision parents");
    EXPECT(pyvb_pca_update_entry_precisions(h), PYVB_E_ARG);
    EXPECT(pyvb_pca_set_entry_precisions(h, a0, NULL, qb0), PYVB_E_ARG);
    NAMES("required");
    {
        double* bad = (double*)malloc(qd * sizeof(double));
        memcpy(bad, qb0, qd * sizeof(double));
        bad[qd - 1] = 0.0;
        EXPECT(pyvb_pca_set_entry_precisions(h, a0, b0, bad), PYVB_E_ARG);
        NAMES("qb of entry");
        bad[qd - 1] = NAN;
        EXPECT(pyvb_pca_set_entry_precisions(h, bad, b0, qb0), PYVB_E_ARG);
        NAMES("a0 of entry");
        bad[qd - 1] = INFINITY;
        EXPECT(pyvb_pca_set_entry_precisions(h, a0, bad, qb0), PYVB_E_ARG);
        NAMES("b0 of entry");
        EXPECT(pyvb_pca_get_entry_precisions(h, qa, qb), PYVB_E_ARG);      /* none of them switched the parents on */
        free(bad);
    }
    CHECK(pyvb_pca_set_entry_precisions(h, a0, b0, qb0));
    CHECK(pyvb_pca_get_entry_precisions(h, qa, qb));
    for (size_t e = 0; e < qd; ++e)
        if (qb[e] != qb0[e] || qa[e] != a0[e] + 0.5) { fprintf(stderr, "entry %d: qa %.17g qb %.17g\n", (int)e, qa[e], qb[e]); return 4; }
    /* the two kinds of parent exclude each other: Gamma parents are not what this handle has, and giving them takes these away */
    EXPECT(pyvb_pca_get_column_precisions(h, qa, qb), PYVB_E_ARG);
    EXPECT(pyvb_pca_update_column_precisions(h), PYVB_E_ARG);
    CHECK(pyvb_pca_set_column_precisions(h, a0, b0, qb0));
    EXPECT(pyvb_pca_get_entry_precisions(h, qa, qb), PYVB_E_ARG);
    EXPECT(pyvb_pca_update_entry_precisions(h), PYVB_E_ARG);
    CHECK(pyvb_pca_set_entry_precisions(h, a0, b0, qb0));
    EXPECT(pyvb_pca_get_column_precisions(h, qa, qb), PYVB_E_ARG);
    CHECK(pyvb_pca_iterate(h, niters));
    double parts[5], tot = 0.0;
    CHECK(pyvb_pca_elbo(h, parts));
    for (int p = 0; p < 5; ++p) tot += parts[p];
    printf("lower bound %.17g\n", tot);
    CHECK(pyvb_pca_get_entry_precisions(h, NULL, qb));         /* NULL = skip */
    printf("qb");
    for (size_t e = 0; e < qd; ++e) printf(" %.17g", qb[e]);
    printf("\n");
    /* the explicit entry: the columns have not changed since iterate's own update of the parents, so qb comes out the same */
    double* again = (double*)malloc(qd * sizeof(double));
    CHECK(pyvb_pca_update_entry_precisions(h));
    CHECK(pyvb_pca_get_entry_precisions(h, NULL, again));
    if (memcmp(again, qb, qd * sizeof(double))) { fprintf(stderr, "a second update of the parents changed qb\n"); return 4; }
    /* back to Constant parents */
    CHECK(pyvb_pca_set_priors(h, W_pm, W_pp, Mu_pm, Mu_pp, 1e-3, 1e-3));
    EXPECT(pyvb_pca_get_entry_precisions(h, qa, qb), PYVB_E_ARG);
    CHECK(pyvb_pca_destroy(h));
    printf("done\n");
    return 0;
}
