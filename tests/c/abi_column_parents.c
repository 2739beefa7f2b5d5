/* A host program in plain C for the two read-only entries of include/pyvb_hip.h that say which kind of precision parent the columns
 * of a matrix have: pyvb_lds_get_column_parents, pyvb_pca_get_column_parents.  Builds like tests/c/abi_entry.c.  Without an argument
 * it checks what needs no device; with one it walks a small handle of each path through the kinds and reads the kind after every
 * step (tests/test_column_parents_c_abi_gpu.py). */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "pyvb_hip.h"

#define CHECK(call) do { int rc_ = (call); if (rc_ != PYVB_OK) { fprintf(stderr, "%s failed: %d %s\n", #call, rc_, pyvb_last_error()); return 1; } } while (0)
#define EXPECT(call, want) do { int rc_ = (call); if (rc_ != (want)) { fprintf(stderr, "%s gave %d, expected %d (%s)\n", #call, rc_, (want), pyvb_last_error()); return 1; } } while (0)
#define NAMES(what) do { if (!strstr(pyvb_last_error(), what)) { fprintf(stderr, "the message does not name %s: %s\n", what, pyvb_last_error()); return 4; } } while (0)
#define KINDS(a, c) do { int k_[2] = {-1, -1}; CHECK(pyvb_lds_get_column_parents(h, k_)); \
    if (k_[0] != (a) || k_[1] != (c)) { fprintf(stderr, "line %d: kinds %d %d, expected %d %d\n", __LINE__, k_[0], k_[1], (a), (c)); return 4; } } while (0)
#define KIND(w) do { int k_ = -1; CHECK(pyvb_pca_get_column_parents(p, &k_)); \
    if (k_ != (w)) { fprintf(stderr, "line %d: kind %d, expected %d\n", __LINE__, k_, (w)); return 4; } } while (0)

enum { N = 2, T = 3, D = 2, K = 3, d = 3, q = 2 };

int main(int argc, char** argv) {
    int kind[2];
    EXPECT(pyvb_lds_get_column_parents(NULL, kind), PYVB_E_ARG);
    NAMES("handle is NULL");
    EXPECT(pyvb_pca_get_column_parents(NULL, kind), PYVB_E_ARG);
    NAMES("handle is NULL");
    if (PYVB_PARENTS_CONSTANT != 0 || PYVB_PARENTS_GAMMA != 1 || PYVB_PARENTS_DIAGONAL_GAMMA != 2) return 4;
    if (argc < 2) { printf("argument checks ok\n"); return 0; }

    double ones[N * D * K], zeros[N * D * K], eye[D * D] = {1.0, 0.0, 0.0, 1.0}, bad[N * D * K];
    for (int i = 0; i < N * D * K; ++i) { ones[i] = 1.0; zeros[i] = 0.0; bad[i] = 1.0; }
    bad[0] = NAN;

    pyvb_lds* h = NULL;
    CHECK(pyvb_lds_create(&h, 0, N, T, D, K, PYVB_NOISE_DIAGONAL_GAMMA));
    EXPECT(pyvb_lds_get_column_parents(h, NULL), PYVB_E_ARG);
    NAMES("kind is NULL");
    KINDS(PYVB_PARENTS_CONSTANT, PYVB_PARENTS_CONSTANT);
    CHECK(pyvb_lds_set_priors(h, zeros, eye, zeros, ones, zeros, ones, ones, ones, ones, ones));
    CHECK(pyvb_lds_set_column_precisions(h, 0, ones, ones, ones));
    KINDS(PYVB_PARENTS_GAMMA, PYVB_PARENTS_CONSTANT);
    CHECK(pyvb_lds_set_entry_precisions(h, 1, ones, ones, ones));
    KINDS(PYVB_PARENTS_GAMMA, PYVB_PARENTS_DIAGONAL_GAMMA);
    EXPECT(pyvb_lds_set_entry_precisions(h, 0, ones, bad, ones), PYVB_E_ARG);       /* a refused setter changes nothing */
    NAMES("b0 of column 0, row 0 of A");
    KINDS(PYVB_PARENTS_GAMMA, PYVB_PARENTS_DIAGONAL_GAMMA);
    CHECK(pyvb_lds_set_entry_precisions(h, 0, ones, ones, ones));
    KINDS(PYVB_PARENTS_DIAGONAL_GAMMA, PYVB_PARENTS_DIAGONAL_GAMMA);
    CHECK(pyvb_lds_set_column_precisions(h, 1, ones, ones, ones));
    KINDS(PYVB_PARENTS_DIAGONAL_GAMMA, PYVB_PARENTS_GAMMA);
    CHECK(pyvb_lds_set_priors(h, zeros, eye, zeros, ones, zeros, ones, ones, ones, ones, ones));
    KINDS(PYVB_PARENTS_CONSTANT, PYVB_PARENTS_CONSTANT);
    CHECK(pyvb_lds_destroy(h));

    pyvb_pca* p = NULL;
    CHECK(pyvb_pca_create(&p, 0, N, d, q, N, 0));
    EXPECT(pyvb_pca_get_column_parents(p, NULL), PYVB_E_ARG);
    KIND(PYVB_PARENTS_CONSTANT);
    CHECK(pyvb_pca_set_priors(p, zeros, ones, zeros, ones, 1e-3, 1e-3));
    CHECK(pyvb_pca_set_entry_precisions(p, ones, ones, ones));
    KIND(PYVB_PARENTS_DIAGONAL_GAMMA);
    EXPECT(pyvb_pca_set_column_precisions(p, ones, ones, bad), PYVB_E_ARG);
    NAMES("qb of column 0 of W");
    KIND(PYVB_PARENTS_DIAGONAL_GAMMA);
    CHECK(pyvb_pca_set_column_precisions(p, ones, ones, ones));
    KIND(PYVB_PARENTS_GAMMA);
    CHECK(pyvb_pca_set_priors(p, zeros, ones, zeros, ones, 1e-3, 1e-3));
    KIND(PYVB_PARENTS_CONSTANT);
    CHECK(pyvb_pca_destroy(p));
    printf("done\n");
    return 0;
}
