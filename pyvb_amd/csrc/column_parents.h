// The precision parents of the columns of a matrix -- A or C of a pyvb_lds, W of a pyvb_pca -- on the host: which of the three
// kinds is in force, the device block of each kind, and what a setter does before its upload (the finite-and-positive check, the
// staging of what follows from a0 and b0, the broadcast of a model's qb to its chains).  Standard C++ only: nothing here needs a
// device, so tests/c/column_parents_driver.cpp runs it under the host sanitizers (tests/test_column_parents_cpu.py).  api.hip and
// api_pca.hip are the only writers of a record; make_args (k_params.hip) and pca_args (k_pca.hip) read it.  DESIGN.md section 25.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdio>
#include <vector>
#include "../../include/pyvb_hip.h"
#include "digamma.h"
#include "replicates.h"

void pyvb_set_error(const char* fmt, ...);

enum { PARENTS_CONSTANT = PYVB_PARENTS_CONSTANT, PARENTS_GAMMA = PYVB_PARENTS_GAMMA, PARENTS_DIAGONAL_GAMMA = PYVB_PARENTS_DIAGONAL_GAMMA, PARENTS_KINDS };

// The words of a message: the matrix's name; pca: a pyvb_pca's, whose texts name pyvb_pca_* entries and put the entry before the column
struct ParentWords { const char* of; bool pca; };

// One record per matrix.  A matrix has one kind of parent: the most recent successful setter's, Constant after *_set_priors.
// All zero is a matrix with Constant parents and no block.
struct ColumnParents {
    int kind, was;                  // the kind in force: the one place that answers "which kind"; inside a setter: the one to fall back to
    double* block[PARENTS_KINDS];   // device, one per kind ([PARENTS_CONSTANT] stays null): allocated by the first setter of the kind,
                                    // kept when the kind changes, never allocated on a handle that does not ask

    void clear() { kind = PARENTS_CONSTANT; }               // *_set_priors: Constant parents again
    // A setter, once its block is uploaded: `k` is in force for the launch that derives what follows from qb, and stays if that
    // launch was made (rc == 0); a failed one leaves the previous kind in force.  commit returns rc.
    void begin(int k) { was = kind; kind = k; }
    int commit(int rc) { if (rc) kind = was; return rc; }
    double* current() const { return block[kind]; }

    // get / update of parents of kind `want`: PYVB_OK, or the refusal
    int require(int want, ParentWords w) const {
        if (want == PARENTS_GAMMA && kind == PARENTS_DIAGONAL_GAMMA && !w.pca) {
            pyvb_set_error("the columns of %s have DiagonalGamma precision parents, one per entry: pyvb_lds_get_entry_precisions / pyvb_lds_update_entry_precisions serve them", w.of);
            return PYVB_E_ARG;
        }
        if (kind == want) return PYVB_OK;
        if (want == PARENTS_GAMMA)
            pyvb_set_error("the columns of %s have Constant precision parents: no hyperpriors were given (%s_set_column_precisions)", w.of, w.pca ? "pyvb_pca" : "pyvb_lds");
        else if (w.pca)
            pyvb_set_error("the columns of %s have no DiagonalGamma precision parents (pyvb_pca_set_entry_precisions)", w.of);
        else
            pyvb_set_error("the columns of %s have no DiagonalGamma precision parents: no per-entry hyperpriors were given (pyvb_lds_set_entry_precisions)", w.of);
        return PYVB_E_ARG;
    }
};

// The matrices of a pair (A, C) whose parents are of `kind`, as the `which` of one launch: -1 none, 0 the first, 1 the second, 2 both
static inline int parents_of_kind(const ColumnParents p[2], int kind) {
    const bool a = p[0].kind == kind, c = p[1].kind == kind;
    return a && c ? 2 : c ? 1 : a ? 0 : -1;
}

// Every v[e], e < n, is finite and positive, or PYVB_E_ARG with the message naming the place.  rows: entries per column of an array
// [column][row], 0: an array with one value per column.  replicate >= 0: v is that replicate's row of qb.
static inline int check_positive(const double* v, size_t n, size_t rows, const char* what, ParentWords w, int replicate = -1) {
    for (size_t e = 0; e < n; ++e) {
        if (v[e] > 0.0 && v[e] - v[e] == 0.0) continue;
        char rep[32] = "", place[64];
        const int i = (int)(rows ? e / rows : e), k = (int)(rows ? e % rows : 0);
        if (replicate >= 0) snprintf(rep, sizeof(rep), "replicate %d, ", replicate);
        if (!rows) snprintf(place, sizeof(place), "column %d", i);
        else if (w.pca) snprintf(place, sizeof(place), "entry %d of column %d", k, i);
        else snprintf(place, sizeof(place), "column %d, row %d", i, k);
        pyvb_set_error("%s of %s%s of %s is %g: it must be finite and positive", what, rep, place, w.of, v[e]);
        return PYVB_E_ARG;
    }
    return PYVB_OK;
}

// Chains that share A, C, Q, R: the row of a model's first replicate is the model's state and goes to all its rows.  qb [N][per]
// as the caller gave it -> out [N][per]; only the rows of first replicates are read, and checked.
static inline int broadcast_qb(const Replicates& rep, const double* qb, size_t per, size_t rows, ParentWords w, std::vector<double>& out) {
    const size_t N = (size_t)rep.size();
    out.resize(N * per);
    for (size_t n = 0; n < N; ++n) {
        const int first = rep.first_of((int)n);
        const double* src = qb + (size_t)first * per;
        const int rc = check_positive(src, per, rows, "qb", w, first);
        if (rc) return rc;
        for (size_t e = 0; e < per; ++e) out[n * per + e] = src[e];
    }
    return PYVB_OK;
}

// ---- device layouts.  A block of a pyvb_lds starts with what the replicates share, arrays of `per` doubles (Gamma: per = D;
// DiagonalGamma: per = D rows, [column][row]): a0 | b0 | qa, and for DiagonalGamma | ln qa | psi(qa) | cst.  Behind that head, the
// arrays that follow qb (params.h: ColumnPrior), at the offsets below.
struct LdsParentBlock { size_t head, ex, qb, ld_ref, ld_exact, own, total; };      // in doubles; own: DiagonalGamma only
static inline LdsParentBlock lds_parent_block(int kind, size_t N, size_t D, size_t per) {
    const size_t h = (kind == PARENTS_DIAGONAL_GAMMA ? 6 : 3) * per, ND = N * D, Np = N * per;
    if (kind == PARENTS_DIAGONAL_GAMMA) return {h, h, h + Np, h + 2 * Np, h + 2 * Np + ND, h + 2 * Np + 2 * ND, h + 2 * Np + 3 * ND};
    return {h, h, h + 3 * ND, h + ND, h + 2 * ND, 0, h + 4 * ND};       // Gamma: ex | ld_ref | ld_exact | qb
}
// The block of a pyvb_pca with Gamma parents: rows [q] each.  qa_i = a0_i + d / 2 never changes (nodes_todo.py:125-128): lgamma, digamma
// and ln of it are formed on the host, as for Beta.  AR_LN_REF = ln qa - ln qb (nodes_todo.py:147), AR_LN_EXACT = psi(qa) - ln qb follow qb.
enum { AR_A0 = 0, AR_B0, AR_QA, AR_QB, AR_LGAMMA_A0, AR_LGAMMA_QA, AR_DIGAMMA_QA, AR_LN_QA, AR_LN_REF, AR_LN_EXACT, AR_COUNT };
// With DiagonalGamma parents: arrays [q][d] each ([column i][row k], as W_var and W_pp).  qa = a0 + 1/2 never changes (one child per
// entry, nodes_todo.py:183-186), so what of DiagonalGamma.log_lower_bound does not follow qb is one constant per entry, EN_CST (cst
// below), formed on the host; the entry's own term is then EN_CST - a0 ln qb - b0 qa / qb.  Behind the arrays, at EN_COUNT * q * d:
//   ES_OWN    the sum of the own terms over all entries, as of the last PCA_ENTRY
//   ES_EXACT  1/2 sum_ik (psi(qa_ik) - ln qa_ik), what the exact bound has over the per-entry 1/2 ln W_pp (host; never changes)
enum { EN_A0 = 0, EN_B0, EN_QA, EN_QB, EN_CST, EN_COUNT };
enum { ES_OWN = 0, ES_EXACT, EN_SCALARS = 8 };

// ---- staging: everything a setter uploads that follows from a0, b0 (and, on a pyvb_pca, holds qb), n values each.  Gamma parents,
// one child of `rows` entries: qa = a0 + rows / 2 (update_a, nodes_todo.py:125-128).  qb null: the head of a pyvb_lds block,
// a0 | b0 | qa.  qb given: the AR_* rows of a pyvb_pca, whose first three are the same.
static inline void stage_gamma(std::vector<double>& out, const double* a0, const double* b0, size_t n, int rows, const double* qb = nullptr) {
    out.assign((qb ? (size_t)AR_COUNT : 3) * n, 0.0);
    for (size_t i = 0; i < n; ++i) {
        const double qa = a0[i] + 0.5 * rows;
        out[AR_A0 * n + i] = a0[i]; out[AR_B0 * n + i] = b0[i]; out[AR_QA * n + i] = qa;
        if (!qb) continue;
        out[AR_QB * n + i] = qb[i];
        out[AR_LGAMMA_A0 * n + i] = lgamma(a0[i]); out[AR_LGAMMA_QA * n + i] = lgamma(qa);
        out[AR_DIGAMMA_QA * n + i] = digamma_pos(qa); out[AR_LN_QA * n + i] = log(qa);
    }
}
// DiagonalGamma parents, one child per entry: qa = a0 + 1/2 (update_a, nodes_todo.py:183-186), ln qa, psi(qa), and the part of
// log_lower_bound (:199-204) without qb:  cst = (a0 - qa) psi(qa) - lgamma(a0) + a0 ln b0 + lgamma(qa) + qa;  the kernels add
// - a0 ln qb - b0 qa / qb.  qb null: the head of a pyvb_lds block, a0 | b0 | qa | ln qa | psi | cst.  qb given: the EN_* arrays and
// ES_* scalars of a pyvb_pca; ES_EXACT is summed over the entries in ascending order.
static inline void stage_diagonal_gamma(std::vector<double>& out, const double* a0, const double* b0, size_t n, const double* qb = nullptr) {
    out.assign(qb ? EN_COUNT * n + EN_SCALARS : 6 * n, 0.0);
    double exact = 0.0;
    for (size_t e = 0; e < n; ++e) {
        const double qa = a0[e] + 0.5, psi = digamma_pos(qa);
        const double cst = (a0[e] - qa) * psi - lgamma(a0[e]) + a0[e] * log(b0[e]) + lgamma(qa) + qa;
        out[e] = a0[e]; out[n + e] = b0[e]; out[2 * n + e] = qa;
        if (qb) { out[EN_QB * n + e] = qb[e]; out[EN_CST * n + e] = cst; exact += psi - log(qa); }
        else { out[3 * n + e] = log(qa); out[4 * n + e] = psi; out[5 * n + e] = cst; }
    }
    if (qb) out[EN_COUNT * n + ES_EXACT] = 0.5 * exact;
}
