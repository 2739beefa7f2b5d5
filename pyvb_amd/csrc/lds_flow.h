// The control flow of a pyvb_lds: what an update entry launches, decided from LdsState (lds_state.h) and a few facts of the handle,
// and the events it raises.  One copy, over a "device" type Dev that carries out the steps: in api.hip a thin struct over the
// handle whose methods are the launchers of the kernel files, in tests/c/lds_flow_driver.cpp a recorder that writes one line per
// step.  Standard C++ only: nothing here needs a device, so the driver runs this flow -- the one that ships -- under the host
// sanitizers, and tests/test_lds_flow_cpu.py holds every step to a model that does not use the flags.  Argument checks, copies,
// staging buffers, streams, events and the history ring stay in api.hip.  DESIGN.md, "What is current: the host-side state of a
// handle", has the dependency table and the step list of an iteration per class of handle.
//
// Dev has, each returning the status of the launcher it stands for (common.h):
//   prep, wexpect, dense_pre, sweep(direction, src, read_cache, keep_x), step(t), stats(with_sxx), moments(sxx_from_sweep),
//   tie_moments, tie_syy, resid(which), wresid(which, update, use_sg), cols(which, c0, c1, fuse),
//   cols_dense(which, c0, c1), noise(which), parents(kind, which, derive), syy, syy_missing, syy_full, missing_ent_dense(diag_cov),
//   impute, impute_dense, elbo(stream), elbo_dense(), carry_x(src), carry_classes,
// for the known channels of the state equation (side 0: inputs, B) and of the output equation (side 1: regressors, E), k_known.hip:
//   known_gains(side), known_moments(side), known_H(side), known_cols(side), known_resid(side), known_elbo(side, stream)
// and three operations that are not launches:
//   swap_classes()     the pointers Sigma / qld_x / lnd_x change places with their *_new
//   join_elbo()        the main stream waits for a lower bound in flight on the side stream
//   form_lnd_x()       ln det of every class of Sigma on the host, and its two copies
// with main_stream() and a type stream_t for the two calls that take a stream.
// `which` and `side` count alike: 0 is the state equation (A, B, Q), 1 the output equation (C, E, R).
#pragma once
#include <cstddef>
#include "../../include/pyvb_hip.h"
#include "lds_state.h"
#include "replicates.h"
#include "column_parents.h"

void pyvb_set_error(const char* fmt, ...);

// What the flow reads of a handle beside its state, filled from the handle at the call
struct LdsFacts {
    int T, N, D;                    // fixed at creation
    bool dense, big;
    bool has_missing;               // as of this call
    int bound;
    const Replicates* rep;          // host-only records of the handle, read through
    const ColumnParents* parents;   // [2]
    // the known channels of the state equation ([0]) and of the output equation ([1]) (KnownChannels, common.h)
    int width[2];                   // P, Pv: fixed at creation (0: none)
    bool known_set[2], known_priors_set[2];     // as of this call
};

template <class Dev>
struct LdsFlow {
    LdsState& st;
    LdsFacts in;
    Dev dev;

    bool known(int side) const { return in.width[side] > 0; }

    // every replicate switched off: the update entries are successful no-ops without a launch
    bool idle() const { return in.rep->n_active() == 0; }

    // Rows of switched-off replicates sit out the two ping-pongs of the handle: the X buffers (a sweep reads one and writes the
    // other) and the covariance classes (k_prep writes Sigma_new, adopt_classes swaps).  They stay where they were when the row
    // was switched off, and are copied across here, before a getter reads every row, before a setter or a staging copy uses the
    // other X buffer, and before the mask changes -- never on the update path.
    int settle_parked() {
        if (in.rep->n_active() == in.N) return PYVB_OK;
        int rc;
        if (st.x_park != st.cur && (rc = dev.carry_x(st.x_park))) return rc;
        if (st.cls_parked_other && (rc = dev.carry_classes())) return rc;
        st.parked_here();
        return PYVB_OK;
    }

    // sum_t <y^2> per chain, then summed over the chains of every model (k_tie.hip: once per production, it is in place)
    int syy() {
        const int rc = dev.syy();
        return rc ? rc : dev.tie_syy();
    }
    int syy_missing() {
        const int rc = dev.syy_missing();
        return rc ? rc : dev.tie_syy();
    }
    // Wishart noise, after the means of the outputs changed: sum_t qmu qmu^T, and the entropy terms of the rows that are not
    // fully observed (diag_cov: they still carry their diagonal initial covariances, whose sum is formed here too)
    int outputs_changed_dense(int diag_cov) {
        int rc;
        if ((rc = dev.syy_full())) return rc;
        return dev.missing_ent_dense(diag_cov);
    }

    // ---- recomputing what an event dropped (LdsState, lds_state.h; the table is in DESIGN.md) ---------
    int ensure_expect() {        // E[Q], E[R] of the current Wishart posteriors
        if (st.expect_valid) return PYVB_OK;
        int rc = dev.wexpect();
        if (rc) return rc;
        st.expect_valid = true;
        return PYVB_OK;
    }

    // Covariances of the X_t given by pyvb_lds_set_posterior_classes: ln det of each (Cholesky on the host, NaN where one is not
    // positive definite), formed once, when the exact bound or pyvb_lds_get_logdets first needs it -- not on the default path.
    int ensure_lnd_x() {
        if (!st.lnd_x_pending) return PYVB_OK;
        int rc;
        if ((rc = settle_parked())) return rc;       // every row of Sigma is read, every row of lnd_x written
        if ((rc = dev.form_lnd_x())) return rc;
        st.lnd_x_pending = false;
        return PYVB_OK;
    }

    // a handle with known channels before it has them: the updates would read zeros for u_t / v_t and for the parents of B / E
    int known_ready(int side) const {
        static const char* const what[2] = {"inputs", "regressors"};
        static const char* const one[2] = {"input", "regressor"};
        if (!in.known_set[side]) {
            pyvb_set_error("the handle was created with %s: call pyvb_lds_set_%s before the first update", what[side], what[side]);
            return PYVB_E_ARG;
        }
        if (!in.known_priors_set[side]) {
            pyvb_set_error("the handle was created with %s: call pyvb_lds_set_%s_priors before the first update", what[side], one[side]);
            return PYVB_E_ARG;
        }
        return PYVB_OK;
    }

    int ensure_gains() {
        if (st.gains_valid) return PYVB_OK;
        int rc;
        if (in.dense) {
            if ((rc = ensure_expect())) return rc;
            if ((rc = dev.dense_pre())) return rc;
        }
        for (int side = 0; side < 2; ++side)
            if (known(side) && (rc = known_ready(side))) return rc;
        if ((rc = dev.prep())) return rc;
        for (int side = 0; side < 2; ++side)        // the gains of the known channels, from Sigma_1 as k_prep has just left it
            if (known(side) && (rc = dev.known_gains(side))) return rc;
        st.gains_formed();
        return PYVB_OK;
    }

    // The posterior covariance classes that the statistics use are those of the X_t's LAST update; they switch to the freshly
    // prepared ones once every X_t has been updated under the current parameters (LdsState::node_fresh / all_fresh say when).
    void adopt_classes() {
        dev.swap_classes();
        st.classes_adopted(in.rep->n_active() < in.N);
    }

    int ensure_stats() {
        if (st.stats_valid) return PYVB_OK;
        if (!st.classes_valid) {
            // the reference's X_t start with individual random covariances (gaussian.py:70-72); the three-class form the
            // statistics use exists once every X_t has been updated, or once the caller has supplied the classes
            pyvb_set_error("the posterior covariances of the X_t are undefined before the first complete sweep "
                           "(run pyvb_lds_sweep, or give them with pyvb_lds_set_posterior_classes)");
            return PYVB_E_STALE;
        }
        if (st.mixed_cov || (st.gains_valid && st.fresh_count != 0 && st.fresh_count != in.T)) {
            pyvb_set_error("%d of %d X_t were updated since the parameters changed: their covariances differ; sweep all states first",
                           st.fresh_count, in.T);
            return PYVB_E_STALE;
        }
        int rc;
        if (known(1) && (rc = known_ready(1))) return rc;       // before any launch
        if ((rc = dev.stats(!st.sxx_valid))) return rc;
        if ((rc = dev.moments(st.sxx_valid))) return rc;
        if ((rc = dev.tie_moments())) return rc;        // chains that share A, C, Q, R: the moments of a model
        if (known(0) && (rc = known_ready(0))) return rc;       // (the inputs have always been asked for here, behind the launches)
        for (int side = 0; side < 2; ++side)            // Sxu, Su1x / Svx; Sx1x / Syx aside
            if (known(side) && (rc = dev.known_moments(side))) return rc;
        st.stats_valid = true;
        return PYVB_OK;
    }

    int ensure_resid(int which) {
        bool& valid = which == 0 ? st.resQ_valid : st.resR_valid;
        if (valid) return PYVB_OK;
        int rc = ensure_stats();
        if (rc) return rc;
        if (known(which)) {     // H_A / H_C of the current gain, the residual as k_cols forms it, the terms of the gain alone
            if ((rc = dev.known_H(which)) || (rc = dev.resid(which)) || (rc = dev.known_resid(which))) return rc;
        } else if ((rc = in.dense ? dev.wresid(which, 0, st.sg_valid[which]) : dev.resid(which))) return rc;
        valid = true;
        return PYVB_OK;
    }

    int sweep(int direction, bool keep_x) {
        int rc = ensure_gains();
        if (rc) return rc;
        // a backward sweep right behind a forward one reads the c_t that one left in U; the 128-wide class fuses no Sxx
        const bool read_cache = direction == PYVB_BACKWARD && st.u_valid;
        if ((rc = dev.sweep(direction, st.cur, read_cache, keep_x))) return rc;
        st.sweep_ran(direction, read_cache, !in.big);
        if (st.all_fresh()) adopt_classes();
        return PYVB_OK;
    }

    // ---- the update entries, behind ENTER and the argument checks of api.hip
    int update_sweep(int direction) { return idle() ? PYVB_OK : sweep(direction, true); }

    int update_x(int t) {
        if (idle()) return PYVB_OK;
        int rc = ensure_gains();
        if (rc) return rc;
        if ((rc = dev.step(t))) return rc;
        st.x_changed();
        if (st.node_fresh(t)) adopt_classes();
        return PYVB_OK;
    }

    int update_columns(int which, int col_begin, int col_end) {
        if (idle()) return PYVB_OK;
        int rc = ensure_stats();
        if (rc) return rc;
        if (in.dense) {
            if ((rc = ensure_expect())) return rc;
            if ((rc = dev.cols_dense(which, col_begin, col_end))) return rc;
        } else {
            if (known(which) && (rc = dev.known_H(which))) return rc;       // H = Sx1x - <B> Su1x / Syx - <E> Svx
            if ((rc = dev.cols(which, col_begin, col_end))) return rc;
        }
        st.columns_updated(which, in.dense && col_begin == 0 && col_end == in.D);
        return PYVB_OK;
    }

    // the columns of B (side 0) / E (side 1)
    int update_gain(int side) {
        if (idle()) return PYVB_OK;
        int rc;
        if ((rc = ensure_stats()) || (rc = dev.known_cols(side))) return rc;
        st.columns_updated(side, false);        // as a column of A / C: the gains and the residual of Q / R depend on it
        return PYVB_OK;
    }

    int update_parents(int which, int kind) { return idle() ? PYVB_OK : dev.parents(kind, which, false); }

    int update_noise(int which) {
        if (idle()) return PYVB_OK;
        int rc;
        if (in.dense) {     // Wishart.update: the residual matrix and qw = w0 + it in one launch
            if ((rc = ensure_stats())) return rc;
            if ((rc = dev.wresid(which, 1, st.sg_valid[which]))) return rc;
        } else {
            if ((rc = ensure_resid(which))) return rc;
            if ((rc = dev.noise(which))) return rc;
        }
        st.noise_updated(which);
        return PYVB_OK;
    }

    int update_Y() {
        if (!in.has_missing) return PYVB_OK;            // observed nodes never update (gaussian.py:109-110)
        if (idle()) return PYVB_OK;
        int rc;
        if (in.dense) {
            if ((rc = ensure_expect())) return rc;     // E[R] and its log-determinant
            if ((rc = dev.impute_dense())) return rc;
            if ((rc = outputs_changed_dense(0))) return rc;
        } else {
            if ((rc = dev.impute())) return rc;
            if ((rc = syy_missing())) return rc;
        }
        st.outputs_changed();
        return PYVB_OK;
    }

    // k_elbo, and behind it the columns of B into part 2 on a handle with inputs, those of E into part 3 with regressors
    int lds_bound(typename Dev::stream_t stream) {
        int rc = dev.elbo(stream);
        for (int side = 0; side < 2; ++side)
            if (!rc && known(side)) rc = dev.known_elbo(side, stream);
        return rc;
    }

    int elbo() {
        if (idle()) return PYVB_OK;
        int rc;
        if ((rc = ensure_resid(0))) return rc;
        if ((rc = ensure_resid(1))) return rc;
        if (in.bound == PYVB_BOUND_EXACT && (rc = ensure_lnd_x())) return rc;
        if (in.dense) {
            if ((rc = ensure_expect())) return rc;
            return dev.elbo_dense();
        }
        return lds_bound(dev.main_stream());
    }

    // The updates of one iteration: forward sweep, backward sweep, A, C, Q, R (the example's loop body, Linear_Dynamic_System.py:70-79)
    int iterate_updates() {
        int rc;
        // the backward sweep follows at once and reads c_t, not the forward states: those are not written out
        if ((rc = sweep(PYVB_FORWARD, false))) return rc;
        if ((rc = dev.join_elbo())) return rc;
        if ((rc = sweep(PYVB_BACKWARD, true))) return rc;
        // A and C are independent given the statistics, and so are Q and R given A and C: the pairs
        // share launches here (same arithmetic as update_A, update_C, update_Q, update_R in turn)
        if ((rc = ensure_stats())) return rc;
        if (in.dense) {
            if ((rc = ensure_expect())) return rc;
            if ((rc = dev.cols_dense(2, 0, in.D))) return rc;
            st.columns_updated(2, true);
            if ((rc = dev.wresid(2, 1, true))) return rc;    // both residual matrices and both qw = w0 + residual
            st.noise_updated(2);
            if ((rc = ensure_expect())) return rc;                // E[Q], E[R] of the new posteriors: the bound and the next k_prep read them
        } else if (!known(0) && !known(1)) {
            if ((rc = dev.cols(2, 0, in.D, 3))) return rc;       // columns, residuals and noise update in one launch
            st.columns_updated(2, false);
            st.noise_updated(2);
            // [al.update() for al in alphas]: they read their own column and feed the next column update only, so they commute with Q
            // and R.  They sit behind the join_elbo above like k_cols: the bound of the iteration before reads qb and qa / qb.
            // Then [dg.update() for dg in ...]: the DiagonalGamma parents of the matrices that have those instead, in the same place.
            for (int kind = PARENTS_GAMMA; kind <= PARENTS_DIAGONAL_GAMMA; ++kind) {
                const int which = parents_of_kind(in.parents, kind);     // both matrices of a kind: one launch
                if (which >= 0 && (rc = dev.parents(kind, which, false))) return rc;
            }
        } else {
            // As, [Bs], Cs, [Es], Q, R.  The gain of an equation sees the new matrix beside it and the noise sees both, so an equation
            // with known channels takes its steps one by one; one without keeps its columns, residual and noise in one launch.
            for (int which = 0; which < 2; ++which) {
                if (!known(which)) { if ((rc = dev.cols(which, 0, in.D, 3))) return rc; }
                else if ((rc = dev.known_H(which)) || (rc = dev.cols(which, 0, in.D)) || (rc = dev.known_cols(which))) return rc;
            }
            st.columns_updated(2, false);
            for (int which = 0; which < 2; ++which)
                if (!known(which)) st.noise_updated(which);
            for (int which = 0; which < 2; ++which)
                if (known(which)) {
                    if ((rc = ensure_resid(which)) || (rc = dev.noise(which))) return rc;
                    st.noise_updated(which);
                }
        }
        if (in.bound == PYVB_BOUND_EXACT && (rc = ensure_lnd_x())) return rc;       // (only before the first complete sweep)
        return PYVB_OK;
    }

    // ---- setters end in events on the state; where the choice of event is more than one line, it is here.
    // pyvb_lds_set_state: x: states given; covs: Wishart, and column variances given (diagonal initial covariances); parameters:
    // any posterior mean, variance or rate given
    void state_given(bool x, bool covs, bool parameters) {
        if (x) st.x_changed();
        if (covs) st.columns_changed();
        else if (parameters) st.parameters_changed();
    }
};
