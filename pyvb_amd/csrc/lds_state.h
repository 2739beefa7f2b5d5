// What a pyvb_lds tracks on the host about what is current on the device, with the events that change it.  Standard C++ only:
// nothing here needs a device, so tests/c/lds_flow_driver.cpp runs it, under the flow that reads and writes it (lds_flow.h), with
// the host sanitizers (tests/test_lds_flow_cpu.py).  host.h includes it; kernel files read the state, only the flow and the
// setters of api.hip (through the events) write it.  DESIGN.md, "What is current: the host-side state of a handle", has the
// dependency table.
#pragma once
#include <cstring>
#include "../../include/pyvb_hip.h"

// ---- pyvb_lds: what is current ---------------------------------------------------------------------------------------------
// One field per derived buffer (or per property of the states), each with what it describes and which events drop it; the
// ensure_* helpers of lds_flow.h recompute a buffer and set its field.  Every entry point of api.hip ends in one or more events.
struct LdsState {
    int T;
    int cur;                    // X[cur] holds the states; a sweep reads it and writes the other (sweep_ran flips)
    bool gains_valid;           // gains, Sigma_new / qld_x_new / lnd_x_new (k_prep; Wishart: QA, RC, trA, trC) belong to the current
                                // parameter posteriors.  Dropped by every event that changes a parameter (params_touched).
    bool expect_valid;          // Wishart: Qbar, Rbar, lnd belong to the current Q_w, R_w, qv.  Dropped by noise_changed, noise_updated.
    bool stats_valid;           // stats, mom are sums over the current states and outputs.  Dropped by x_changed, outputs_changed,
                                // sweep_ran, classes_set (the moments hold the covariance classes).
    bool resQ_valid, resR_valid;    // resQ / resR (Wishart: RQ / RR) belong to the statistics AND the columns of A / C.  Dropped with
                                // stats_valid, and by parameters_changed, columns_changed, columns_updated (of that matrix).
    bool sg_valid[2];           // Wishart: SG[0 / 1] sums every column covariance of A / C as it is now, weighted with the current
                                // statistics.  Set by columns_updated over all columns; dropped with stats_valid, by a partial
                                // columns_updated and by columns_changed.  Never set for the Gamma kinds (nothing reads it there).
    bool u_valid;               // U holds c_t = F mu_{t-1} + G y_t of the current gains, outputs and of X as the last forward sweep left
                                // it: the backward sweep right behind reads it.  Set by a forward sweep_ran, dropped by everything else
                                // that changes gains, outputs or states.
    bool sxx_valid;             // sxx is the interior sum of mu mu^T of the current states (written by a backward sweep that read U; not
                                // in the 128-wide class).  Dropped by x_changed and by every other sweep_ran.
    unsigned char* fresh;       // [T] X_t updated since gains were last formed; fresh_count of them.  All of them: the classes of
    int fresh_count;            // Sigma_new describe every X_t and are adopted (lds_flow.h: adopt_classes).  Reset by gains_formed.
    bool mixed_cov;             // the X_t hold covariances of different parameter generations: a parameter changed while only some were
                                // fresh.  Cleared when all are fresh again.
    bool classes_valid;         // Sigma / qld_x describe the X_t (after the first complete sweep, or classes_set)
    bool lnd_x_pending;         // Sigma came from the caller (classes_set): lnd_x is formed from it when first needed (ensure_lnd_x)
    int x_park;                 // the X buffer that holds the rows of the switched-off replicates (they sit out the ping-pong)
    bool cls_parked_other;      // their Sigma / qld_x / lnd_x are in the *_new set (adopt_classes swapped since)

    // -- the events.  Shared parts first.
    void params_touched() {
        if (gains_valid && fresh_count != 0 && fresh_count != T) mixed_cov = true;
        gains_valid = false;
        u_valid = false;
    }
    void sums_stale() { stats_valid = false; resQ_valid = resR_valid = false; sg_valid[0] = sg_valid[1] = false; }

    // Priors, known entries, or posterior means / variances / rates given by the caller.  (pyvb_lds_set_priors used to drop sg_valid
    // too, for the Gamma kinds only, where the field is never set: no difference.  SG does not depend on priors.)
    void parameters_changed() { params_touched(); resQ_valid = resR_valid = false; }
    // the same, where the column covariances themselves were replaced (Wishart: set_column_cov, set_state with variances,
    // set_column_observations, which zeroes those of known columns; for the Gamma kinds sg_valid is false already)
    void columns_changed() { parameters_changed(); sg_valid[0] = sg_valid[1] = false; }
    // Q_w / R_w / qv given by the caller.  The residual matrices RQ, RR are sums over states and columns only and stay;
    // pyvb_lds_set_wishart_priors, which also changes w0 (added to them by the update), raises parameters_changed beside this.
    void noise_changed() { expect_valid = false; params_touched(); }
    // Q / R (which: 0, 1, 2 = both) updated by a launch that also left their residuals current
    void noise_updated(int which) {
        if (which != 1) resQ_valid = true;
        if (which != 0) resR_valid = true;
        noise_changed();
    }
    // columns [c0, c1) of A / C / both updated from the current statistics; sums_all: Wishart, and every column went through
    void columns_updated(int which, bool sums_all) {
        if (which != 1) { sg_valid[0] = sums_all; resQ_valid = false; }
        if (which != 0) { sg_valid[1] = sums_all; resR_valid = false; }
        params_touched();
    }
    void outputs_changed() { u_valid = false; sums_stale(); }           // Y replaced or imputed
    void x_changed() { u_valid = false; sxx_valid = false; sums_stale(); }      // states replaced or one updated; also a new time split,
                                                                                // which re-shapes sxx and the parts U was written for
    void classes_set() { lnd_x_pending = true; classes_valid = true; sums_stale(); }
    void gains_formed() { gains_valid = true; memset(fresh, 0, T); fresh_count = 0; }
    // X_t / every X_t updated under the current gains.  True: all are fresh now and the caller adopts the new classes.
    bool node_fresh(int t) {
        if (fresh[t]) return false;
        fresh[t] = 1;
        if (++fresh_count < T) return false;
        mixed_cov = false;
        return true;
    }
    bool all_fresh() {
        const bool adopt = fresh_count < T;     // Sigma_new holds the classes of the current parameters exactly when some node is not fresh yet
        if (adopt) { memset(fresh, 1, T); fresh_count = T; }
        mixed_cov = false;
        return adopt;
    }
    // a sweep wrote X[1 - cur]; read_cache: it was the backward kernel that reads U; fused_sxx: that kernel also writes sxx
    void sweep_ran(int direction, bool read_cache, bool fused_sxx) {
        cur = 1 - cur;
        sxx_valid = read_cache && fused_sxx;
        u_valid = direction == PYVB_FORWARD;
        sums_stale();
    }
    void classes_adopted(bool some_parked) {
        lnd_x_pending = false;
        classes_valid = true;
        if (some_parked) cls_parked_other = !cls_parked_other;      // the parked rows did not move with the pointers
    }
    void parked_here() { x_park = cur; cls_parked_other = false; }      // settled, or the mask changed: parked rows are in the current buffers
};
