// What a pyvb_pca handle tracks on the host about what is current on the device (PcaState, with the events that change it), and
// the planner of the next pass over the rows (plan_sweep): a pure function of that state, a handful of handle constants and the
// requested row range.  Standard C++ only: nothing here needs a device, so tests/c/pca_plan_driver.cpp runs it under the host
// sanitizers on call sequences and tests/test_pca_plan_cpu.py holds it against a model of which rows hold unstored entries.
// api_pca.hip writes the state through the events below only; k_pca.hip carries a plan out and assigns nothing.
#pragma once
#include "../../include/pyvb_hip.h"

// What the next pass over the rows is (plan_sweep decides; the launchers of pca.h carry it out).
struct PcaSweepPlan {
    long lo_upd, hi_upd;                 // rows of X to update
    bool with_z;                         // the deferred Z update rides along (k_pca_pass12 / k_pca_pairs); false: k_pca_pass2 alone
    bool keep_z0;                        // z_0 was stored by the X_0 step already
    bool lazy;                           // the imputed entries stay unstored; then the rows [lo_upd, hi_upd) are the new lazy range
    bool pairs;                          // lazy, by k_pca_pairs on its own partition of the rows
    bool materialize;                    // rows [vin_lo, vin_hi) hold unstored entries that this pass cannot take in: store them first
    long vin_lo, vin_hi;                 // the incoming lazy range (empty: none)
    int part_chunks;                     // chunks of partial statistics the pass leaves in `part`
};

// the handle constants the planner reads
struct PcaPlanInput {
    long N;                              // rows of this handle
    int QT;                              // 16-wide tiles of the latent dimension
    int sweep;                           // PYVB_PCA_SWEEP_*
    bool has_xdata;                      // pyvb_pca_set_unpinned_rows has run: rows may still wait for their first update
    int nchunk, nchunkB;                 // the partitions of k_pca_pass2 / k_pca_pass12 and of k_pca_pairs
};

struct PcaState {
    bool full_valid, lin_valid; // stats: every sum current / at least sum x and sum z current.  Dropped by every setter of data or state;
                                // full_valid also by the deferred Z update and the X_0 step, which keep only the linear sums current.
    bool res_valid;             // scal[PS_RES] is the residual of the current W, Z, X, Mu (nothing but Beta updated since)
    bool z_pending;             // [z.update() for z in Zs] has been requested and its operands (Gz, g0, sum z) are set, but the
                                // rows of Z are not written yet: the next pass over X does it on its way (k_pca_pass12)
    bool z0_done;               // while z_pending: Xs[0].update() has run and stored z_0 itself
    bool xlazy; long vlo, vhi;  // the missing entries of rows [vlo, vhi) are not in X: they stand for <W>_x z_n + <Mu>_x
                                // (k_pca_pass12<.., LAZY>, k_pca_pairs); k_pca_materialize puts them there
    int part_chunks;            // chunks of the partial statistics in `part` now (the partition of the sweep that wrote them)

    // Rows [lo, hi) of X are about to be read outside a sweep: true where a lazy sweep left imputed entries of some of them
    // unstored, which are then put into X first (all of [vlo, vhi); x_stored() follows).
    bool needs_store(long lo, long hi) const { return xlazy && lo < vhi && vlo < hi; }

    void inputs_changed() { full_valid = lin_valid = false; res_valid = false; }
    void residual_stale() { res_valid = false; }       // W, Mu or their variances changed
    void beta_updated() { res_valid = true; }          // the residual does not depend on Beta: the lower bound can reuse it
    void z_requested() { z_pending = true; z0_done = false; }
    void z_request_failed() { z_pending = false; }     // the launch that forms the operands failed
    void z_written() { z_pending = false; z0_done = false; }
    void x0_stepped(bool holds_row0) { if (z_pending && holds_row0) z0_done = true; }    // the kernel has stored z_0 from the row as it was
    void linear_step() { full_valid = false; res_valid = false; }      // lin_valid stays: sum x and sum z were kept current
    void x_stored() { xlazy = false; }                 // k_pca_materialize has put the entries of [vlo, vhi) into X
    // The launch of plan p has returned.  The Z update rode along whether or not the launch succeeded (one sweep over X instead
    // of two); the rest holds after a successful launch only.
    void sweep_ran(const PcaSweepPlan& p, bool launched) {
        if (p.with_z) z_written();
        if (!launched) return;
        part_chunks = p.part_chunks;
        if (p.materialize) xlazy = false;
        if (p.lazy) { xlazy = true; vlo = p.lo_upd; vhi = p.hi_upd; }
    }
    // ... and its partial statistics have been reduced (and all-reduced)
    void stats_reduced(const PcaSweepPlan& p) {
        full_valid = lin_valid = true;
        if (p.hi_upd > p.lo_upd) res_valid = false;     // rows changed: the cached residual of the last Beta update is stale
    }
};

// What the next pass over the rows is, for the update of rows [lo_upd, hi_upd) of X: pass 2, or pass 1+2 where a Z update is
// pending.  The standard sweep of an iteration -- all rows, or all but row 0, which the crawl order updates on its own -- leaves
// the imputed entries to be recomputed by the next one (lazy); any other range, latent dimensions beyond 16 (the register budget)
// and rows that still wait for their first update take the write-back, and entries an earlier sweep left unstored that the new
// range does not cover are stored first.
static inline PcaSweepPlan plan_sweep(const PcaState& st, const PcaPlanInput& h, long lo_upd, long hi_upd) {
    PcaSweepPlan p;
    p.lo_upd = lo_upd; p.hi_upd = hi_upd;
    p.with_z = st.z_pending;
    p.keep_z0 = st.z0_done;
    p.lazy = p.with_z && h.sweep != PYVB_PCA_SWEEP_STORE && h.QT == 1 && !h.has_xdata && lo_upd <= 1 && hi_upd == h.N && hi_upd > lo_upd
             && (!st.xlazy || (lo_upd <= st.vlo && st.vhi <= hi_upd));
    p.pairs = p.lazy && h.sweep == PYVB_PCA_SWEEP_PAIRS;
    p.materialize = st.xlazy && !p.lazy;
    p.vin_lo = st.xlazy ? st.vlo : 0; p.vin_hi = st.xlazy ? st.vhi : 0;
    p.part_chunks = p.pairs ? h.nchunkB : h.nchunk;
    return p;
}
