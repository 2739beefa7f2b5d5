// What replicate n of a pyvb_lds handle is, on the host: the length of its chain, the model it belongs to, whether the caller
// has switched it off and whether the stopping test has frozen it -- with the rules that govern those four (ids start at 0
// and rise by 0 or 1; the mask only shrinks and never splits a model; a replicate runs while it is switched on and not
// converged).  Standard C++ only: nothing here needs a device, so tests/c/replicates_driver.cpp runs it under the host
// sanitizers and tests/test_replicates_cpu.py compares it with numpy.  api.hip is the only writer.
#pragma once
#include <cstddef>
#include <vector>
#include "../../include/pyvb_hip.h"

void pyvb_set_error(const char* fmt, ...);

struct Replicates {
    // ---- validation of what a *_create entry is given (before any HIP call): PYVB_OK or the status, with the message set
    static int check_models(int N, const int* model, bool* tied) {
        *tied = false;
        for (int n = 0; n < N; ++n) {
            const int prev = n ? model[n - 1] : 0;
            if (n == 0 ? model[0] != 0 : (model[n] != prev && model[n] != prev + 1)) {
                pyvb_set_error("replicate %d has model %d after %d: model ids start at 0, never decrease and rise in steps of 0 or 1 "
                               "(a model is a run of consecutive replicates)", n, model[n], n ? prev : -1);
                return PYVB_E_ARG;
            }
            *tied = *tied || (n && model[n] == prev);
        }
        return PYVB_OK;
    }
    static int check_lengths(int N, int T, const int* lengths, bool* ragged) {
        *ragged = false;
        for (int n = 0; n < N; ++n) {
            if (lengths[n] < 2 || lengths[n] > T) {
                pyvb_set_error("replicate %d has length %d: every chain needs 2 <= T_n <= T = %d", n, lengths[n], T);
                return PYVB_E_ARG;
            }
            *ragged = *ragged || lengths[n] != T;
        }
        return PYVB_OK;
    }

    // checked arguments; lengths null: every chain has T nodes, model null: every replicate is a model.  All switched on.
    void init(int N_, int T_, const int* lengths, const int* model) {
        N = N_; T = T_;
        len.clear(); mod.clear(); mstart.clear(); first.clear();
        if (lengths) len.assign(lengths, lengths + N);
        if (model) {
            mod.assign(model, model + N);
            mstart.assign((size_t)model[N - 1] + 2, N);
            first.assign((size_t)N, 0);
            for (int n = N - 1; n >= 0; --n) mstart[model[n]] = n;
            for (int m = 0; m < M(); ++m) first[mstart[m]] = 1;
        }
        on.assign((size_t)N, 1);
        conv.assign((size_t)N, 0);
        recount();
    }

    // ---- queries
    bool ragged() const { return !len.empty(); }
    bool tied() const { return !mod.empty(); }
    int M() const { return tied() ? (int)mstart.size() - 1 : N; }
    int length(int n) const { return ragged() ? len[n] : T; }
    int model(int n) const { return tied() ? mod[n] : n; }
    int first_of(int n) const { return tied() ? mstart[mod[n]] : n; }      // the first replicate of n's model
    // the children of replicate n's Q (the X_1.. of a chain) and R (its Y_t), summed over the chains of its model
    void children(std::vector<long>& nq, std::vector<long>& nr) const {
        std::vector<long> mq((size_t)M(), 0), mr((size_t)M(), 0);
        for (int n = 0; n < N; ++n) { mq[model(n)] += length(n) - 1; mr[model(n)] += length(n); }
        nq.resize((size_t)N); nr.resize((size_t)N);
        for (int n = 0; n < N; ++n) { nq[n] = mq[model(n)]; nr[n] = mr[model(n)]; }
    }

    // ---- masks
    bool active(int n) const { return on[n] != 0; }
    const unsigned char* caller_mask() const { return on.data(); }      // [N] bytes 0 / 1: what the totals count
    int n_active() const { return running; }                              // replicates the update kernels run
    std::vector<unsigned char> run_mask() const {                         // switched on and not converged
        std::vector<unsigned char> run((size_t)N);
        for (int n = 0; n < N; ++n) run[n] = on[n] && !conv[n];
        return run;
    }
    // what pyvb_lds_set_active checks before it touches anything
    int check_mask(const unsigned char* active) const {
        for (int n = 0; n < N; ++n)
            if (active[n] && !on[n]) {
                pyvb_set_error("replicate %d is switched off and cannot be switched on again: the mask can only shrink "
                               "(the validity tracking of gains and statistics is per handle)", n);
                return PYVB_E_ARG;
            }
        for (int n = 1; tied() && n < N; ++n)
            if (mod[n] == mod[n - 1] && (active[n] != 0) != (active[n - 1] != 0)) {
                pyvb_set_error("the mask switches off part of model %d (replicate %d is %s, replicate %d is %s): the chains of a model "
                               "share A, C, Q, R and are switched off together", mod[n], n - 1, active[n - 1] ? "on" : "off",
                               n, active[n] ? "on" : "off");
                return PYVB_E_ARG;
            }
        return PYVB_OK;
    }
    bool mask_differs(const unsigned char* active) const {
        for (int n = 0; n < N; ++n)
            if ((active[n] != 0) != (on[n] != 0)) return true;
        return false;
    }
    void adopt_mask(const unsigned char* active) {                        // a checked mask
        for (int n = 0; n < N; ++n) on[n] = active[n] ? 1 : 0;
        recount();
    }
    void adopt_conv(const unsigned char* converged) {                     // the device's conv bytes after pyvb_lds_iterate_until
        conv.assign(converged, converged + N);
        recount();
    }

    // the two arrays a tied handle uploads; empty on a handle whose models are single replicates
    const std::vector<int>& model_starts() const { return mstart; }            // [M + 1]: model m is replicates mstart[m] .. mstart[m + 1] - 1
    const std::vector<unsigned char>& first_flags() const { return first; }    // [N]: 1 = the first replicate of its model
    int size() const { return N; }

private:
    void recount() {
        running = 0;
        for (int n = 0; n < N; ++n) running += on[n] && !conv[n];
    }
    int N = 0, T = 0;
    std::vector<int> len;                   // [N] T_n; empty on a handle whose chains all have T nodes
    std::vector<int> mod;                   // [N] model ids; empty on a handle whose models are single replicates
    std::vector<int> mstart;
    std::vector<unsigned char> first;
    std::vector<unsigned char> on, conv;    // [N] the caller's mask; [N] 1 = converged, frozen for the life of the handle
    int running = 0;
};
