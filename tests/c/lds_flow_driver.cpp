// Runs the update flow of a pyvb_lds handle (pyvb_amd/csrc/lds_flow.h over LdsState of lds_state.h) on a file of call sequences, for
// tests/test_lds_flow_cpu.py and tests/test_lds_flow_regressors_cpu.py, which build it with the address and undefined-behaviour sanitizers.  LdsFlow is instantiated here
// itself, the header that ships, over a device that writes one line per step in place of a launch.  What api.hip keeps -- the
// copies and the staging of getters and setters, the loops of pyvb_lds_iterate / iterate_until, the change of mask -- is a line of
// output each ("copy", "stage", "mask", "bound", "converge"), behind the settle_parked or the event api.hip has there.  No checks
// of its own: the test reads the output.
//   init T N D P dense big [Pv]         a new handle, as pyvb_lds_create leaves it (Pv: 0 unless given)
//   sweep dir | x t | cols which c0 c1 | B | E | parents which kind | Q | R | Y | elbo       the update entries
//   iterate n | until n conv...         pyvb_lds_iterate(n); pyvb_lds_iterate_until that ran n iterations and left the N conv bytes
//   priors | wishart_priors | wishart_state | column_cov | column_obs | observations missing | output_state | inputs |
//   input_priors | input_state | regressors | regressor_priors | regressor_state | state x covs parameters | classes | time_split | set_parents which kind       the setters' events
//   get_state | get_classes | get_logdets | active m...  | bound mode
// Output: "> command", the steps of the call -- the names of LdsDevice in api.hip with their arguments, streams as 0 (main) and
// 1 (side) --, "! status message" where the call failed, and the state after it:
//   "= cur gains expect stats resQ resR sg0 sg1 u sxx fresh_count mixed classes lnd_x_pending x_park cls_parked_other"
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>
#include "lds_flow.h"

static char g_err[512] = "";
void pyvb_set_error(const char* fmt, ...) {
    va_list ap; va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

struct Recorder {
    typedef int stream_t;
    FILE* out;
    int say(const char* fmt, ...) {
        va_list ap; va_start(ap, fmt);
        vfprintf(out, fmt, ap);
        va_end(ap);
        fputc('\n', out);
        return PYVB_OK;
    }
    int main_stream() const { return 0; }
    int prep() { return say("prep"); }
    int wexpect() { return say("wexpect"); }
    int dense_pre() { return say("dense_pre"); }
    int sweep(int direction, int src, bool read_cache, bool keep_x) { return say("sweep %d %d %d %d", direction, src, (int)read_cache, (int)keep_x); }
    int step(int t) { return say("step %d", t); }
    int stats(bool with_sxx) { return say("stats %d", (int)with_sxx); }
    int moments(bool sxx_from_sweep) { return say("moments %d", (int)sxx_from_sweep); }
    int tie_moments() { return say("tie moments"); }
    int tie_syy() { return say("tie syy"); }
    // the steps of the known channels under the names they have per side: in_* for the inputs (0), rg_* for the regressors (1)
    int known_gains(int side) { return say(side ? "rg_gains" : "in_gains"); }
    int known_moments(int side) { return say(side ? "rg_moments" : "in_moments"); }
    int known_H(int side) { return say(side ? "rg_HC" : "in_HA"); }
    int known_cols(int side) { return say(side ? "rg_colsE" : "in_colsB"); }
    int known_resid(int side) { return say(side ? "rg_resR" : "in_resQ"); }
    int known_elbo(int side, int stream) { return say("%s_elbo %d", side ? "rg" : "in", stream); }
    int resid(int which) { return say("resid %d", which); }
    int wresid(int which, int update, bool use_sg) { return say("wresid %d %d %d", which, update, (int)use_sg); }
    int cols(int which, int c0, int c1, int fuse = 0) { return say("cols %d %d %d %d", which, c0, c1, fuse); }
    int cols_dense(int which, int c0, int c1) { return say("cols_dense %d %d %d", which, c0, c1); }
    int noise(int which) { return say("noise %d", which); }
    int parents(int kind, int which, bool derive) { return say("parents %d %d %d", kind, which, (int)derive); }
    int syy() { return say("syy"); }
    int syy_missing() { return say("syy_missing"); }
    int syy_full() { return say("syy_full"); }
    int missing_ent_dense(int diag_cov) { return say("missing_ent_dense %d", diag_cov); }
    int impute() { return say("impute"); }
    int impute_dense() { return say("impute_dense"); }
    int elbo(int stream) { return say("elbo %d", stream); }
    int elbo_dense() { return say("elbo_dense 0"); }
    int carry_x(int src) { return say("carry x %d", src); }
    int carry_classes() { return say("carry classes"); }
    void swap_classes() { say("swap_classes"); }
    int join_elbo() { return say("join_elbo"); }
    int form_lnd_x() { return say("form_lnd_x"); }
};

struct Handle {
    LdsState st;
    LdsFacts facts;
    Replicates rep;
    ColumnParents parents[2];
    std::vector<unsigned char> fresh;
    FILE* out;

    LdsFlow<Recorder> flow() {
        facts.rep = &rep; facts.parents = parents;
        return {st, facts, {out}};
    }
    void init(int T, int N, int D, int P, bool dense, bool big, int Pv) {
        st = LdsState();            // as in a value-initialised handle
        fresh.assign((size_t)T, 0);
        st.T = T; st.fresh = fresh.data();
        facts = LdsFacts();
        facts.T = T; facts.N = N; facts.D = D; facts.width[0] = P; facts.width[1] = Pv; facts.dense = dense; facts.big = big;
        facts.bound = PYVB_BOUND_REFERENCE;
        rep.init(N, T, nullptr, nullptr);
        parents[0] = parents[1] = ColumnParents();
    }
    // the bound of an iteration, as pyvb_lds_iterate (side stream) and iterate_until (main stream) launch it
    int bound(LdsFlow<Recorder>& f, int stream) {
        if (facts.dense) { fprintf(out, "elbo_dense %d\n", stream); return PYVB_OK; }
        return f.lds_bound(stream);
    }
    int iterate(int n) {
        LdsFlow<Recorder> f = flow();
        const bool idle = f.idle();
        int rc;
        for (int it = 0; it < n; ++it) {
            if ((rc = idle ? f.dev.join_elbo() : f.iterate_updates())) return rc;
            if (!idle && (rc = bound(f, 1))) return rc;
        }
        return PYVB_OK;
    }
    int until(int n, const std::vector<unsigned char>& conv) {
        LdsFlow<Recorder> f = flow();
        const bool idle = f.idle();
        int rc;
        for (int it = 0; it < n && !idle; ++it) {
            if ((rc = f.iterate_updates()) || (rc = bound(f, 0))) return rc;
            fputs("converge\n", out);
        }
        rep.adopt_conv(conv.data());
        return PYVB_OK;
    }
    int set_active(const std::vector<unsigned char>& m) {
        int rc = rep.check_mask(m.data());
        if (rc) return rc;
        if (!rep.mask_differs(m.data())) return PYVB_OK;
        if ((rc = flow().settle_parked())) return rc;
        rep.adopt_mask(m.data());
        st.parked_here();
        fputs("mask\n", out);
        return PYVB_OK;
    }
    // a getter of every row, or a setter that stages through the other X buffer: settle, then the copy
    int settled(const char* what) {
        const int rc = flow().settle_parked();
        if (rc == PYVB_OK) fprintf(out, "%s\n", what);
        return rc;
    }
};

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    std::ifstream in(argv[1]);
    FILE* out = fopen(argv[2], "w");
    if (!in || !out) return 2;
    Handle h;
    h.out = out;
    h.init(2, 1, 1, 0, false, false, 0);
    std::string line, cmd;
    while (std::getline(in, line)) {
        std::istringstream ls(line);
        ls >> cmd;
        fprintf(out, "> %s\n", line.c_str());
        int rc = PYVB_OK, a = 0, b = 0, c = 0;
        g_err[0] = 0;
        if (cmd == "init") { int T, N, D, P, dense, big, Pv = 0; ls >> T >> N >> D >> P >> dense >> big; ls >> Pv; h.init(T, N, D, P, dense != 0, big != 0, Pv); }
        else if (cmd == "sweep") { ls >> a; rc = h.flow().update_sweep(a); }
        else if (cmd == "x") { ls >> a; rc = h.flow().update_x(a); }
        else if (cmd == "cols") { ls >> a >> b >> c; rc = h.flow().update_columns(a, b, c); }
        else if (cmd == "B" || cmd == "E") rc = h.flow().update_gain(cmd == "E");
        else if (cmd == "parents") { ls >> a >> b; rc = h.flow().update_parents(a, b); }
        else if (cmd == "Q") rc = h.flow().update_noise(0);
        else if (cmd == "R") rc = h.flow().update_noise(1);
        else if (cmd == "Y") rc = h.flow().update_Y();
        else if (cmd == "elbo") rc = h.flow().elbo();
        else if (cmd == "iterate") { ls >> a; rc = h.iterate(a); }
        else if (cmd == "until") {
            ls >> a;
            std::vector<unsigned char> conv;
            while (ls >> b) conv.push_back((unsigned char)b);
            rc = h.until(a, conv);
        }
        // the setters: what api.hip launches and copies for them reads no state; their events
        else if (cmd == "priors") { h.parents[0].clear(); h.parents[1].clear(); h.st.parameters_changed(); }
        else if (cmd == "wishart_priors") { h.st.noise_changed(); h.st.parameters_changed(); }
        else if (cmd == "wishart_state") h.st.noise_changed();
        else if (cmd == "column_cov" || cmd == "column_obs") h.st.columns_changed();
        else if (cmd == "observations") { ls >> a; h.facts.has_missing = a != 0; h.st.outputs_changed(); }
        else if (cmd == "output_state") { if ((rc = h.settled("stage")) == PYVB_OK) h.st.outputs_changed(); }
        else if (cmd == "inputs" || cmd == "regressors") { h.facts.known_set[cmd == "regressors"] = true; h.st.outputs_changed(); }
        else if (cmd == "input_priors" || cmd == "regressor_priors") { h.facts.known_priors_set[cmd == "regressor_priors"] = true; h.st.parameters_changed(); }
        else if (cmd == "input_state" || cmd == "regressor_state") h.st.parameters_changed();
        else if (cmd == "state") { ls >> a >> b >> c; if ((rc = h.settled("stage")) == PYVB_OK) h.flow().state_given(a != 0, b != 0, c != 0); }
        else if (cmd == "classes") { if ((rc = h.settled("stage")) == PYVB_OK) h.st.classes_set(); }
        else if (cmd == "time_split") h.st.x_changed();
        else if (cmd == "set_parents") { ls >> a >> b; h.parents[a].begin(b); rc = h.parents[a].commit(h.flow().dev.parents(b, a, true)); }
        else if (cmd == "get_state" || cmd == "get_classes") rc = h.settled("copy");
        else if (cmd == "get_logdets") { if ((rc = h.flow().settle_parked()) == PYVB_OK && (rc = h.flow().ensure_lnd_x()) == PYVB_OK) fputs("copy\n", out); }
        else if (cmd == "active") {
            std::vector<unsigned char> m;
            while (ls >> b) m.push_back((unsigned char)b);
            rc = h.set_active(m);
        }
        else if (cmd == "bound") ls >> h.facts.bound;
        else return 2;
        if (rc) fprintf(out, "! %d %s\n", rc, g_err);
        const LdsState& s = h.st;
        fprintf(out, "= %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d\n", s.cur, (int)s.gains_valid, (int)s.expect_valid, (int)s.stats_valid,
                (int)s.resQ_valid, (int)s.resR_valid, (int)s.sg_valid[0], (int)s.sg_valid[1], (int)s.u_valid, (int)s.sxx_valid, s.fresh_count,
                (int)s.mixed_cov, (int)s.classes_valid, (int)s.lnd_x_pending, s.x_park, (int)s.cls_parked_other);
    }
    return fclose(out) == 0 ? 0 : 2;
}
