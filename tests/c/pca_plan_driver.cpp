// Runs the host-only state of a pyvb_pca handle and the planner of its sweeps (pyvb_amd/csrc/pca_plan.h) on a file of call
// sequences, for tests/test_pca_plan_cpu.py, which builds it with the address and undefined-behaviour sanitizers.  The entry
// points below string the state events and the planner together as api_pca.hip does, with a line of output where api_pca.hip
// launches or copies; nothing else happens.  No checks of its own: the test reads the output.
//   init N QT sweep has_xdata row_offset comm nchunk nchunkB     a new handle (comm: a communicator is attached)
//   W | Z | X0 | Mu | X lo hi | Beta | elbo | iterate n | read | set | variances | sweep kind      one call each
// Output: "> command", then the steps of the call --
//   store lo hi          k_pca_materialize on rows [lo, hi), from x_read
//   pass1 keep_z0        the rows of Z alone (resolve_z)
//   sweep lo hi with_z keep_z0 lazy pairs materialize vin_lo vin_hi part_chunks       the plan handed to pca_launch_sweep
//   small NAME           pca_launch_small; X0 and RUN_MID read row 0 where row_offset is 0, PREPZ and RUN_HEAD request the Z update
//   copy                 every row of X and Z is read (get_state) or about to be replaced (a setter)
// -- and "= full lin res z_pending z0_done xlazy vlo vhi part_chunks", the state after the call.
#include <cstdio>
#include <fstream>
#include <sstream>
#include <string>
#include "pca_plan.h"

struct Handle {
    PcaState st;
    PcaPlanInput in;
    long row_offset;
    bool comm;
    FILE* out;

    void x_read(long lo, long hi) {
        if (!st.needs_store(lo, hi)) return;
        fprintf(out, "store %ld %ld\n", st.vlo, st.vhi);
        st.x_stored();
    }
    void resolve_z() {
        x_read(0, in.N);
        if (!st.z_pending) return;
        fprintf(out, "pass1 %d\n", (int)st.z0_done);
        st.z_written();
    }
    void full_stats(long lo, long hi) {
        const PcaSweepPlan p = plan_sweep(st, in, lo, hi);
        fprintf(out, "sweep %ld %ld %d %d %d %d %d %ld %ld %d\n", p.lo_upd, p.hi_upd, (int)p.with_z, (int)p.keep_z0, (int)p.lazy, (int)p.pairs,
                (int)p.materialize, p.vin_lo, p.vin_hi, p.part_chunks);
        st.sweep_ran(p, true);
        st.stats_reduced(p);
    }
    void ensure_full() { if (!st.full_valid) full_stats(0, 0); }
    void small(const char* name) { fprintf(out, "small %s\n", name); }

    void update_W() { ensure_full(); st.residual_stale(); small("W"); }
    void update_Z() {
        if (!st.lin_valid) ensure_full();
        st.z_requested();
        small("PREPZ");
        st.linear_step();
    }
    void x0_step() {
        if (!st.lin_valid) ensure_full();
        x_read(0, row_offset == 0 ? 1 : 0);
        small("X0");
        st.x0_stepped(row_offset == 0);
        st.linear_step();
    }
    void x_rows(long lo, long hi) {
        if (lo == hi && !comm) return;
        full_stats(lo, hi);
    }
    void update_X(long lo, long hi) {
        if (lo == 0 && hi == 1 && row_offset == 0 && !comm) x0_step(); else x_rows(lo, hi);
    }
    void update_Mu() { if (!st.lin_valid) ensure_full(); st.residual_stale(); small("MU"); }
    void update_Beta() { ensure_full(); small("BETA"); st.beta_updated(); }
    void elbo() { ensure_full(); small("ELBO"); }
    void iterate(int n) {
        for (int it = 0; it < n; ++it) {
            const long first = row_offset == 0 ? 1 : 0;
            if (!comm) {
                ensure_full();
                st.z_requested();
                small("RUN_HEAD");
                st.linear_step();
                x_read(0, row_offset == 0 ? 1 : 0);
                small("RUN_MID");
                st.x0_stepped(row_offset == 0);
                x_rows(first, in.N);
                ensure_full();
                small("RUN_TAIL");
                st.beta_updated();
                continue;
            }
            update_W(); update_Z(); x0_step(); update_Mu(); x_rows(first, in.N); update_Beta(); elbo();
        }
    }
    void read() { resolve_z(); fputs("copy\n", out); }
    void set() { resolve_z(); fputs("copy\n", out); st.inputs_changed(); }
    void variances() { resolve_z(); st.residual_stale(); }
};

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    std::ifstream in(argv[1]);
    FILE* out = fopen(argv[2], "w");
    if (!in || !out) return 2;
    Handle h = Handle();
    h.out = out;
    std::string line, cmd;
    while (std::getline(in, line)) {
        std::istringstream ls(line);
        ls >> cmd;
        fprintf(out, "> %s\n", line.c_str());
        if (cmd == "init") {
            int xdata = 0, comm = 0;
            h.st = PcaState();          // as in a value-initialised handle: nothing valid, nothing pending
            ls >> h.in.N >> h.in.QT >> h.in.sweep >> xdata >> h.row_offset >> comm >> h.in.nchunk >> h.in.nchunkB;
            h.in.has_xdata = xdata != 0; h.comm = comm != 0;
        } else if (cmd == "W") h.update_W();
        else if (cmd == "Z") h.update_Z();
        else if (cmd == "X0") h.x0_step();
        else if (cmd == "Mu") h.update_Mu();
        else if (cmd == "X") { long lo = 0, hi = 0; ls >> lo >> hi; h.update_X(lo, hi); }
        else if (cmd == "Beta") h.update_Beta();
        else if (cmd == "elbo") h.elbo();
        else if (cmd == "iterate") { int n = 0; ls >> n; h.iterate(n); }
        else if (cmd == "read") h.read();
        else if (cmd == "set") h.set();
        else if (cmd == "variances") h.variances();
        else if (cmd == "sweep") ls >> h.in.sweep;
        else return 2;
        const PcaState& s = h.st;
        fprintf(out, "= %d %d %d %d %d %d %ld %ld %d\n", (int)s.full_valid, (int)s.lin_valid, (int)s.res_valid, (int)s.z_pending, (int)s.z0_done,
                (int)s.xlazy, s.vlo, s.vhi, s.part_chunks);
    }
    return fclose(out) == 0 ? 0 : 2;
}
