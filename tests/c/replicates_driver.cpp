// Runs the host-only record of a handle's replicates (pyvb_amd/csrc/replicates.h) on a file of commands, for
// tests/test_replicates_cpu.py, which builds it with the address and undefined-behaviour sanitizers.  No checks of its own: the
// test reads the output.  One command per line, integers separated by blanks; one or more lines of output per command.
//   models N id..            -> "rc tied|message"                       Replicates::check_models
//   lengths N T len..        -> "rc ragged|message"                     Replicates::check_lengths
//   init N T nl len.. nm id..   (nl, nm: 0 = the array is null, else N) -> "M ragged tied", then one line each of length, model,
//                               first_of, children of Q, children of R (N numbers), mstart, first (as stored), and the state
//   mask b..                 -> "rc differs|message" (check_mask; adopted where it passes and differs), then the state
//   conv b..                 -> the state (adopt_conv)
//   state: "n_active|run mask|caller mask"
#include <cstdarg>
#include <cstdio>
#include <fstream>
#include <sstream>
#include <string>
#include "replicates.h"

static char g_err[512] = "";
void pyvb_set_error(const char* fmt, ...) {
    va_list ap; va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

template <class V> static void row(FILE* out, const V& v, const char* end = "\n") {
    for (size_t i = 0; i < v.size(); ++i) fprintf(out, "%s%ld", i ? " " : "", (long)v[i]);
    fputs(end, out);
}
template <class T> static std::vector<T> take(std::istringstream& in, size_t n) {
    std::vector<T> v(n);
    for (size_t i = 0; i < n; ++i) { long x = 0; in >> x; v[i] = (T)x; }
    return v;
}
static void state(FILE* out, const Replicates& r) {
    fprintf(out, "%d|", r.n_active());
    row(out, r.run_mask(), "|");
    row(out, std::vector<unsigned char>(r.caller_mask(), r.caller_mask() + r.size()));
}

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    std::ifstream in(argv[1]);
    FILE* out = fopen(argv[2], "w");
    if (!in || !out) return 2;
    Replicates r;
    std::string line, cmd;
    while (std::getline(in, line)) {
        std::istringstream ls(line);
        ls >> cmd;
        g_err[0] = 0;
        if (cmd == "models" || cmd == "lengths") {
            int N = 0, T = 0;
            ls >> N;
            if (cmd == "lengths") ls >> T;
            const std::vector<int> a = take<int>(ls, (size_t)N);
            bool flag = false;
            const int rc = cmd == "models" ? Replicates::check_models(N, a.data(), &flag) : Replicates::check_lengths(N, T, a.data(), &flag);
            fprintf(out, "%d %d|%s\n", rc, (int)flag, g_err);
        } else if (cmd == "init") {
            int N = 0, T = 0, nl = 0, nm = 0;
            ls >> N >> T >> nl;
            const std::vector<int> len = take<int>(ls, (size_t)nl);
            ls >> nm;
            const std::vector<int> mod = take<int>(ls, (size_t)nm);
            r.init(N, T, nl ? len.data() : nullptr, nm ? mod.data() : nullptr);
            fprintf(out, "%d %d %d\n", r.M(), (int)r.ragged(), (int)r.tied());
            std::vector<long> q[3], nq, nr;
            for (int n = 0; n < N; ++n) { q[0].push_back(r.length(n)); q[1].push_back(r.model(n)); q[2].push_back(r.first_of(n)); }
            r.children(nq, nr);
            row(out, q[0]); row(out, q[1]); row(out, q[2]); row(out, nq); row(out, nr); row(out, r.model_starts()); row(out, r.first_flags());
            state(out, r);
        } else if (cmd == "mask") {
            const std::vector<unsigned char> b = take<unsigned char>(ls, (size_t)r.size());
            const int rc = r.check_mask(b.data());
            const bool differs = rc == PYVB_OK && r.mask_differs(b.data());
            if (differs) r.adopt_mask(b.data());
            fprintf(out, "%d %d|%s\n", rc, (int)differs, g_err);
            state(out, r);
        } else if (cmd == "conv") {
            const std::vector<unsigned char> b = take<unsigned char>(ls, (size_t)r.size());
            r.adopt_conv(b.data());
            state(out, r);
        } else return 2;
    }
    return fclose(out) == 0 ? 0 : 2;
}
