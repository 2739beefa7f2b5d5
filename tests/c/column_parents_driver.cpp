// Runs the host-only record of the columns' precision parents (pyvb_amd/csrc/column_parents.h) on a file of commands, for
// tests/test_column_parents_cpu.py, which builds it with the address and undefined-behaviour sanitizers.  No checks of its own: the
// test reads the output.  One command per line, words separated by blanks, doubles as strtod reads them (hexadecimal floats, nan,
// inf); one line of output per command, doubles as %a.
//   seq op..                 two records, all zero at the start.  op = a letter and the matrix (0 / 1): c clear, g / d a setter of
//                            Gamma / DiagonalGamma parents whose launch is made, G / D one whose launch fails
//                            -> per op "kind0 kind1 which_gamma which_dg rc", joined by "|"  (which_*: parents_of_kind)
//   require kind want pca of -> "rc|message"                              a record of that kind asked for parents of kind `want`
//   check what rows pca replicate of n v..       -> "rc|message"          check_positive
//   bcast N per rows model.. qb..                -> "rc|message|out.."    broadcast_qb on Replicates::init(N, 2, null, model)
//   gamma n rows with_qb a0.. b0.. [qb..]        -> out..                 stage_gamma
//   dgamma n with_qb a0.. b0.. [qb..]            -> out..                 stage_diagonal_gamma
//   block kind N D per       -> "head ex qb ld_ref ld_exact own total"    lds_parent_block
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>
#include "column_parents.h"

static char g_err[512] = "";
void pyvb_set_error(const char* fmt, ...) {
    va_list ap; va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

static std::vector<double> take(std::istringstream& in, size_t n) {
    std::vector<double> v(n);
    std::string w;
    for (size_t i = 0; i < n; ++i) { in >> w; v[i] = strtod(w.c_str(), nullptr); }
    return v;
}
static void row(FILE* out, const std::vector<double>& v) {
    for (size_t i = 0; i < v.size(); ++i) fprintf(out, "%s%a", i ? " " : "", v[i]);
    fputs("\n", out);
}

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    std::ifstream in(argv[1]);
    FILE* out = fopen(argv[2], "w");
    if (!in || !out) return 2;
    std::string line, cmd;
    while (std::getline(in, line)) {
        std::istringstream ls(line);
        ls >> cmd;
        g_err[0] = 0;
        if (cmd == "seq") {
            ColumnParents p[2];
            memset(p, 0, sizeof(p));
            std::string op;
            for (int i = 0; ls >> op; ++i) {
                ColumnParents& r = p[op[1] - '0'];
                int rc = PYVB_OK;
                if (op[0] == 'c') r.clear();
                else {
                    r.begin(op[0] == 'g' || op[0] == 'G' ? PARENTS_GAMMA : PARENTS_DIAGONAL_GAMMA);
                    rc = r.commit(op[0] == 'G' || op[0] == 'D' ? PYVB_E_HIP : PYVB_OK);
                }
                fprintf(out, "%s%d %d %d %d %d", i ? "|" : "", p[0].kind, p[1].kind, parents_of_kind(p, PARENTS_GAMMA),
                        parents_of_kind(p, PARENTS_DIAGONAL_GAMMA), rc);
            }
            fputs("\n", out);
        } else if (cmd == "require") {
            int kind = 0, want = 0, pca = 0;
            std::string of;
            ls >> kind >> want >> pca >> of;
            ColumnParents r;
            memset(&r, 0, sizeof(r));
            r.kind = kind;
            const int rc = r.require(want, ParentWords{of.c_str(), pca != 0});
            fprintf(out, "%d|%s\n", rc, g_err);
        } else if (cmd == "check") {
            std::string what, of;
            size_t rows = 0, n = 0;
            int pca = 0, replicate = 0;
            ls >> what >> rows >> pca >> replicate >> of >> n;
            const std::vector<double> v = take(ls, n);
            const int rc = check_positive(v.data(), n, rows, what.c_str(), ParentWords{of.c_str(), pca != 0}, replicate);
            fprintf(out, "%d|%s\n", rc, g_err);
        } else if (cmd == "bcast") {
            size_t N = 0, per = 0, rows = 0;
            ls >> N >> per >> rows;
            std::vector<int> model(N);
            for (size_t n = 0; n < N; ++n) ls >> model[n];
            const std::vector<double> qb = take(ls, N * per);
            Replicates rep;
            rep.init((int)N, 2, nullptr, model.data());
            std::vector<double> o;
            const int rc = broadcast_qb(rep, qb.data(), per, rows, ParentWords{"A", false}, o);
            fprintf(out, "%d|%s|", rc, g_err);
            row(out, rc ? std::vector<double>() : o);
        } else if (cmd == "gamma" || cmd == "dgamma") {
            size_t n = 0;
            int rows = 0, with_qb = 0;
            ls >> n;
            if (cmd == "gamma") ls >> rows;
            ls >> with_qb;
            const std::vector<double> a0 = take(ls, n), b0 = take(ls, n), qb = take(ls, with_qb ? n : 0);
            std::vector<double> o;
            if (cmd == "gamma") stage_gamma(o, a0.data(), b0.data(), n, rows, with_qb ? qb.data() : nullptr);
            else stage_diagonal_gamma(o, a0.data(), b0.data(), n, with_qb ? qb.data() : nullptr);
            row(out, o);
        } else if (cmd == "block") {
            int kind = 0;
            size_t N = 0, D = 0, per = 0;
            ls >> kind >> N >> D >> per;
            const LdsParentBlock o = lds_parent_block(kind, N, D, per);
            fprintf(out, "%zu %zu %zu %zu %zu %zu %zu\n", o.head, o.ex, o.qb, o.ld_ref, o.ld_exact, o.own, o.total);
        } else return 2;
    }
    return fclose(out) == 0 ? 0 : 2;
}
