// Runs the host-only sizing rules of a handle (pyvb_amd/csrc/geometry.h) on a file of commands, for tests/test_geometry_cpu.py,
// which builds it with the address and undefined-behaviour sanitizers.  No checks of its own: the test reads the output.
// One command per line, integers separated by blanks; one line of output per command.
//   lds N T D K noise        -> "big dense nchunk chunk_len W|sxx U2 trash scratch SG stats mom priors"       lds_geometry
//   split N T D K noise W    -> the same line for lds_geometry(..).with_time_split(W)
//   check T W                -> "rc|message"                                                                  check_time_split
//   parts T W TL..           -> "part_len split_part_len|live_parts(TL, T, W).."
//   layout D K               -> "D K DT KT DP KP DS KS QR|oFn oBn oGp oS0 oS2 oqr ow0 gains_total|oSxx oSx1x oSyx stats_total"
//   xpos n                   -> xpos(0) .. xpos(n - 1)
//   nat R C S / perm R C S   -> pos_nat / pos_perm of (i, j), i < R, j < C, row by row
//   cov rows                 -> "cov_tiles cov_stride"
//   pca N d q ncu            -> "DP QP DT QT nchunk chunk_rows nchunkB chunk_rowsB sweep"                      pca_geometry
#include <cstdarg>
#include <cstdio>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>
#include "geometry.h"

static char g_err[512] = "";
void pyvb_set_error(const char* fmt, ...) {
    va_list ap; va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

static void lds_line(FILE* out, const LdsGeometry& g) {
    fprintf(out, "%d %d %d %d %d|%zu %zu %zu %zu %zu %zu %zu %zu\n", (int)g.big, (int)g.dense, g.nchunk, g.chunk_len, g.W,
            g.sxx, g.U2, g.trash, g.scratch, g.SG, g.stats, g.mom, g.priors);
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
        if (cmd == "lds" || cmd == "split") {
            int N = 0, T = 0, D = 0, K = 0, noise = 0, W = 0;
            ls >> N >> T >> D >> K >> noise;
            const LdsGeometry g = lds_geometry(N, T, D, K, noise);
            if (cmd == "split") { ls >> W; lds_line(out, g.with_time_split(W)); } else lds_line(out, g);
        } else if (cmd == "check") {
            int T = 0, W = 0;
            ls >> T >> W;
            const int rc = check_time_split(T, W);
            fprintf(out, "%d|%s\n", rc, g_err);
        } else if (cmd == "parts") {
            int T = 0, W = 0, TL = 0;
            ls >> T >> W;
            fprintf(out, "%d %d|", part_len(T, W), split_part_len(T, W));
            for (bool first = true; ls >> TL; first = false) fprintf(out, "%s%d", first ? "" : " ", live_parts(TL, T, W));
            fputs("\n", out);
        } else if (cmd == "layout") {
            int D = 0, K = 0;
            ls >> D >> K;
            const Layout L = make_layout(D, K);
            fprintf(out, "%d %d %d %d %d %d %d %d %d|%zu %zu %zu %zu %zu %zu %zu %zu|%zu %zu %zu %zu\n", L.D, L.K, L.DT, L.KT, L.DP, L.KP, L.DS, L.KS, L.QR,
                    L.oFn, L.oBn, L.oGp, L.oS0, L.oS2, L.oqr, L.ow0, L.gains_total, L.oSxx, L.oSx1x, L.oSyx, L.stats_total);
        } else if (cmd == "xpos") {
            int n = 0;
            ls >> n;
            for (int d = 0; d < n; ++d) fprintf(out, "%s%d", d ? " " : "", xpos(d));
            fputs("\n", out);
        } else if (cmd == "nat" || cmd == "perm") {
            int R = 0, C = 0, S = 0;
            ls >> R >> C >> S;
            for (int i = 0; i < R; ++i)
                for (int j = 0; j < C; ++j) fprintf(out, "%s%zu", i + j ? " " : "", cmd == "nat" ? pos_nat(i, j, S) : pos_perm(i, j, S));
            fputs("\n", out);
        } else if (cmd == "cov") {
            int rows = 0;
            ls >> rows;
            fprintf(out, "%d %zu\n", cov_tiles(rows), cov_stride(rows));
        } else if (cmd == "pca") {
            long N = 0; int d = 0, q = 0, ncu = 0;
            ls >> N >> d >> q >> ncu;
            const PcaGeometry g = pca_geometry(N, d, q, ncu);
            fprintf(out, "%d %d %d %d %d %ld %d %ld %d\n", g.DP, g.QP, g.DT, g.QT, g.nchunk, g.chunk_rows, g.nchunkB, g.chunk_rowsB, g.sweep);
        } else return 2;
    }
    return fclose(out) == 0 ? 0 : 2;
}
