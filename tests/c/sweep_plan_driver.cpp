// Runs the plan of a segmented sweep (pyvb_amd/csrc/sweep_plan.h) on a file of commands, for tests/test_sweep_plan_cpu.py,
// which builds it with the address and undefined-behaviour sanitizers.  No checks of its own: the test reads the output.
// One command per line, integers separated by blanks; one line of output per command.
//   plan TL T W w J forward  -> "Tint ow Tw Lseg first_step correction_steps|before count jc kind|.." (the 16 columns)
//   active TL T W w J forward c j0 j1 -> sweep_active of column c at loop indices j0 .. j1 - 1, as 0 / 1
#include <cstdarg>
#include <cstdio>
#include <fstream>
#include <sstream>
#include <string>
#include "sweep_plan.h"

void pyvb_set_error(const char*, ...) {}

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    std::ifstream in(argv[1]);
    FILE* out = fopen(argv[2], "w");
    if (!in || !out) return 2;
    std::string line, cmd;
    while (std::getline(in, line)) {
        std::istringstream ls(line);
        ls >> cmd;
        int TL = 0, T = 0, W = 0, w = 0, J = 0, forward = 0;
        ls >> TL >> T >> W >> w >> J >> forward;
        const SweepPart p = sweep_part(TL, T, W, w, J, forward != 0);
        if (cmd == "plan") {
            fprintf(out, "%d %d %d %d %d %d", p.Tint, p.ow, p.Tw, p.Lseg, sweep_first_step(p), sweep_correction_steps(p));
            for (int c = 0; c < SWEEP_COLUMNS; ++c) {
                const SweepColumn s = sweep_column(p, c);
                fprintf(out, "|%d %d %d %d", s.before, s.count, s.jc, s.kind);
            }
            fputs("\n", out);
        } else if (cmd == "active") {
            int c = 0, j0 = 0, j1 = 0;
            ls >> c >> j0 >> j1;
            const SweepColumn s = sweep_column(p, c);
            for (int j = j0; j < j1; ++j) fputc(sweep_active(p, s, j) ? '1' : '0', out);
            fputs("\n", out);
        } else return 2;
    }
    return fclose(out) == 0 ? 0 : 2;
}
