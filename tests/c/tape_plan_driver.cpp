// Runs the host-only tape planner (pyvb_amd/csrc/tape_plan.h) on a file, for tests/test_tape_plan_cpu.py, which builds it with
// the address and undefined-behaviour sanitizers.  No checks of its own: the test reads the output.
//   in : int64 arena_n; int32 nrec, nblocks, nlaunches, plan; int32 records[nrec][8], blocks[nblocks][2], launches[nlaunches][2]
//   out: int32 valid[nrec]; int64 tiled(blocks), tiled(launches); and if `plan` (records must all be valid, the tables tile):
//        int64 in_lds, ncops, nblockints, nwindows, nsegs, nlaunches, lds_windows, bundled_windows, lds_doubles, slots, bundles;
//        int32 cops[], blocks[], windows[][8], segs[][4], width[]; int64 lds_bytes[]
#include <cstdint>
#include <cstdio>
#include "tape_plan.h"

template <class T> static std::vector<T> get(FILE* f, size_t n) { std::vector<T> v(n); if (n && fread(v.data(), sizeof(T), n, f) != n) v.clear(); return v; }
template <class T> static void put(FILE* f, const std::vector<T>& v) { if (!v.empty()) fwrite(v.data(), sizeof(T), v.size(), f); }

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    FILE* in = fopen(argv[1], "rb");
    FILE* out = fopen(argv[2], "wb");
    if (!in || !out) return 2;
    const int64_t arena_n = get<int64_t>(in, 1).at(0);
    const std::vector<int> head = get<int>(in, 4);
    const std::vector<int> recs = get<int>(in, 8 * (size_t)head.at(0)), blocks = get<int>(in, 2 * (size_t)head.at(1)), launches = get<int>(in, 2 * (size_t)head.at(2));
    std::vector<int> valid;
    for (int r = 0; r < head[0]; ++r) valid.push_back(tape_record_valid(&recs.at(8 * (size_t)r), (size_t)arena_n));
    put(out, valid);
    put(out, std::vector<int64_t>{tape_tiled(blocks.data(), head[1]), tape_tiled(launches.data(), head[2])});
    if (head[3]) {
        const TapePlan P = tape_plan(recs, blocks, launches, (size_t)arena_n);
        put(out, std::vector<int64_t>{P.in_lds, (int64_t)P.cops.size(), (int64_t)P.blocks.size(), (int64_t)P.windows.size(), (int64_t)P.segs.size(),
                                      (int64_t)P.width.size(), P.lds_windows, P.bundled_windows, P.lds_doubles, P.slots, P.bundles});
        put(out, P.cops); put(out, P.blocks); put(out, P.windows); put(out, P.segs); put(out, P.width);
        put(out, std::vector<int64_t>(P.lds_bytes.begin(), P.lds_bytes.end()));
    }
    fclose(in);
    return fclose(out) == 0 ? 0 : 2;
}
