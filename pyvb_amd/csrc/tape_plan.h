// The host half of the generic per-node path: which arena extents a tape record touches, whether a record is well formed,
// and the LDS-window form of a tape (tape.h).  Standard C++ only: nothing here needs a device, so tests/c/tape_plan_driver.cpp
// runs it under the host sanitizers and tests/test_tape_plan_cpu.py replays its plans in numpy.
#pragma once
#include <algorithm>
#include <cstddef>
#include <vector>
#include "tape.h"

// ---- one description per opcode: validation, windows and bundles all read it
struct TapeExtent { long off; size_t len; bool write; int field; };     // field: index of the record field that holds `off`
struct TapeRecord {
    bool ok;                    // known opcode whose shape constraints hold (sizes not negative, leading dimensions >= n, ...)
    bool data;                  // gather / scatter: the elements the index vectors address are checked by the kernel; ext: the rest
    int n; TapeExtent ext[5];   // extents of length zero touch nothing and are not listed
};

inline size_t tape_span(int rows, int cols, int ld) { return rows > 0 && cols > 0 ? (size_t)(rows - 1) * (size_t)ld + cols : 0; }

inline TapeRecord tape_describe(const int* o) {
    const int op = o[0], m = o[4], n = o[5], p = o[6], flags = o[7];
    TapeRecord d{};
    if (m < 0 || n < 0) return d;
    const size_t mn = (size_t)m * n, mm = (size_t)m * m;
    const bool R = false, W = true;
    // the opcodes whose elements get their row and column from tape_divmod: exact up to TAPE_MAX_ELEMS elements (tape.h)
    const bool by_mn = op == T_COPY2D || op == T_FILL || op == T_GEMM, by_mm = op == T_CHOLINV || (op == T_DIAG && (flags & 1));
    if ((by_mn && mn > (size_t)TAPE_MAX_ELEMS) || (by_mm && mm > (size_t)TAPE_MAX_ELEMS)) return d;
    auto at = [&](int field, long off, size_t len, bool write) { if (len) d.ext[d.n++] = TapeExtent{off, len, write, field}; };
    auto add = [&](int field, size_t len, bool write) { at(field, o[field], len, write); };
    switch (op) {
    case T_NOP: break;
    case T_COPY2D: if (o[3] < n || p < n) return d; add(1, tape_span(m, n, o[3]), W); add(2, tape_span(m, n, p), R); break;
    case T_FILL: if (o[3] < n) return d; add(1, tape_span(m, n, o[3]), W); break;
    case T_AXPBY: add(1, mn, W); add(2, mn, R); add(6, 1, R); if (o[3] >= 0) { add(3, mn, R); add(7, 1, R); } break;
    case T_GEMM: if (p < 0) return d; add(1, mn, W); add(2, (size_t)m * p, R); add(3, (size_t)p * n, R); break;
    case T_SCALE: add(1, mn, W); add(2, mn, R); add(3, 1, R); break;
    case T_TRACE: add(1, 1, W); add(2, mm, R); break;
    case T_DOT: add(1, 1, W); add(2, mn, R); add(3, mn, R); break;
    case T_DIAG: if (flags & 1) { add(1, mm, W); add(2, m, R); } else { add(1, m, W); add(2, mm, R); } break;
    case T_CHOLINV: add(1, mm, W); add(2, mm, R); add(3, 2, W); add(6, 2 * mm, W); break;
    case T_UNARY: if (flags < 0 || flags > 5) return d; add(1, mn, W); add(2, mn, R); break;
    case T_MUL: add(1, mn, W); add(2, mn, R); add(3, mn, R); break;
    case T_GATHER: if (p < 0) return d; d.data = true; add(1, mn, W); add(2, 1, R); add(3, m, R); add(7, n, R); break;
    case T_SCATTER: if (p < 0) return d; d.data = true; add(1, 1, W); add(2, mn, R); add(3, m, R); at(7, flags & ~T_ACC, n, R); break;
    default: return d;
    }
    d.ok = true;
    return d;
}

// well formed, and every extent inside an arena of arena_n doubles
inline bool tape_record_valid(const int* o, size_t arena_n) {
    const TapeRecord d = tape_describe(o);
    for (int k = 0; k < d.n; ++k)
        if (d.ext[k].off < 0 || (size_t)d.ext[k].off + d.ext[k].len > arena_n) return false;
    return d.ok;
}

// {first, count} pairs that tile a range from 0 in order (the blocks of a program its tape, the launches its blocks): its length, or -1
inline long tape_tiled(const int* t, int n) {
    long at = 0;
    for (int i = 0; i < n; ++i) { if (t[2 * i] != at || t[2 * i + 1] <= 0) return -1; at += t[2 * i + 1]; }
    return at;
}

// ---- the plan: what the device gets for a tape, its blocks and launches (all records valid)
struct TapePlan {
    bool in_lds = false;                // some window runs out of LDS: otherwise the plain tape is as good and nothing is uploaded
    std::vector<int> cops;              // device records, window by window: resolved (T_LDS) and bundled, or as given
    std::vector<int> blocks;            // {first window, number of windows} per block
    std::vector<TapeWindow> windows;
    std::vector<TapeSegment> segs;
    std::vector<size_t> lds_bytes;      // per launch: dynamic LDS of its workgroups (window, padding, TAPE_CHUNK staged records)
    std::vector<int> width;             // per launch: records of a bundle = wavefronts of a workgroup
    int lds_windows = 0, bundled_windows = 0;           // counts of the plan, for who asks the planner (tests/c/tape_plan_driver.cpp); the library does not read them
    long lds_doubles = 0, slots = 0, bundles = 0;
};

// The extents of records [first, first + count) merged into segments (overlapping or adjacent only: a gap may be another
// block's state), `total` doubles of LDS; false if a record's addresses are data.
inline bool tape_segments(const std::vector<int>& raw, int first, int count, std::vector<TapeSegment>& sg, long& total) {
    std::vector<TapeExtent> ext;
    for (int r = first; r < first + count; ++r) {
        const TapeRecord d = tape_describe(&raw[8 * (size_t)r]);
        if (d.data) return false;
        ext.insert(ext.end(), d.ext, d.ext + d.n);
    }
    std::sort(ext.begin(), ext.end(), [](const TapeExtent& x, const TapeExtent& y) { return x.off < y.off; });
    sg.clear(); total = 0;
    for (const TapeExtent& e : ext) {           // (offsets and lengths of valid records are below 2^30)
        const int off = (int)e.off, end = off + (int)e.len;
        if (!sg.empty() && off <= sg.back().off + sg.back().len) {
            sg.back().len = std::max(sg.back().len, end - sg.back().off);
            sg.back().written |= e.write;
        } else sg.push_back(TapeSegment{off, (int)e.len, -1, e.write});
    }
    for (const TapeSegment& q : sg) total += (q.len + 1) & ~1;
    return true;
}

// The longest run of at most `left` records from r whose segments fit the LDS budget: grown geometrically, then bisected.
// Its segments and their doubles are left in best / used.
inline int tape_longest_run(const std::vector<int>& raw, int r, int left, std::vector<TapeSegment>& best, long& used) {
    std::vector<TapeSegment> sg;
    long tot = 0;
    auto fits = [&](int c) {
        if (!tape_segments(raw, r, c, sg, tot) || tot > TAPE_LDS_CAP || (int)sg.size() > TAPE_MAX_SEGS) return false;
        best = sg; used = tot;
        return true;
    };
    int lo = 0, hi = 1;             // lo fits (0 = nothing tried), hi is the next candidate
    while (lo < left && fits(hi)) { lo = hi; hi = std::min(2 * hi, left); }
    while (hi - lo > 1 && lo < left) {          // lo fits, hi does not
        const int mid = (lo + hi) / 2;
        if (fits(mid)) lo = mid; else hi = mid;
    }
    return lo;
}

// Lay the segments out in the window and rewrite the offsets of records [r, r + len) in `ops` to window positions: every
// extent of these records lies in one segment.  Returns the largest element count of a record.
inline long tape_resolve(const std::vector<int>& raw, std::vector<int>& ops, int r, int len, std::vector<TapeSegment>& best) {
    long widest = 0;
    int pos = 0;
    for (TapeSegment& q : best) { q.lds = pos; pos += (q.len + 1) & ~1; }
    for (int rr = r; rr < r + len; ++rr) {
        const int* o = &raw[8 * (size_t)rr];
        const TapeRecord d = tape_describe(o);
        for (int k = 0; k < d.n; ++k) {
            const TapeExtent& e = d.ext[k];
            // the segment that holds e.off: the last one starting at or before it
            const auto q = std::upper_bound(best.begin(), best.end(), e.off, [](long off, const TapeSegment& s) { return off < s.off; }) - 1;
            ops[8 * (size_t)rr + e.field] = T_LDS | (q->lds + (int)(e.off - q->off));
        }
        const long mm = (long)o[4] * o[4], mn = (long)o[4] * o[5];
        widest = std::max(widest, (o[0] == T_CHOLINV || o[0] == T_DIAG || o[0] == T_TRACE) ? mm : mn);
    }
    return widest;
}

inline bool tape_hazard(const TapeRecord& x, const TapeRecord& y) {     // an extent of one overlaps one of the other, not both read
    for (int i = 0; i < x.n; ++i)
        for (int j = 0; j < y.n; ++j) {
            const TapeExtent &a = x.ext[i], &b = y.ext[j];
            if ((a.write || b.write) && a.off < b.off + (long)b.len && b.off < a.off + (long)a.len) return true;
        }
    return false;
}

// Records [first, first + count) of `ops` (resolved: window offsets) scheduled into bundles of BW mutually independent records,
// appended to `out` (T_NOP in the free slots).  A record depends on every earlier one that touches one of its extents unless both
// only read it; it goes into the first bundle after all of its dependencies that has a free slot (list scheduling: any order that
// respects the dependencies computes what the tape computes).  Extents are taken from the unresolved records `raw`.
inline void tape_bundle(const std::vector<int>& raw, const std::vector<int>& ops, int first, int count, std::vector<int>& out, int BW) {
    std::vector<TapeRecord> rec((size_t)count);
    for (int r = 0; r < count; ++r) rec[r] = tape_describe(&raw[8 * (size_t)(first + r)]);
    std::vector<int> bundle((size_t)count, 0), fill;
    for (int r = 0; r < count; ++r) {
        int earliest = 0;
        for (int q = r - 1; q >= 0; --q)
            if (bundle[q] >= earliest && tape_hazard(rec[r], rec[q])) earliest = bundle[q] + 1;     // below: cannot raise the bound
        int b = earliest;
        while (b < (int)fill.size() && fill[b] >= BW) ++b;
        if (b >= (int)fill.size()) fill.resize((size_t)b + 1, 0);
        bundle[r] = b; ++fill[b];
    }
    const size_t base = out.size();
    out.resize(base + fill.size() * 8 * BW, 0);                 // T_NOP == 0
    std::fill(fill.begin(), fill.end(), 0);
    for (int r = 0; r < count; ++r)             // in tape order into the slots of its bundle
        std::copy_n(&ops[8 * (size_t)(first + r)], 8, &out[base + ((size_t)bundle[r] * BW + fill[bundle[r]]++) * 8]);
}

// c records from r stay on the arena: gather / scatter, a record that does not fit by itself, or a run too short to pay for a
// load and a write-back.  Runs of such records of one block (its windows start at w0) are kept together in one window.
inline void tape_arena_run(TapePlan& P, const std::vector<int>& raw, int r, int c, size_t w0) {
    const int at = (int)(P.cops.size() / 8);
    P.cops.insert(P.cops.end(), raw.begin() + 8 * (size_t)r, raw.begin() + 8 * (size_t)(r + c));
    if (P.windows.size() > w0 && P.windows.back().nseg == 0 && P.windows.back().first + P.windows.back().count == at) P.windows.back().count += c;
    else P.windows.push_back(TapeWindow{at, c, (int)P.segs.size(), 0, 0, 0, {0, 0}});
}

// The windows of one block, records [r, end), with bundles BW wide.  Returns the doubles of its largest window.
inline long tape_plan_block(TapePlan& P, const std::vector<int>& raw, std::vector<int>& ops, int r, int end, int BW) {
    const size_t w0 = P.windows.size();
    std::vector<TapeSegment> best;
    long need = 0, used = 0;
    for (int len; r < end; r += len) {
        len = tape_longest_run(raw, r, end - r, best, used);
        if (len < 3) { len = std::max(len, 1); tape_arena_run(P, raw, r, len, w0); continue; }
        const bool bundled = tape_resolve(raw, ops, r, len, best) <= 64;        // every record is node-sized
        const int at = (int)(P.cops.size() / 8);
        if (!bundled) P.cops.insert(P.cops.end(), ops.begin() + 8 * (size_t)r, ops.begin() + 8 * (size_t)(r + len));
        else for (int p0 = 0; p0 < len; p0 += TAPE_BUNDLE_MAX)                  // piece by piece: the search is quadratic in the piece
            tape_bundle(raw, ops, r + p0, std::min(TAPE_BUNDLE_MAX, len - p0), P.cops, BW);
        P.windows.push_back(TapeWindow{at, (int)(P.cops.size() / 8) - at, (int)P.segs.size(), (int)best.size(), (int)used, bundled, {0, 0}});
        P.segs.insert(P.segs.end(), best.begin(), best.end());
        P.in_lds = true; need = std::max(need, used);
    }
    P.blocks.push_back((int)w0); P.blocks.push_back((int)(P.windows.size() - w0));
    return need;
}

// The window form of the tape `raw` for the given blocks ({first record, count} each, tiling the tape) and launches ({first
// block, number}, tiling the blocks).  Nothing is planned when the arena does not leave bit 30 of an offset free.
inline TapePlan tape_plan(const std::vector<int>& raw, const std::vector<int>& blocks, const std::vector<int>& launches, size_t arena_n) {
    TapePlan P;
    if (arena_n >= (size_t)T_LDS) return P;
    std::vector<int> ops = raw;                                 // resolved in place
    for (size_t l = 0; l + 1 < launches.size(); l += 2) {
        P.width.push_back(launches[l + 1] >= 512 ? 4 : TAPE_BUNDLE);        // many short blocks: narrow workgroups fit a CU more often
        long need = 0;
        for (int b = launches[l]; b < launches[l] + launches[l + 1]; ++b)
            need = std::max(need, tape_plan_block(P, raw, ops, blocks[2 * b], blocks[2 * b] + blocks[2 * b + 1], P.width.back()));
        P.lds_bytes.push_back(((size_t)need + 2 + (size_t)TAPE_CHUNK * 4) * sizeof(double));
    }
    for (const TapeWindow& w : P.windows) {
        if (w.bundled) { ++P.bundled_windows; P.slots += w.count; }
        if (w.nseg) { ++P.lds_windows; P.lds_doubles += w.doubles; }
    }
    P.bundles = P.slots / (P.width.empty() ? TAPE_BUNDLE : P.width[0]);
    return P;
}
