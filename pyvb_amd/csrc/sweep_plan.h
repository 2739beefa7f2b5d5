// The plan of a segmented sweep (k_sweep.hip): which interior nodes each of the 16 columns of a wavefront owns, at which
// loop index it begins and from what state.  Standard C++ only: tests/c/sweep_plan_driver.cpp runs it under the host
// sanitizers and tests/test_sweep_plan_cpu.py checks it over a grid of chain lengths and warm-up lengths; the kernel reads
// `before`, `jc`, `jstart` and `active` from the same functions.
//
// The interior nodes 1 .. T_n-2 of a chain, counted from the side the sweep starts at, are dealt out to W parts
// (geometry.h: part_len) and every part to 16 columns of Lseg = ceil(Tw / 16) nodes.  Loop index j of a column is its
// (j+1)-th own node; negative j are warm-up steps on the nodes of the column before.  A column starts in one of three ways:
//   SWEEP_START_BOUNDARY  the warm-up would reach the chain's first node (before <= J): the column starts there, from the
//                         true boundary state, and reproduces the sequential chain exactly (short chains take this path);
//   SWEEP_START_SEAM      at its own first node (j = 0) from zero.  The recurrence is linear, so what it then computes is
//                         mu_t - R^(k+1) e for its (k+1)-th node, e the final state of the column to its left; the sweep
//                         hands e over afterwards and adds delta <- R delta for J steps (one product a step, not three);
//   SWEEP_START_WARM      J steps early from zero, on the nodes of the column before.
// A seam start needs the forward sweep without time split (W == 1), J own nodes to correct, and a left neighbour of at
// least J nodes: then that neighbour's final state is exact to ||R^J|| <= 1e-18, whatever its own start was -- the bound
// that sizes the warm-up.  Everything else warms up as before.
#pragma once
#include "geometry.h"

enum { SWEEP_START_BOUNDARY = 0, SWEEP_START_SEAM = 1, SWEEP_START_WARM = 2 };
enum { SWEEP_COLUMNS = 16 };

// one part of one chain in one direction: wave-uniform
struct SweepPart {
    int Tint;       // interior nodes of the chain
    int ow;         // interior nodes before this part
    int Tw;         // interior nodes of this part (<= 0: none)
    int Lseg;       // nodes per column
    int J;          // warm-up length
    bool seams;     // seam starts are admitted: forward, W == 1
};

struct SweepColumn {
    int before;     // interior nodes between the chain's start and this column
    int count;      // nodes this column owns (0: none)
    int jc;         // its first loop index: -before, 0 or -J
    int kind;       // SWEEP_START_*
};

// TL: nodes of the chain; T: the handle's row stride, from which the parts are cut; w: the part; J: a.warm of the direction
PYVB_HD static inline SweepPart sweep_part(int TL, int T, int W, int w, int J, bool forward) {
    SweepPart p;
    p.Tint = TL - 2;
    const int Lw = W > 1 ? split_part_len(T, W) : p.Tint;
    p.ow = W > 1 ? w * Lw : 0;
    p.Tw = (p.Tint - p.ow < Lw) ? p.Tint - p.ow : Lw;
    p.Lseg = p.Tw > 0 ? (p.Tw + 15) >> 4 : 0;
    p.J = J;
    p.seams = forward && W == 1;
    return p;
}

// nodes column c owns
PYVB_HD static inline int sweep_column_count(const SweepPart& p, int c) {
    const int left = p.Tw - c * p.Lseg;
    return left <= 0 ? 0 : (left < p.Lseg ? left : p.Lseg);
}

PYVB_HD static inline SweepColumn sweep_column(const SweepPart& p, int c) {
    SweepColumn s;
    s.before = p.ow + c * p.Lseg;
    s.count = sweep_column_count(p, c);
    if (s.before <= p.J) { s.kind = SWEEP_START_BOUNDARY; s.jc = -s.before; }
    else if (p.seams && c > 0 && s.count >= p.J && sweep_column_count(p, c - 1) >= p.J) { s.kind = SWEEP_START_SEAM; s.jc = 0; }
    else { s.kind = SWEEP_START_WARM; s.jc = -p.J; }
    return s;
}

// The two wave-uniform figures in closed form (a kernel wants no loop over the columns; the test holds them against
// sweep_column).  The columns that start at a seam are c0 .. c1: with ow = 0, before = c Lseg > J first holds at c0 = 1, or 2
// where Lseg == J; count >= J holds up to c1 = (Tw - J) / Lseg, and implies Lseg >= J, which is the neighbour's count.
PYVB_HD static inline void sweep_seam_columns(const SweepPart& p, int& c0, int& c1) {
    c0 = 1; c1 = 0;
    if (!p.seams || p.Tw < p.J || p.Lseg < p.J || p.Lseg <= 0) return;
    c0 = p.Lseg > p.J ? 1 : 2;
    c1 = (p.Tw - p.J) / p.Lseg;
    c1 = c1 < SWEEP_COLUMNS - 1 ? c1 : SWEEP_COLUMNS - 1;
}

// first loop index of the wavefront: the earliest of its columns'.  Without seams that is the last column's, -min(J, before);
// with them, -J if a column before c0 or behind c1 warms up (column 0 never does), else 0.
PYVB_HD static inline int sweep_first_step(const SweepPart& p) {
    int c0, c1;
    sweep_seam_columns(p, c0, c1);
    const int last = p.ow + (SWEEP_COLUMNS - 1) * p.Lseg;
    if (c0 > c1) return -(p.J < last ? p.J : last);
    return (c0 > 1 || c1 < SWEEP_COLUMNS - 1) ? -p.J : 0;
}

// steps of the correction loop behind the main loop: J if any column starts at a seam, else none
PYVB_HD static inline int sweep_correction_steps(const SweepPart& p) {
    int c0, c1;
    sweep_seam_columns(p, c0, c1);
    return c0 <= c1 ? p.J : 0;
}

// does column s of part p work on a node at loop index j?
PYVB_HD static inline bool sweep_active(const SweepPart& p, const SweepColumn& s, int j) {
    return j >= s.jc && j < p.Lseg && (s.before - p.ow) + j < p.Tw;
}
