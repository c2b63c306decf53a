// The chained plan of a stream cut into segments (cjs_bz2_compress_multi) or slices (compress_overlapped): where the block
// boundaries fall inside a piece that is planned as an input of its own.  The integer arithmetic of compressjs_amd/dist.py
// (plan_bases, chain_step), restated; pure host code, no HIP call.
#pragma once
#include "cjs_common.h"

namespace cjs {
struct MSeg {
    uint64_t lo = 0, e = 0;         // the segment's bytes [lo, e) (absolute input offsets)
    uint64_t cost = 0;              // RLE1 cost of its bytes, scanned as an input of its own
    u32 phase = 0;                  // block boundaries lie where the slice's own cost prefix reaches phase + m * cap - while no boundary in front of the segment moved
    uint64_t base = 0;              // origin of the segment's own cost prefix in the stream's: G(lo + i) = base + C_own(i) beyond the head run
    bool has_span = false;          // a run of four or more bytes straddles the segment's start: its cost span [c0, c1] from the run's first byte
    uint64_t c0 = 0, c1 = 0;        //   (the own prefix is wrong inside it: a boundary target in there cannot be planned by this segment)
    uint64_t t0 = 0, tnext = 0;     // round 6, the chained plan: the target the segment was planned from, the one it hands on
    int64_t nb = 0;                 // blocks that start in the segment
    u32 first_blk = 0;              // the first of them in the context's plan (the replicated plan: every context holds all blocks)
    bool ok = true;                 // can be planned on its own
    uint64_t bits = 0, off = 0;
    u32 fold = 0, count = 0;
    u8* dseg = nullptr;             // device: the segment's bit stream from bit 0
    uint64_t dseg_cap = 0;
    u8 first = 0, last = 0;         // seam bytes (shifted)
};
static inline u32 rotl32(u32 v, u32 k) { k &= 31u; return k ? (v << k) | (v >> (32u - k)) : v; }
// RLE1 output bytes of the first k bytes of a fresh run (k0_g in k0_rle1.hip)
static inline uint64_t rle1_g(uint64_t k) { const uint64_t q = k / 255u, r = k % 255u; return 5u * q + (r < 4u ? r : 5u); }
// first and last run of in[lo, e), from its first / last 4096 bytes; long_run: a boundary run that reaches beyond them
struct EdgeRuns { int hb = -1, tb = -1; uint64_t lh = 0, lt = 0; bool long_run = false; };
static inline EdgeRuns edge_runs(const uint8_t* in, uint64_t lo, uint64_t e) {
    EdgeRuns r;
    const uint64_t n = e - lo, EDGE = 4096;
    if (!n) return r;
    const uint64_t hn = n < EDGE ? n : EDGE;
    r.hb = in[lo]; r.tb = in[e - 1];
    while (r.lh < hn && in[lo + r.lh] == (uint8_t)r.hb) r.lh++;
    while (r.lt < hn && in[e - 1 - r.lt] == (uint8_t)r.tb) r.lt++;
    r.long_run = (r.lh == hn && n > hn) || (r.lt == hn && n > hn);
    return r;
}
// compressjs_amd/dist.py:plan_bases for one more segment: G = cost prefix of the stream at the segment's start, (inb, ink) = the
// run that reaches it from the left
struct PlanChain { uint64_t G = 0; int inb = -1; uint64_t ink = 0; };
static inline void plan_base(PlanChain& P, MSeg& g, const EdgeRuns& r, u32 cap) {
    const uint64_t n = g.e - g.lo;
    g.ok = !r.long_run;
    int64_t delta = 0;
    if (n && P.inb == r.hb && P.ink > 0) {
        delta = (int64_t)rle1_g(P.ink + r.lh) - (int64_t)rle1_g(P.ink) - (int64_t)rle1_g(r.lh);      // the head run costs what the tail of a longer run costs
        if (P.ink + r.lh >= 4) {
            // a run of four or more bytes straddles the cut: no block boundary may fall into its cost span, measured from the run's first byte
            // (round 6: checked against the target the chain actually carries to this segment - seg_target - not against multiples of cap)
            g.has_span = true;
            g.c0 = P.G - rle1_g(P.ink);
            g.c1 = P.G + rle1_g(P.ink + r.lh) - rle1_g(P.ink);
        }
    }
    const uint64_t base = (uint64_t)((int64_t)P.G + delta);
    g.base = base;
    g.phase = (u32)((cap - base % cap) % cap);
    if (n) {
        if (r.lh == n && P.inb == r.hb && P.ink > 0) P.ink += n;       // the whole segment continues the incoming run
        else if (r.lh == n) { P.inb = r.hb; P.ink = n; }
        else { P.inb = r.tb; P.ink = r.lt; }
    }
    P.G = (uint64_t)((int64_t)P.G + (int64_t)g.cost + delta);
}
// The chained plan (compressjs_amd/dist.py: chain_step): tau = the stream-wide target of the first block boundary at or behind the
// segment's start (what the segment before it handed on; 0 for the first).  Sets g.t0, the same target under the segment's own origin;
// false when the boundary falls into a run that straddles the segment's start (the segment cannot plan it: the caller falls back).
static inline bool seg_target(MSeg& g, uint64_t tau) {
    if (g.has_span && tau >= g.c0 && tau <= g.c1) return false;
    g.t0 = tau > g.base ? tau - g.base : 0;
    return true;
}
}
