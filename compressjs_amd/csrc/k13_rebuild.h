// DefSumModel's rebuild (lib/DefSumModel.js:54-80) wave-wide, shared by the encoder's model (k13_defsum_model.hip) and the decoder
// (k14_defsum_decoder.hip).  prob[], esc[] and upd[] sit in LDS (K13_TAB u32 each).
#pragma once
#include "cjs_common.h"
#include "devutil.h"

#define K13_TAB 264u                   // >= numSyms + 2 = alphabetSize + 3 <= 259
#define K13_MAX_ESC 40u                // MAX_ESCAPE_COUNT  lib/DefSumModel.js:9

// A wave-uniform call over the size + 1 <= 258 entries, 64 a round: newProb = (p >> 1) + update, the cumulative probability from
// a DPP scan, the cumulative escape index and the odd count from ballots.  uesc is update[ESCAPE] (kept in a register by both
// callers), ESCAPE = size.  Leaves upd[] zeroed and prob[size + 1] = the sum (:71, always 256).  -> the new updateThresh (:74)
__device__ __forceinline__ u32 k13_rebuild(u32* prob, u32* esc, u32* upd, u32 size, u32 uesc, u32 lane, u64 lt_lanes) {
    __builtin_amdgcn_wave_barrier();
    u32 cum = 0u, cume = 0u, odd = 0u;
    for (u32 r = 0; r * 64u <= size; r++) {
        const u32 i = r * 64u + lane;
        const bool v = i <= size;
        const u32 ii = v ? i : 0u;
        const u32 np = v ? ((prob[ii + 1u] - prob[ii]) >> 1) + (i == size ? uesc : upd[ii]) : 0u;
        const u32 inc = wave_incl_scan_dpp(np);
        const u64 dead = __ballot(v && np == 0u);
        const u64 oddm = __ballot((np & 1u) != 0u);
        if (v) { prob[i] = cum + inc - np; esc[i] = cume + (u32)__popcll(dead & lt_lanes); upd[i] = 0u; }
        cum += (u32)__builtin_amdgcn_readlane((int)inc, 63);
        cume += (u32)__popcll(dead);
        odd += (u32)__popcll(oddm);
    }
    if (lane == 0) prob[size + 1u] = cum;                     // :71 (= 256)
    __builtin_amdgcn_wave_barrier();
    return 256u - (cum - odd) / 2u;                           // :74
}
