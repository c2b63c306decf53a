// The packed FenwickModel tree in LDS, shared by the encoder's model (k10_bwtc_model.hip) and the decoder (k12_bwtc_decoder.hip).
#pragma once
#include "cjs_common.h"

#define K10_MAXSYM 260

__device__ __forceinline__ void k10_sum_tree(u32* tree, u32 numSyms, u32 lane) {      // lib/FenwickModel.js:167-172
    // tree[i] = tree[2i] + tree[2i+1] for i = numSyms-1 .. 1: children have a longer bit length, so go level by level
    for (int bl = 9; bl >= 1; bl--) {
        const u32 lo = 1u << (bl - 1), hi = (1u << bl) < numSyms ? (1u << bl) : numSyms;
        for (u32 i = lo + lane; i < hi; i += 64u) tree[i] = tree[2u * i] + tree[2u * i + 1u];
        __builtin_amdgcn_wave_barrier();
    }
}
