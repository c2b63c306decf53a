// K0 device helpers shared by the single-stream plan (k0_rle1.hip) and the batched plan (k0_docs.hip): the RLE1 cost
// functions, 16-byte tile loads, run starts inside a tile, and the workgroup-cooperative C(i) / search / run-end walks.
// Moved here from k0_rle1.hip, where the scheme is described: the text is the same, except that k0_evalC, k0_searchC and
// k0_run_end are `static` now (the header is included by two translation units).
#pragma once
#include "pipeline.h"
#include "devutil.h"

#define K0_TILE 4096
#define K0_NONE 0ull          // boundary positions are stored +1 so that 0 means "none"

__device__ __forceinline__ u32 k0_g(u64 k) {          // output bytes before the k-th byte of a fresh run
    const u64 q = k / 255u;
    const u32 r = (u32)(k - q * 255u);
    return (u32)(5u * q) + (r < 4u ? r : 5u);
}
__device__ __forceinline__ u32 k0_c(u64 k) {
    const u32 sub = (u32)(k % 255u);
    return sub < 3u ? 1u : (sub == 3u ? 2u : 0u);
}

// ---- per-tile: last run boundary (position j with j == 0 or in[j] != in[j-1]), stored +1 -------
// 16 consecutive input bytes of a thread: one 16-byte load when the address allows it
__device__ __forceinline__ void load16(const K0Buf& K, u64 j0, u8* b) {
    if (j0 + 16u <= K.in_len && ((((uintptr_t)K.in) + j0) & 15u) == 0) {
        const uint4 v = *(const uint4*)(K.in + j0);
        const u32 w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int k = 0; k < 16; k++) b[k] = (u8)(w[k >> 2] >> (8 * (k & 3)));
    } else {
#pragma unroll
        for (int k = 0; k < 16; k++) b[k] = j0 + k < K.in_len ? K.in[j0 + k] : 0;
    }
}

// ---- in-tile helper: every thread owns 16 consecutive bytes of tile t ----------------------------
// Returns, for the thread's first byte, the start of its run (global, uncut), given the tile's
// incoming run start rs_in.  `sh` is 256 u64 of LDS.  Also returns the bytes in b[16].
// hm: bit k = the thread's k-th byte exists (is below in_len) and starts a run.  Everything inside is tile-relative and 32 bits wide
// (round 6: 64-bit positions per byte - compares, the max-scan's shuffles - were a third of the instructions of the kernels that call it).
__device__ __forceinline__ u64 tile_runstarts(const K0Buf& K, u64 t, u64 rs_in, u8* b, u64* sh, u32& hm) {
    const u32 tid = threadIdx.x;
    const u64 j0 = t * K0_TILE + tid * 16u;
    u8 prev = 0;
    if (j0 > 0 && j0 - 1 < K.in_len) prev = K.in[j0 - 1];
    load16(K, j0, b);
    const u32 nv = j0 >= K.in_len ? 0u : (K.in_len - j0 < 16u ? (u32)(K.in_len - j0) : 16u);   // bytes of the thread that exist
    u32 heads = (j0 == 0 || b[0] != prev) ? 1u : 0u;
#pragma unroll
    for (int k = 1; k < 16; k++) heads |= b[k] != b[k - 1] ? 1u << k : 0u;
    heads &= (1u << nv) - 1u;
    hm = heads;
    // 1 + tile-relative index of the thread's last run start, 0 = none; exclusive max-scan over the 256 threads: shuffles inside a wave, one LDS hop across the 4 waves
    u32 v = heads ? tid * 16u + 32u - (u32)__clz((int)heads) : 0u;
    const u32 lane = tid & 63u, w = tid >> 6;
    u32* sh32 = (u32*)sh;
    for (u32 off = 1; off < 64; off <<= 1) {
        const u32 u = (u32)__shfl_up((int)v, off);
        if (lane >= off && u > v) v = u;
    }
    if (lane == 63u) sh32[w] = v;
    __syncthreads();
    u32 before = (u32)__shfl_up((int)v, 1u);              // inclusive of the previous lane = exclusive here
    if (lane == 0) before = 0;
    for (u32 ww = 0; ww < w; ww++) if (sh32[ww] > before) before = sh32[ww];
    __syncthreads();
    return before ? t * K0_TILE + before - 1u : rs_in;
}
__device__ __forceinline__ u64 tile_runstarts(const K0Buf& K, u64 t, u64 rs_in, u8* b, u64* sh) {
    u32 hm;
    return tile_runstarts(K, t, rs_in, b, sh, hm);
}
__device__ __forceinline__ u32 k0_mod255(u64 d) { return (d >> 32) ? (u32)(d % 255u) : (u32)d % 255u; }

// ---- C(i) for an arbitrary position; workgroup-cooperative (256 threads), all threads get it ---
static __device__ u64 k0_evalC(const K0Buf& K, u64 i, u64* sh, u32* sh32) {
    if (i >= K.in_len) return K.tileC[K.ntiles];           // total
    const u64 t = i / K0_TILE;
    const u64 rsin_raw = K.tileA[t];
    const u64 rs_in = rsin_raw != K0_NONE ? rsin_raw - 1 : 0;
    u8 b[16];
    u64 rs = tile_runstarts(K, t, rs_in, b, sh);
    const u64 j0 = t * K0_TILE + threadIdx.x * 16u;
    if (threadIdx.x == 0) sh32[0] = 0;
    __syncthreads();
    u32 c = 0;
    for (int k = 0; k < 16; k++) {
        const u64 j = j0 + k;
        if (j >= i) break;
        if (k == 0 ? (j == 0 || K.in[j - 1] != b[0]) : (b[k] != b[k - 1])) rs = j;
        c += k0_c(j - rs);
    }
    if (c) atomicAdd(&sh32[0], c);
    __syncthreads();
    const u64 r = K.tileC[t] + sh32[0];
    __syncthreads();
    return r;
}

// smallest i in (from, in_len] with C(i) >= target, or in_len+1 when the total is below target
static __device__ u64 k0_searchC(const K0Buf& K, u64 target, u64 from, u64* sh, u32* sh32, u64* c_at) {
    const u32 tid = threadIdx.x;
    u64 lo = from / K0_TILE, hi = K.ntiles;                // tiles [lo, hi); Ctile[lo] <= C(from) < target
    while (hi - lo > 256) {
        const u64 step = (hi - lo + 255) / 256;
        const u64 p = lo + (u64)tid * step;
        if (tid == 0) sh32[0] = 0;
        __syncthreads();
        if (p < hi && K.tileC[p] < target) atomicAdd(&sh32[0], 1u);
        __syncthreads();
        const u32 cnt = sh32[0];                          // >= 1 because Ctile[lo] < target
        __syncthreads();
        const u64 nlo = lo + (u64)(cnt - 1) * step;
        hi = nlo + step < hi ? nlo + step : hi;
        lo = nlo;
    }
    if (tid == 0) sh32[0] = 0;
    __syncthreads();
    if (lo + tid < hi && K.tileC[lo + tid] < target) atomicAdd(&sh32[0], 1u);
    __syncthreads();
    const u64 t = lo + sh32[0] - 1;
    __syncthreads();
    // inside tile t
    const u64 rsin_raw = K.tileA[t];
    const u64 rs_in = rsin_raw != K0_NONE ? rsin_raw - 1 : 0;
    u8 b[16];
    u64 rs = tile_runstarts(K, t, rs_in, b, sh);
    const u64 j0 = t * K0_TILE + tid * 16u;
    u32 cs[16], mine = 0;
    for (int k = 0; k < 16; k++) {
        const u64 j = j0 + k;
        cs[k] = 0;
        if (j >= K.in_len) continue;
        if (k == 0 ? (j == 0 || K.in[j - 1] != b[0]) : (b[k] != b[k - 1])) rs = j;
        cs[k] = k0_c(j - rs);
        mine += cs[k];
    }
    // exclusive scan of `mine` over the 256 threads
    u32* s32 = (u32*)sh;
    s32[tid] = mine;
    __syncthreads();
    for (u32 off = 1; off < 256; off <<= 1) {
        u32 tv = 0;
        if (tid >= off) tv = s32[tid - off];
        __syncthreads();
        if (tid >= off) s32[tid] += tv;
        __syncthreads();
    }
    u64 run = K.tileC[t] + (tid ? s32[tid - 1] : 0);
    __syncthreads();
    unsigned long long* best = (unsigned long long*)sh;
    if (tid == 0) best[0] = ~0ull;
    __syncthreads();
    u64 myhit = ~0ull, myrun = 0;
    for (int k = 0; k < 16; k++) {
        const u64 j = j0 + k;
        if (j >= K.in_len) break;
        run += cs[k];
        if (run >= target && j + 1 > from) {
            myhit = j + 1; myrun = run;
            atomicMin(&best[0], (unsigned long long)(j + 1));
            break;
        }
    }
    __syncthreads();
    const u64 r = best[0];
    if (r != ~0ull && myhit == r) best[1] = myrun;        // C(r), published by the thread that found it
    __syncthreads();
    *c_at = best[1];
    __syncthreads();
    return r == ~0ull ? K.in_len + 1 : r;
}

// first position > s whose byte differs from in[s] (the end of s's run), or in_len
static __device__ u64 k0_run_end(const K0Buf& K, u64 s, u64* sh) {
    const u32 tid = threadIdx.x;
    const u8 c = K.in[s];
    unsigned long long* best = (unsigned long long*)sh;
    u64 t = s / K0_TILE;
    for (;;) {
        if (tid == 0) best[0] = ~0ull;
        __syncthreads();
        const u64 j0 = t * K0_TILE + tid * 16u;
        for (int k = 0; k < 16; k++) {
            const u64 j = j0 + k;
            if (j > s && j < K.in_len && K.in[j] != c) { atomicMin(&best[0], (unsigned long long)j); break; }
        }
        __syncthreads();
        const u64 r = best[0];
        __syncthreads();
        if (r != ~0ull) return r;
        // skip tiles that contain no boundary at all
        t++;
        for (;;) {
            if (t >= K.ntiles) return K.in_len;
            if (tid == 0) best[0] = ~0ull;
            __syncthreads();
            const u64 tt = t + tid;
            // tileB[tt] = last boundary (+1) inside tile tt (unscanned copy)
            if (tt < K.ntiles && K.tileB[tt] != K0_NONE) atomicMin(&best[0], (unsigned long long)tt);
            __syncthreads();
            const u64 ft = best[0];
            __syncthreads();
            if (ft != ~0ull) { t = ft; break; }
            t += 256;
        }
    }
}
