// K6: inverse of the linear BWT, BWT.unbwtransform (lib/BWT.js:352-363), for gfx950.
//
// The reference walks the LF chain serially:  t = 0; for i = n-1 .. 0: U[i] = T[t];
// t = LF[t] + C[T[t]]; if (t < pidx) t++.   Here:
//   k6_hist / k6_scan   per-tile byte counts -> C[] and the tile offsets (a stable counting sort)
//   k6_next             next(t) = LF[t] + C[T[t]] (+1 below pidx) with wave-ballot ranks, and the
//                       inverse links pred[next[t]] = t (injective except for the last position of
//                       the chain, whose successor is the sentinel row and is skipped)
//   k6_jump x log2(n)   Wyllie list ranking towards node 0 over pred: R[t] = index of t in the chain
//   k6_emit             U[n-1-R[t]] = T[t]
// k6_unbwt_linear: one block per launch set.  k6_unbwt_batch: the same kernels over MANY blocks at once (the k6b_* wrappers:
// blockIdx.y = the block, taken from a K6Blk row), for the batched BWTC decoder and cjs_unbwt_linear_batch.
#include "pipeline.h"

#define K6_TILE 4096

// (the bodies take the tile / the 256-element piece `bx` of ONE block: the single and the batched kernels share them)
__device__ __forceinline__ void k6_hist_body(const u8* T, u32 n, u32* tileHist, u32 bx) {
    __shared__ u32 h[256];
    const u32 tid = threadIdx.x;
    h[tid] = 0;
    __syncthreads();
    const u32 t0 = bx * K6_TILE;
    for (int k = 0; k < 16; k++) {
        const u32 i = t0 + k * 256u + tid;
        if (i < n) atomicAdd(&h[T[i]], 1u);
    }
    __syncthreads();
    tileHist[(size_t)bx * 256 + tid] = h[tid];
}
__global__ __launch_bounds__(256) void k6_hist(const u8* T, u32 n, u32* tileHist) { k6_hist_body(T, n, tileHist, blockIdx.x); }

// digit-major exclusive offsets: tileHist[t][c] <- C[c] + sum_{t' < t} count[t'][c]
__device__ __forceinline__ void k6_scan_body(u32* tileHist, u32 ntiles) {
    __shared__ u32 sh[256];
    const u32 c = threadIdx.x;
    u32 tot = 0;
    for (u32 t = 0; t < ntiles; t++) tot += tileHist[(size_t)t * 256 + c];
    const u32 base = block_excl_scan_256(tot, sh);
    u32 run = base;
    for (u32 t = 0; t < ntiles; t++) {
        const u32 v = tileHist[(size_t)t * 256 + c];
        tileHist[(size_t)t * 256 + c] = run;
        run += v;
    }
}
__global__ __launch_bounds__(256) void k6_scan(u32* tileHist, u32 ntiles) { k6_scan_body(tileHist, ntiles); }

// RAW = false: inverse links pred[next(t)] = t for the list ranking.  RAW = true: the successor map itself,
// nxt[t] = LF[t] + C[T[t]] (+1 below pidx), exactly what the reference's loop computes (may be n): only for the
// serial fallback below.
template <bool RAW>
__device__ __forceinline__ void k6_next_body(const u8* T, u32 n, u32 pidx, const u32* tileHist, u32* pred, u32 bx) {
    __shared__ u32 wh[4][256];
    const u32 tid = threadIdx.x, w = tid >> 6, lane = tid & 63u;
    for (u32 i = tid; i < 1024; i += 256) (&wh[0][0])[i] = 0;
    __syncthreads();
    const u32 t0 = bx * K6_TILE;
    const u64 lt = lanemask_lt();
    u32 rk[16], cv[16];
#pragma unroll
    for (int it = 0; it < 16; it++) {                      // stable rank of every byte inside its wave's range
        const u32 i = t0 + w * 1024u + it * 64u + lane;
        const bool valid = i < n;
        const u32 c = valid ? T[i] : 0u;
        const u64 m = match_any(c, 8, valid);
        const u32 rank = (u32)__popcll(m & lt), cnt = (u32)__popcll(m);
        const u32 prior = valid ? wh[w][c] : 0u;
        __builtin_amdgcn_wave_barrier();
        if (valid && rank == 0) wh[w][c] = prior + cnt;
        __builtin_amdgcn_wave_barrier();
        rk[it] = prior + rank;
        cv[it] = c;
    }
    __syncthreads();
    {
        u32 o = tileHist[(size_t)bx * 256 + tid];
        for (int ww = 0; ww < 4; ww++) { const u32 c = wh[ww][tid]; wh[ww][tid] = o; o += c; }
    }
    __syncthreads();
#pragma unroll
    for (int it = 0; it < 16; it++) {
        const u32 i = t0 + w * 1024u + it * 64u + lane;
        if (i < n) {
            u32 t = wh[w][cv[it]] + rk[it];                // LF[i] + C[T[i]] = (full row of the predecessor) - 1
            // Row pidx of the full (n+1)-row matrix holds the sentinel: the position that maps onto
            // it is the END of the chain (its successor is never used by the reference loop), every
            // other successor is unique.
            const bool last = t + 1u == pidx;
            if (t < pidx) t++;
            if (RAW) pred[i] = t;
            else if (!last && t < n) pred[t] = i;
        }
    }
}
template <bool RAW>
__global__ __launch_bounds__(256) void k6_next(const u8* T, u32 n, u32 pidx, const u32* tileHist, u32* pred) {
    k6_next_body<RAW>(T, n, pidx, tileHist, pred, blockIdx.x);
}

// A position nothing links to (pred still ~0: only possible for a (T, pidx) pair no BWT produces) becomes a
// self-loop of rank n; ranks saturate at n, so exactly the positions on the chain that starts at node 0 end up
// with R < n, all distinct.
__device__ __forceinline__ void k6_init_body(u32 n, const u32* pred, u32* P, u32* R, u32 bx) {
    const u32 t = bx * 256u + threadIdx.x;
    if (t >= n) return;
    const u32 p = pred[t];
    P[t] = t == 0 ? 0u : (p == 0xFFFFFFFFu ? t : p);
    R[t] = t == 0 ? 0u : (p == 0xFFFFFFFFu ? n : 1u);
}
__device__ __forceinline__ void k6_jump_body(u32 n, const u32* Pin, const u32* Rin, u32* Pout, u32* Rout, u32 bx) {
    const u32 t = bx * 256u + threadIdx.x;
    if (t >= n) return;
    const u32 p = Pin[t];
    const u32 r = Rin[t] + Rin[p];
    Rout[t] = r < n ? r : n;
    Pout[t] = Pin[p];
}
__device__ __forceinline__ void k6_emit_body(const u8* T, u32 n, const u32* R, u8* U, u32* onChain, u32 bx) {
    const u32 t = bx * 256u + threadIdx.x;
    const u32 r = t < n ? R[t] : n;
    if (r < n) U[n - 1u - r] = T[t];
    const u64 bal = __ballot(r < n);
    if ((threadIdx.x & 63u) == 0 && bal) atomicAdd(onChain, (u32)__popcll(bal));
}
__global__ __launch_bounds__(256) void k6_init(u32 n, const u32* pred, u32* P, u32* R) { k6_init_body(n, pred, P, R, blockIdx.x); }
__global__ __launch_bounds__(256) void k6_jump(u32 n, const u32* Pin, const u32* Rin, u32* Pout, u32* Rout) { k6_jump_body(n, Pin, Rin, Pout, Rout, blockIdx.x); }
__global__ __launch_bounds__(256) void k6_emit(const u8* T, u32 n, const u32* R, u8* U, u32* onChain) { k6_emit_body(T, n, R, U, onChain, blockIdx.x); }
// The LF mapping of a real BWT is one cycle through all n positions.  For any other (T, pidx) the reference's
// loop (lib/BWT.js:359-362) still takes n steps from t = 0: this kernel repeats it literally (one lane).  When t
// leaves [0, n) the reference's arithmetic turns to NaN and every remaining U[i] = T[NaN] stores 0.
__device__ __forceinline__ void k6_serial_body(const u8* T, u32 n, const u32* nxt, u8* U) {
    u32 t = 0;
    bool dead = false;
    for (u32 i = n; i-- > 0;) {
        if (dead) { U[i] = 0; continue; }
        U[i] = T[t];
        t = nxt[t];
        if (t >= n) dead = true;
    }
}
__global__ void k6_serial(const u8* T, u32 n, const u32* nxt, u8* U) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    k6_serial_body(T, n, nxt, U);
}

// device pointers; ws needs 5*n*4 + ntiles*1024 + 256 bytes
int k6_unbwt_linear(const u8* dT, u8* dU, u32 n, u32 pidx, void* ws, hipStream_t stream) {
    const u32 ntiles = (n + K6_TILE - 1) / K6_TILE, nb = (n + 255) / 256;
    u32* pred = (u32*)ws;
    u32* P0 = pred + n; u32* R0 = P0 + n; u32* P1 = R0 + n; u32* R1 = P1 + n;
    u32* tileHist = R1 + n;
    u32* onChain = tileHist + (size_t)ntiles * 256;
    HIP_CHECK_RET(hipMemsetAsync(pred, 0xFF, (size_t)n * 4, stream));
    HIP_CHECK_RET(hipMemsetAsync(onChain, 0, 4, stream));
    hipLaunchKernelGGL(k6_hist, dim3(ntiles), dim3(256), 0, stream, dT, n, tileHist);
    hipLaunchKernelGGL(k6_scan, dim3(1), dim3(256), 0, stream, tileHist, ntiles);
    hipLaunchKernelGGL(k6_next<false>, dim3(ntiles), dim3(256), 0, stream, dT, n, pidx, (const u32*)tileHist, pred);
    hipLaunchKernelGGL(k6_init, dim3(nb), dim3(256), 0, stream, n, (const u32*)pred, P0, R0);
    u32 *Pi = P0, *Ri = R0, *Po = P1, *Ro = R1;
    for (u32 span = 1; span < n; span <<= 1) {
        hipLaunchKernelGGL(k6_jump, dim3(nb), dim3(256), 0, stream, n, (const u32*)Pi, (const u32*)Ri, Po, Ro);
        u32* t = Pi; Pi = Po; Po = t; t = Ri; Ri = Ro; Ro = t;
    }
    hipLaunchKernelGGL(k6_emit, dim3(nb), dim3(256), 0, stream, dT, n, (const u32*)Ri, dU, onChain);
    u32 got = 0;
    HIP_CHECK_RET(hipMemcpyAsync(&got, onChain, 4, hipMemcpyDeviceToHost, stream));
    HIP_CHECK_RET(hipStreamSynchronize(stream));
    if (got != n) {
        // not one n-cycle (corrupt BWTC stream, or a caller's arbitrary (T, pidx)): the reference's walk, literally
        hipLaunchKernelGGL(k6_next<true>, dim3(ntiles), dim3(256), 0, stream, dT, n, pidx, (const u32*)tileHist, pred);
        hipLaunchKernelGGL(k6_serial, dim3(1), dim3(64), 0, stream, dT, n, (const u32*)pred, dU);
    }
    HIP_CHECK_RET(hipGetLastError());
    return CJS_OK;
}

// ---- many blocks at once ---------------------------------------------------------------------------
// Block k of a group is row B[k]: T + tAt, U + uAt (its FINAL place: k6_emit writes there), and its own slice of the group's
// workspace at ws + wsAt (u32 units), laid out as k6_unbwt_linear's.  blockIdx.y = k; blockIdx.x runs to what the group's LONGEST
// block needs, the workgroups beyond a shorter block's own count leave at once.  Every kernel is uniform per workgroup.
struct K6View { const u8* T; u8* U; u32 n, pidx, ntiles; u32 *pred, *P0, *R0, *P1, *R1, *tileHist, *onChain; };
__device__ __forceinline__ K6View k6_view(const K6Blk* B, const u8* T, u8* U, u32* ws) {
    const K6Blk b = B[blockIdx.y];
    K6View v;
    v.T = T + b.tAt; v.U = U + b.uAt; v.n = b.n; v.pidx = b.pidx;
    v.ntiles = (b.n + K6_TILE - 1) / K6_TILE;
    v.pred = ws + b.wsAt;
    v.P0 = v.pred + b.n; v.R0 = v.P0 + b.n; v.P1 = v.R0 + b.n; v.R1 = v.P1 + b.n;
    v.tileHist = v.R1 + b.n;
    v.onChain = v.tileHist + (size_t)v.ntiles * 256;
    return v;
}
__global__ __launch_bounds__(256) void k6b_hist(const K6Blk* B, const u8* T, u8* U, u32* ws) {
    const K6View v = k6_view(B, T, U, ws);
    if (blockIdx.x == 0 && threadIdx.x == 0) *v.onChain = 0u;
    if (blockIdx.x >= v.ntiles) return;
    k6_hist_body(v.T, v.n, v.tileHist, blockIdx.x);
}
__global__ __launch_bounds__(256) void k6b_scan(const K6Blk* B, const u8* T, u8* U, u32* ws) {
    const K6View v = k6_view(B, T, U, ws);
    k6_scan_body(v.tileHist, v.ntiles);
}
// RAW: only the blocks whose chain did not cover them (onChain != n after k6b_emit) do work
template <bool RAW>
__global__ __launch_bounds__(256) void k6b_next(const K6Blk* B, const u8* T, u8* U, u32* ws) {
    const K6View v = k6_view(B, T, U, ws);
    if (blockIdx.x >= v.ntiles) return;
    if (RAW && *v.onChain == v.n) return;
    k6_next_body<RAW>(v.T, v.n, v.pidx, v.tileHist, v.pred, blockIdx.x);
}
__global__ __launch_bounds__(256) void k6b_fill(const K6Blk* B, const u8* T, u8* U, u32* ws) {   // pred = ~0 (k6_unbwt_linear's memset)
    const K6View v = k6_view(B, T, U, ws);
    const u32 t = blockIdx.x * 256u + threadIdx.x;
    if (t < v.n) v.pred[t] = 0xFFFFFFFFu;
}
__global__ __launch_bounds__(256) void k6b_init(const K6Blk* B, const u8* T, u8* U, u32* ws) {
    const K6View v = k6_view(B, T, U, ws);
    k6_init_body(v.n, v.pred, v.P0, v.R0, blockIdx.x);
}
// round r of the list ranking (span 2^r); a block that needs fewer rounds than the group's longest sits the rest out, its result
// stays in the buffer pair its own last round wrote (k6b_emit picks it by the same count)
__device__ __forceinline__ u32 k6_rounds(u32 n) { u32 r = 0; for (u32 span = 1; span < n; span <<= 1) r++; return r; }
__global__ __launch_bounds__(256) void k6b_jump(const K6Blk* B, const u8* T, u8* U, u32* ws, u32 round) {
    const K6View v = k6_view(B, T, U, ws);
    if (round >= k6_rounds(v.n) || blockIdx.x * 256u >= v.n) return;
    if (round & 1u) k6_jump_body(v.n, v.P1, v.R1, v.P0, v.R0, blockIdx.x);
    else k6_jump_body(v.n, v.P0, v.R0, v.P1, v.R1, blockIdx.x);
}
__global__ __launch_bounds__(256) void k6b_emit(const K6Blk* B, const u8* T, u8* U, u32* ws) {
    const K6View v = k6_view(B, T, U, ws);
    if (blockIdx.x * 256u >= v.n) return;
    k6_emit_body(v.T, v.n, (k6_rounds(v.n) & 1u) ? v.R1 : v.R0, v.U, v.onChain, blockIdx.x);
}
__global__ __launch_bounds__(64) void k6b_serial(const K6Blk* B, const u8* T, u8* U, u32* ws, u32 nblk) {
    const u32 k = blockIdx.x * 64u + threadIdx.x;
    if (k >= nblk) return;
    const K6Blk b = B[k];
    const u32 ntiles = (b.n + K6_TILE - 1) / K6_TILE;
    u32* pred = ws + b.wsAt;
    if (pred[(size_t)5 * b.n + (size_t)ntiles * 256] == b.n) return;       // onChain: one n-cycle, k6b_emit has written it
    k6_serial_body(T + b.tAt, b.n, pred, U + b.uAt);
}

size_t k6_ws_words(u32 n) { return (size_t)n * 5 + ((size_t)(n + K6_TILE - 1) / K6_TILE) * 256 + 64; }

// d_B: `nblk` rows (device) of blocks with n >= 1 and pidx <= n, their wsAt disjoint inside ws; max_n = the longest of them.
// No host wait: a block that is not one n-cycle is walked by k6b_serial in the same sequence of launches.
int k6_unbwt_batch(const K6Blk* d_B, u32 nblk, u32 max_n, const u8* dT, u8* dU, void* ws, hipStream_t stream) {
    if (nblk == 0 || max_n == 0) return CJS_OK;
    if (nblk > K6_GROUP_MAX) return CJS_E_ARG;
    const u32 mt = (max_n + K6_TILE - 1) / K6_TILE, mb = (max_n + 255) / 256;
    u32* w = (u32*)ws;
    hipLaunchKernelGGL(k6b_fill, dim3(mb, nblk), dim3(256), 0, stream, d_B, dT, dU, w);
    hipLaunchKernelGGL(k6b_hist, dim3(mt, nblk), dim3(256), 0, stream, d_B, dT, dU, w);
    hipLaunchKernelGGL(k6b_scan, dim3(1, nblk), dim3(256), 0, stream, d_B, dT, dU, w);
    hipLaunchKernelGGL(k6b_next<false>, dim3(mt, nblk), dim3(256), 0, stream, d_B, dT, dU, w);
    hipLaunchKernelGGL(k6b_init, dim3(mb, nblk), dim3(256), 0, stream, d_B, dT, dU, w);
    u32 round = 0;
    for (u32 span = 1; span < max_n; span <<= 1, round++)
        hipLaunchKernelGGL(k6b_jump, dim3(mb, nblk), dim3(256), 0, stream, d_B, dT, dU, w, round);
    hipLaunchKernelGGL(k6b_emit, dim3(mb, nblk), dim3(256), 0, stream, d_B, dT, dU, w);
    hipLaunchKernelGGL(k6b_next<true>, dim3(mt, nblk), dim3(256), 0, stream, d_B, dT, dU, w);
    hipLaunchKernelGGL(k6b_serial, dim3((nblk + 63u) / 64u), dim3(64), 0, stream, d_B, dT, dU, w, nblk);
    HIP_CHECK_RET(hipGetLastError());
    return CJS_OK;
}
