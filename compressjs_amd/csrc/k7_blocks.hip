// K7 for a list of block requests (cjs_bz2_decompress_blocks, decode.hip: dec_blocks): what Bunzip.decodeBlock (lib/Bzip2.js:482-503)
// does in front of the block itself, for N bit positions of one staged stream at once.  The reference seeks to the position and reads
// 48 bits (_get_next_block, :154-161): the block magic, the end-of-stream magic, or 'Not bzip data'; bits behind the stream's end
// read as zeros (lib/BitStream.js:84).  One lane per request, three launches, no host round trip in between:
//
//   k7_blocks_probe    the 48 bits at bitpos[k] from three aligned dwords of the staged, zero padded stream and a funnel shift;
//                      the request's class; the number of block requests of every workgroup.  A position at or behind 8 * len is
//                      'neither' without a load (and without forming pos + 48).
//   k7_blocks_scan     one workgroup: exclusive scan of the workgroup totals, the block count and the stream's 4-byte header word
//                      (the host reads the two in one copy).
//   k7_blocks_compact  the block requests, stably and in request order, into the candidate list k7_decode reads (pos << 1) and the
//                      request of every candidate: wave ballot + lane prefix, wave totals through LDS, the workgroup's base.
#include "decode.h"

#define WHOLEPI 0x314159265359ull
#define SQRTPI 0x177245385090ull

// the 48 bits at bit position pos (< 8 * len) of the big-endian bit stream in32: bytes [pos / 8, pos / 8 + 7) lie in the dwords
// w, w + 1, w + 2 with w = pos / 32 - inside the buffer, whose zero padding is longer than 12 bytes
__device__ __forceinline__ u64 bits48_at(const u32* in32, u64 pos) {
    const u64 w = pos >> 5;
    const u32 sh = (u32)pos & 31u;
    const u32 d0 = __builtin_bswap32(in32[w]), d1 = __builtin_bswap32(in32[w + 1u]), d2 = __builtin_bswap32(in32[w + 2u]);
    const u32 hi = __funnelshift_l(d1, d0, sh), lo = __funnelshift_l(d2, d1, sh);      // bits [pos, pos + 32) and [pos + 32, pos + 64)
    return ((u64)hi << 16) | (lo >> 16);
}

__device__ __forceinline__ u32 block_class(const u32* in32, u64 len, const u64* bitpos, u32 count, u32 k) {
    if (k >= count) return DEC_REQ_NEITHER;
    const u64 pos = bitpos[k];
    if ((pos >> 3) >= len) return DEC_REQ_NEITHER;            // only zeros from there on
    const u64 v = bits48_at(in32, pos);
    return v == WHOLEPI ? DEC_REQ_BLOCK : v == SQRTPI ? DEC_REQ_END : DEC_REQ_NEITHER;
}

__global__ __launch_bounds__(256) void k7_blocks_probe(const u32* in32, u64 len, const u64* bitpos, u32 count, u8* cls, u32* wgTot) {
    __shared__ u32 s_w[4];
    const u32 k = blockIdx.x * 256u + threadIdx.x;
    const u32 c = block_class(in32, len, bitpos, count, k);
    if (k < count) cls[k] = (u8)c;
    const u64 bal = __ballot(c == DEC_REQ_BLOCK);
    if ((threadIdx.x & 63u) == 0) s_w[threadIdx.x >> 6] = (u32)__popcll(bal);
    __syncthreads();
    if (threadIdx.x == 0) wgTot[blockIdx.x] = s_w[0] + s_w[1] + s_w[2] + s_w[3];
}

// wgTot[g] -> the number of block requests in front of workgroup g; head[0] = their total, head[1] = the stream's first 4 bytes
__global__ __launch_bounds__(1024) void k7_blocks_scan(const u32* in32, u32* wgTot, u32 nwg, u32* head) {
    __shared__ u32 sh[20];
    u32 run = 0;
    for (u32 g0 = 0; g0 < nwg; g0 += 1024u) {
        const u32 g = g0 + threadIdx.x;
        const u32 v = g < nwg ? wgTot[g] : 0u;
        u32 tot = 0;
        const u32 ex = block_excl_scan_1024(v, sh, &tot);
        if (g < nwg) wgTot[g] = run + ex;
        run += tot;
    }
    if (threadIdx.x == 0) { head[0] = run; head[1] = __builtin_bswap32(in32[0]); }
}

__global__ __launch_bounds__(256) void k7_blocks_compact(const u64* bitpos, u32 count, const u8* cls, const u32* wgBase, u64* cand,
                                                         u32* reqOf) {
    __shared__ u32 s_w[4];
    const u32 k = blockIdx.x * 256u + threadIdx.x, wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    const bool blk = k < count && cls[k] == DEC_REQ_BLOCK;
    const u64 bal = __ballot(blk);
    if (lane == 0) s_w[wave] = (u32)__popcll(bal);
    __syncthreads();
    if (!blk) return;
    u32 at = wgBase[blockIdx.x] + (u32)__popcll(bal & ((1ull << lane) - 1ull));
    for (u32 w = 0; w < wave; w++) at += s_w[w];
    cand[at] = bitpos[k] << 1;                 // (a block magic starts inside the stream: pos < 2^63)
    reqOf[at] = k;
}

int k7_blocks(const u32* d_in32, u64 len, const u64* d_bitpos, u32 count, u8* d_cls, u32* d_wgTot, u64* d_cand, u32* d_reqOf,
              u32* d_head, hipStream_t stream) {
    const u32 nwg = (count + 255u) / 256u;
    hipLaunchKernelGGL(k7_blocks_probe, dim3(nwg), dim3(256), 0, stream, d_in32, len, d_bitpos, count, d_cls, d_wgTot);
    HIP_CHECK_RET(hipGetLastError());
    hipLaunchKernelGGL(k7_blocks_scan, dim3(1), dim3(1024), 0, stream, d_in32, d_wgTot, nwg, d_head);
    HIP_CHECK_RET(hipGetLastError());
    hipLaunchKernelGGL(k7_blocks_compact, dim3(nwg), dim3(256), 0, stream, d_bitpos, count, (const u8*)d_cls, (const u32*)d_wgTot, d_cand, d_reqOf);
    HIP_CHECK_RET(hipGetLastError());
    return CJS_OK;
}
