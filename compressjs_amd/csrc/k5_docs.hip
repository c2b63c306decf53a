// K5 stream cursor for a batch of documents: k5_blockscan's sibling.  Every document becomes a .bz2 stream of its own,
// byte-aligned and back to back in the output (the reference has no batched entry; each stream is what Bzip2.compressFile
// writes for that document alone):
//   stream header 'B','Z','h','0'+level     lib/Bzip2.js:903-906   at a document's first block
//   combined CRC                            lib/Bzip2.js:917       reset per document
//   end-of-stream magic + combined CRC      lib/Bzip2.js:925-927   behind a document's last block, then zero bits up to a byte
// An empty document has no block: its 14-byte stream is written behind the document in front of it (k5_docs_first writes
// those in front of the first block).  A document may span sub-batches: the cursor and its running CRC wait in StreamState.
// Header and trailer words share 32-bit words with the neighbouring streams and with block bits that k5_pack ORs in later,
// so they are OR-ed into the zeroed output too.
#include "pipeline.h"

__device__ __forceinline__ u32 kd_bswap32(u32 v) {
    return (v >> 24) | ((v >> 8) & 0xFF00u) | ((v << 8) & 0xFF0000u) | (v << 24);
}
// OR `nbits` (24 or 32) of `value` into the stream at bit position pos (MSB first)
__device__ __forceinline__ void kd_put(u32* out, u64 pos, u32 nbits, u32 value) {
    const u32 sh = (u32)(pos & 31u);
    const u64 v = ((u64)value << (64u - nbits)) >> sh;
    const u32 hi = (u32)(v >> 32), lo = (u32)v;
    if (hi) atomicOr(&out[pos >> 5], kd_bswap32(hi));
    if (lo) atomicOr(&out[(pos >> 5) + 1], kd_bswap32(lo));
}

struct DocCursor { u64 bits; u32 crc; u32 ovf; };

// the next piece ends at bit `end`: does it fit?  (k5_blockscan's margin: a piece's last word may lie 8 bytes behind its last bit)
__device__ __forceinline__ bool kd_fits(const Pipe& P, DocCursor& c, u64 end) {
    if (c.ovf || ((end + 7u) >> 3) + 8u > P.outCapBytes) { c.ovf = 1; return false; }
    return true;
}
__device__ __forceinline__ void kd_open(const Pipe& P, const K5Docs& D, DocCursor& c) {
    c.bits = (c.bits + 7u) & ~(u64)7;
    if (kd_fits(P, c, c.bits + 32u)) kd_put(P.out, c.bits, 32, 0x425A6800u | (u32)('0' + D.level));
    c.bits += 32u;
    c.crc = 0;
}
__device__ __forceinline__ void kd_close(const Pipe& P, const K5Docs& D, DocCursor& c, u32 d) {
    if (kd_fits(P, c, c.bits + 80u)) {
        kd_put(P.out, c.bits, 24, 0x177245u);
        kd_put(P.out, c.bits + 24u, 24, 0x385090u);
        kd_put(P.out, c.bits + 48u, 32, c.crc);
    }
    c.bits = (c.bits + 80u + 7u) & ~(u64)7;
    D.outOff[d + 1] = c.bits >> 3;
}
// the streams of the empty documents d, d + 1, ... up to the next document that has a block
__device__ __forceinline__ void kd_empties(const Pipe& P, const K5Docs& D, DocCursor& c, u32 d) {
    for (; d < D.count && D.docFirst[d + 1] == D.docFirst[d]; d++) {
        kd_open(P, D, c);
        kd_close(P, D, c, d);
    }
}

__global__ __launch_bounds__(64) void k5_docs_first(Pipe P, K5Docs D) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    DocCursor c = {0, 0, 0};
    D.outOff[0] = 0;
    kd_empties(P, D, c, 0);
    P.ss->bits = c.bits;
    P.ss->crc = c.crc;
    P.ss->overflow = c.ovf;
}

__global__ __launch_bounds__(64) void k5_docscan(Pipe P, K5Docs D, u32 first_block) {
    if (threadIdx.x != 0) return;
    DocCursor c = {P.ss->bits, P.ss->crc, P.ss->overflow};
    for (u32 b = 0; b < P.g.nb; b++) {
        P.bitoff[b] = c.bits;
        if (!P.nlen[b]) continue;
        const u32 kb = first_block + b, d = D.blkDoc[kb];
        if (kb == D.docFirst[d]) kd_open(P, D, c);
        P.bitoff[b] = c.bits;
        (void)kd_fits(P, c, c.bits + P.bitlen[b]);
        c.bits += P.bitlen[b];
        c.crc = ((c.crc << 1) | (c.crc >> 31)) ^ P.crc[b];
        if (kb + 1u == D.docFirst[d + 1]) {
            kd_close(P, D, c, d);
            kd_empties(P, D, c, d + 1u);
        }
    }
    P.ss->bits = c.bits;
    P.ss->crc = c.crc;
    P.ss->overflow = c.ovf;
    if (P.snap) *P.snap = c.bits;
}

int k5_docs_begin(Pipe P, K5Docs D, hipStream_t stream) {
    hipLaunchKernelGGL(k5_docs_first, dim3(1), dim3(64), 0, stream, P, D);
    HIP_CHECK_RET(hipGetLastError());
    return CJS_OK;
}

int k5_docscan_run(Pipe P, K5Docs D, u32 first_block, hipStream_t stream) {
    hipLaunchKernelGGL(k5_docscan, dim3(1), dim3(64), 0, stream, P, D, first_block);
    HIP_CHECK_RET(hipGetLastError());
    return CJS_OK;
}
