// K7 for a batch of documents (cjs_bz2_decompress_batch, decode.hip: dec_batch): the document level in front of and behind
// k7_decode / K8 / K9.  The reference decodes one stream per call (Bzip2.decompressFile, lib/Bzip2.js:454-481) and reads bits
// past the end of its input as zeros (lib/BitStream.js:84); a document of a batch must see exactly that - never its neighbour.
//
//   k7_stage_docs   copies document d (input bytes [off[d], off[d+1]), any alignment) to a 256-byte aligned base of the
//                   decoder's input buffer, base[d+1] = (base[d] + length + 8) rounded up to 256: zeros follow every document up
//                   to the next chunk boundary, at least 8 of them - more than the 48 bits of a magic, so no pattern runs from
//                   one document into the next.  Also: the document of every chunk, and every document's first 4 bytes (the
//                   stream header the host walk reads, :137-152).
//   k7_scan_docs    k7_scan_magic over the staged batch.  A candidate belongs to the document of its chunk and exists only when
//                   it starts inside that document, behind its 4-byte header; bytes behind the document's end read as zeros, as
//                   in the single call.  The record of a block candidate carries the first chunk behind its document (k7_decode's
//                   limit for that block), the record of an end-of-stream candidate what the walk reads behind it (:465-477): the
//                   32-bit stream CRC and the 4 bytes at the next byte boundary (the header of a follow-on stream) - so the host
//                   never goes back to HBM for 16 bytes per document.
//   k9_docs_meta    out_off / status / detail of every document into the caller's device arrays.
//   k9_docs_gather  closes the gaps that failed documents left in the decoded bytes (a block CRC is known only after K9 has
//                   written the block): the error path only.
#include "decode.h"

#define WHOLEPI 0x314159265359ull
#define SQRTPI 0x177245385090ull

// the document that owns staged byte `at`: the last d < count with base[d] <= at
__device__ __forceinline__ u32 doc_of(const u64* base, u32 count, u64 at) {
    u32 lo = 0, hi = count;                   // base[lo] <= at < base[hi]
    while (hi - lo > 1u) {
        const u32 mid = lo + (hi - lo) / 2u;
        if (base[mid] <= at) lo = mid; else hi = mid;
    }
    return lo;
}

__global__ __launch_bounds__(256) void k7_stage_docs(const u8* in, const u64* off, const u64* base, u32 count, u8* st,
                                                     u32* chunkDoc, u32* head) {
    __shared__ u32 s_d;
    const u64 b0 = (u64)blockIdx.x * 256u;
    if (threadIdx.x == 0) { s_d = doc_of(base, count, b0); chunkDoc[blockIdx.x] = s_d; }
    __syncthreads();
    const u32 d = s_d;
    const u64 src = off[d], len = off[d + 1] - src, rel = b0 + threadIdx.x - base[d];
    st[b0 + threadIdx.x] = rel < len ? in[src + rel] : (u8)0;
    if (rel == 0) {                            // (bases are multiples of 256: thread 0 of the document's first chunk)
        u32 h = 0;
        for (u32 k = 0; k < 4u; k++) h = (h << 8) | (k < len ? in[src + k] : 0u);
        head[d] = h;
    }
}

__device__ __forceinline__ u32 doc_byte(const u8* st, u64 at, u64 end) { return at < end ? st[at] : 0u; }

__global__ __launch_bounds__(256) void k7_scan_docs(const u8* st, const u64* off, const u64* base, const u32* chunkDoc,
                                                    DecCand* cand, u32* ncand, u32 cap) {
    __shared__ u8 s[256 + 8];
    const u64 b0 = (u64)blockIdx.x * 256u;
    const u32 tid = threadIdx.x;
    const u32 d = chunkDoc[blockIdx.x];
    const u64 dbase = base[d], end = dbase + (off[d + 1] - off[d]);
    s[tid] = (u8)doc_byte(st, b0 + tid, end);
    if (tid < 8) s[256 + tid] = (u8)doc_byte(st, b0 + 256 + tid, end);
    __syncthreads();
    if (b0 + tid >= end) return;
    u64 w = 0;
    for (int k = 0; k < 8; k++) w = (w << 8) | s[tid + k];
    for (int sft = 0; sft < 8; sft++) {
        const u64 v = (w >> (16 - sft)) & 0xFFFFFFFFFFFFull;
        const u64 bit = (b0 + tid) * 8u + sft;
        if ((v == WHOLEPI || v == SQRTPI) && bit >= dbase * 8u + 32u) {
            DecCand c;
            c.key = (bit << 1) | (v == SQRTPI ? 1u : 0u);
            if (v == WHOLEPI) { c.a = (u32)((end + 255u) >> 8); c.b = 0; }
            else {
                const u64 q = bit + 48u, qb = q >> 3;                  // the stream CRC: 32 bits at q
                u64 five = 0;
                for (u32 k = 0; k < 5u; k++) five = (five << 8) | doc_byte(st, qb + k, end);
                c.a = (u32)(five >> (8u - (u32)(q & 7u)));
                const u64 nb = (bit + 80u + 7u) >> 3;                  // a follow-on stream starts at the next byte boundary
                u32 h = 0;
                for (u32 k = 0; k < 4u; k++) h = (h << 8) | doc_byte(st, nb + k, end);
                c.b = h;
            }
            const u32 k = atomicAdd(ncand, 1u);
            if (k < cap) cand[k] = c;
        }
    }
}

__global__ __launch_bounds__(256) void k9_docs_meta(const DecDocRec* rec, u32 count, u64* out_off, int* status, u32* detail) {
    const u32 d = blockIdx.x * 256u + threadIdx.x;
    if (d > count) return;
    const DecDocRec r = rec[d];                // (record `count`: dst = the total)
    out_off[d] = r.dst;
    if (d == count) return;
    status[d] = r.status;
    if (detail) { detail[3u * d] = r.detail; detail[3u * d + 1u] = r.got; detail[3u * d + 2u] = r.want; }
}

// dst[rec[d].dst .. +len) = src[rec[d].src .. +len) for every document that decoded; 4096 result bytes per workgroup
__global__ __launch_bounds__(256) void k9_docs_gather(const DecDocRec* rec, u32 count, const u8* src, u8* dst, u64 total) {
    for (u32 i = 0; i < 16u; i++) {
        const u64 at = ((u64)blockIdx.x * 16u + i) * 256u + threadIdx.x;
        if (at >= total) return;
        u32 lo = 0, hi = count;                // the last document with dst <= at (failed and empty ones have length 0: skipped by the search)
        while (hi - lo > 1u) {
            const u32 mid = lo + (hi - lo) / 2u;
            if (rec[mid].dst <= at) lo = mid; else hi = mid;
        }
        dst[at] = src[rec[lo].src + (at - rec[lo].dst)];
    }
}

int k7_stage(const u8* d_in, const u64* d_off, const u64* d_base, u32 count, u64 staged, u8* d_st, u32* d_chunkDoc, u32* d_head,
             hipStream_t stream) {
    if (staged) hipLaunchKernelGGL(k7_stage_docs, dim3((u32)(staged / 256u)), dim3(256), 0, stream, d_in, d_off, d_base, count, d_st, d_chunkDoc, d_head);
    HIP_CHECK_RET(hipGetLastError());
    return CJS_OK;
}
int k7_scan_batch(const u8* d_st, u64 staged, const u64* d_off, const u64* d_base, const u32* d_chunkDoc, DecCand* d_cand,
                  u32* d_ncand, u32 cap, hipStream_t stream) {
    HIP_CHECK_RET(hipMemsetAsync(d_ncand, 0, 4, stream));
    if (staged) hipLaunchKernelGGL(k7_scan_docs, dim3((u32)(staged / 256u)), dim3(256), 0, stream, d_st, d_off, d_base, d_chunkDoc, d_cand, d_ncand, cap);
    HIP_CHECK_RET(hipGetLastError());
    return CJS_OK;
}
int k9_docs_finish(const DecDocRec* d_rec, u32 count, u64* d_out_off, int* d_status, u32* d_detail, hipStream_t stream) {
    hipLaunchKernelGGL(k9_docs_meta, dim3(count / 256u + 1u), dim3(256), 0, stream, d_rec, count, d_out_off, d_status, d_detail);
    HIP_CHECK_RET(hipGetLastError());
    return CJS_OK;
}
int k9_docs_compact(const DecDocRec* d_rec, u32 count, const u8* d_src, u8* d_dst, u64 total, hipStream_t stream) {
    if (total) hipLaunchKernelGGL(k9_docs_gather, dim3((u32)((total + 4095u) / 4096u)), dim3(256), 0, stream, d_rec, count, d_src, d_dst, total);
    HIP_CHECK_RET(hipGetLastError());
    return CJS_OK;
}
