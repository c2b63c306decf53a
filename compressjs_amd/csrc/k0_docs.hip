// K0 for a batch of documents: the blocks readBlock (lib/Bzip2.js:636-667) cuts from every document on its own, numbered in
// document order.  The reference has no batched entry; the contract is "what N single calls would cut".
//
// The tile scans of k0_rle1.hip run over the packed input as they are: C(i) is the RLE1 cost prefix with runs left UNCUT, also
// across document boundaries.  A document start is then what a block start already is to k0_chain - a position that starts a
// fresh run whatever stands in front of it - and gets the same cut-run correction (blkRe / blkAdj); a document end is what the
// end of the input is to it: the last block may be short.  So nothing of the tile passes changes, and k0_materialize / k0_pad /
// k0_crc, whose output no byte outside [blkStart, blkEnd) influences, run unchanged on the plan made here.
//
//   k0_docs_offsets         the offsets must not decrease; off[count] = the bytes of the batch
//   k0_doc_chain<false>     one workgroup per document walks its boundary chain and counts its blocks
//   k0_docs_scan            exclusive scan of the counts: docFirst[d], *nBlocks
//   k0_doc_chain<true>      the same walk, filling blkStart / blkEnd / blkAdj / blkRe / blkN / blkDoc from docFirst[d]
#include "k0_plan.h"
#include <string.h>

__global__ __launch_bounds__(256) void k0_docs_offsets(const u64* off, u32 count, u64* res) {
    const u64 i = (u64)blockIdx.x * 256u + threadIdx.x;
    if (i < count && off[i + 1] < off[i]) res[1] = 1;
    if (i == 0) res[0] = off[count];
}

// The chain of k0_chain for input bytes [d0, dend): the same steps, with the document's end in the place of the input's.
template <bool STORE>
__global__ __launch_bounds__(256) void k0_doc_chain(K0Buf K, K0Docs D, u32 cap) {
    __shared__ u64 sh[256];
    __shared__ u32 sh32[4];
    for (u32 d = blockIdx.x; d < D.count; d += gridDim.x) {   // (the grid is capped: K0_DOC_GRID)
    const u64 d0 = D.off[d], dend = D.off[d + 1];
    K0Buf Kd = K;                                               // the input cut off at the document's end: what the run walk sees
    Kd.in_len = dend;
    Kd.ntiles = (dend + K0_TILE - 1) / K0_TILE;
    const u32 base = STORE ? D.docFirst[d] : 0u;
    u64 s = d0, cnext = 0, cend = 0;
    bool have_cnext = false, have_cend = false;
    u32 kb = 0;
    while (s < dend) {
        const bool cut = s > 0 && K.in[s - 1] == K.in[s];     // (at s == d0: the neighbouring document ends in the same byte)
        u64 e = s, adj = 0, re = s, pre = 0;
        u32 n = 0;
        bool done = false;
        if (cut) {
            re = k0_run_end(Kd, s, sh);                         // (<= dend: a run never continues into the next document)
            const u64 gL = k0_g(re - s);
            if (gL >= cap) {
                // the block ends inside the cut run: smallest k with g(k) >= cap
                const u32 q = cap / 5u, rem = cap % 5u;
                const u64 k = (u64)q * 255u + (rem == 0 ? 0u : (rem <= 3u ? rem : 4u));
                e = s + k;
                const u32 gk = k0_g(k);
                n = gk < cap ? gk : cap;
                re = e;
                done = true;
            } else if (re >= dend) {                            // the cut run reaches the document's end without filling the block
                e = dend;
                n = (u32)gL;
                re = e;
                done = true;
            } else {
                pre = gL;
            }
        }
        if (!done) {
            const u64 cbase = (!cut && have_cnext) ? cnext : k0_evalC(K, re, sh, sh32);
            adj = cbase - pre;                                  // OB_s(i) = C(i) - adj for i >= re
            if (!have_cend) { cend = k0_evalC(K, dend, sh, sh32); have_cend = true; }
            if (cend - adj < cap) {                             // the document ends before the block fills
                e = dend;
                n = (u32)(cend - adj);
                have_cnext = false;
            } else {
                u64 ce = 0;
                e = k0_searchC(K, adj + cap, re, sh, sh32, &ce);   // (<= dend: C(dend) reaches the target)
                const u64 ob = ce - adj;
                n = ob < cap ? (u32)ob : cap;
                cnext = ce;
                have_cnext = true;
            }
        } else {
            have_cnext = false;
        }
        if (STORE && threadIdx.x == 0 && base + kb < K.maxBlocks) {
            const u32 k = base + kb;
            K.blkStart[k] = s;
            K.blkEnd[k] = e;
            K.blkN[k] = n;
            K.blkAdj[k] = adj;
            K.blkRe[k] = re;
            D.blkDoc[k] = d;
        }
        kb++;
        s = e;
        if (n < cap) break;                                     // lib/Bzip2.js:922
    }
    if (!STORE && threadIdx.x == 0) D.docFirst[d] = kb;
    __syncthreads();
    }
}

// docFirst: per-document block counts in, their exclusive scan out; docFirst[count] = *nBlocks = the total
__global__ __launch_bounds__(1024) void k0_docs_scan(K0Buf K, K0Docs D) {
    __shared__ u32 sh[20];
    __shared__ u64 carry;
    const u32 tid = threadIdx.x;
    if (tid == 0) carry = 0;
    __syncthreads();
    for (u64 c0 = 0; c0 < D.count; c0 += 1024u) {
        const u64 i = c0 + tid;
        const u32 v = i < D.count ? D.docFirst[i] : 0u;
        u32 tot;
        const u32 ex = block_excl_scan_1024(v, sh, &tot);
        const u64 at = carry + ex;
        if (i < D.count) D.docFirst[i] = at < 0xFFFFFFFFull ? (u32)at : 0xFFFFFFFFu;
        __syncthreads();
        if (tid == 0) carry += tot;
        __syncthreads();
    }
    if (tid == 0) {
        const bool bad = carry > K.maxBlocks;
        D.docFirst[D.count] = bad ? 0u : (u32)carry;
        *K.nBlocks = bad ? 0u : (u32)carry;
        *D.bad = bad ? 1u : 0u;
    }
}

// ---- host side ---------------------------------------------------------------------------------------
#define K0_DOC_GRID (1u << 20)   // workgroups of k0_doc_chain at most: beyond that a workgroup walks several documents
static inline size_t kd_al(size_t x) { return (x + 255) & ~(size_t)255; }
static inline u64 kd_max_blocks(u64 in_len, u32 count, u32 cap) { return in_len / (cap / 2 + 1) + (u64)count + 2; }   // k0_carve's bound, per document

size_t k0_docs_bytes(u64 in_len, u32 count, u32 cap) {
    const u64 ntiles = (in_len + K0_TILE - 1) / K0_TILE;
    const u64 nchunks = (ntiles + 1 + 1023) / 1024;
    const u64 mb = kd_max_blocks(in_len, count, cap);
    return 3 * kd_al((ntiles + 2) * 8) + kd_al((nchunks + 1) * 8) + 4 * kd_al(mb * 8) + 2 * kd_al(mb * 4) + kd_al(((size_t)count + 1) * 4) + 512;
}

void k0_docs_carve(K0Buf& K, K0Docs& D, const u8* d_in, const u64* d_off, u64 in_len, u32 count, u32 cap, void* ws) {
    memset(&K, 0, sizeof K);
    K.in = d_in;
    K.in_len = in_len;
    K.ntiles = (in_len + K0_TILE - 1) / K0_TILE;
    K.nchunks = (K.ntiles + 1 + 1023) / 1024;
    K.maxBlocks = (u32)kd_max_blocks(in_len, count, cap);
    char* p = (char*)ws;
    const size_t ta = kd_al((K.ntiles + 2) * 8);
    K.tileA = (u64*)p; p += ta;
    K.tileB = (u64*)p; p += ta;
    K.tileC = (u64*)p; p += ta;
    K.chunk = (u64*)p; p += kd_al((K.nchunks + 1) * 8);
    const size_t bb = kd_al((size_t)K.maxBlocks * 8);
    K.blkStart = (u64*)p; p += bb;
    K.blkEnd = (u64*)p; p += bb;
    K.blkAdj = (u64*)p; p += bb;
    K.blkRe = (u64*)p; p += bb;
    K.blkN = (u32*)p; p += kd_al((size_t)K.maxBlocks * 4);
    D.blkDoc = (u32*)p; p += kd_al((size_t)K.maxBlocks * 4);
    D.docFirst = (u32*)p; p += kd_al(((size_t)count + 1) * 4);
    K.nBlocks = (u32*)p;
    D.bad = K.nBlocks + 1;
    p += 256;
    K.specBad = (u64*)p;                                        // (k0_scans resets it; the batch plan does not speculate)
    D.off = d_off;
    D.count = count;
}

int k0_docs_check(const u64* d_off, u32 count, u64* d_res, hipStream_t stream) {
    HIP_CHECK_RET(hipMemsetAsync(d_res, 0, 16, stream));
    hipLaunchKernelGGL(k0_docs_offsets, dim3(count / 256u + 1u), dim3(256), 0, stream, d_off, count, d_res);
    HIP_CHECK_RET(hipGetLastError());
    return CJS_OK;
}

int k0_docs_prepass(K0Buf K, K0Docs D, u32 cap, hipStream_t stream) {
    if (K.in_len == 0) {                                        // only empty documents: no block
        HIP_CHECK_RET(hipMemsetAsync(D.docFirst, 0, ((size_t)D.count + 1) * 4, stream));
        HIP_CHECK_RET(hipMemsetAsync(K.nBlocks, 0, 8, stream));
        return CJS_OK;
    }
    const int rc = k0_scans(K, stream);
    if (rc) return rc;
    hipLaunchKernelGGL(k0_doc_chain<false>, dim3(D.count < K0_DOC_GRID ? D.count : K0_DOC_GRID), dim3(256), 0, stream, K, D, cap);
    hipLaunchKernelGGL(k0_docs_scan, dim3(1), dim3(1024), 0, stream, K, D);
    hipLaunchKernelGGL(k0_doc_chain<true>, dim3(D.count < K0_DOC_GRID ? D.count : K0_DOC_GRID), dim3(256), 0, stream, K, D, cap);
    HIP_CHECK_RET(hipGetLastError());
    return CJS_OK;
}
