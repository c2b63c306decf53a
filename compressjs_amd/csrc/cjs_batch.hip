// cjs_bz2_compress_batch*: many independent documents in, one .bz2 stream each out, in one trip through the kernels
// (declared in include/compressjs_amd.h).  The reference has no batched entry: stream d is what Bzip2.compressFile
// (lib/Bzip2.js:879-929) gives for document d alone.  The plan comes from k0_docs.hip, the stream framing from k5_docs.hip;
// the blocks in between go through issue_blocks as those of a single stream do.
#include "cjs_ctx.h"

using namespace cjs;

// Per block at most 7.6 KB of header that does not depend on its length (six code-length tables of 258 symbols, 39 bits each at
// the worst) - fewer for a short document, whose alphabet has at most length + 2 symbols - plus 6 bits per selector (length / 32
// covers them); RLE1 and the codes as in cjs_bz2_compress_bound.  A document has one block more than its full ones.
extern "C" int64_t cjs_bz2_compress_batch_bound(uint64_t total_len, uint32_t count) {
    const uint64_t avg = count ? total_len / count + 1 : 0;
    const uint64_t per_doc = 256 + 30 * avg < 7700 ? 256 + 30 * avg : 7700;
    return (int64_t)(total_len + total_len / 2 + total_len / 32 + (total_len / 65536 + 2) * 24576 + 4096 + (uint64_t)count * per_doc);
}

extern "C" int64_t cjs_bz2_compress_batch_device(cjs_ctx* c, const void* d_in, const uint64_t* d_off, uint32_t count, int level,
                                                 void* d_out, uint64_t out_cap, uint64_t* d_out_off) {
    if (!c) return CJS_E_ARG;
    if (level < 1 || level > 9) return CJS_E_LEVEL;                  // lib/Bzip2.js:888-890
    if (count == 0) return 0;
    if (!d_off || !d_out || !d_out_off || out_cap < 64 || ((uintptr_t)d_out & 3)) return CJS_E_ARG;
    HIP_CHECK_RET(hipSetDevice(c->device));
    const u32 cap = block_cap(level);
    hipStream_t st = c->stream;
    // the offsets: nondecreasing, and off[count] says how many bytes the batch has (small scratch behind the stream cursor)
    u64* d_res = (u64*)((char*)c->d_ss + 64);
    HIP_CHECK_RET(hipEventRecord(c->ev0, st));                      // (the check is part of the call's device time)
    int rc = k0_docs_check((const u64*)d_off, count, d_res, st);
    if (rc) return rc;
    HIP_CHECK_RET(hipMemcpyAsync(c->pin[0], d_res, 16, hipMemcpyDeviceToHost, st));
    HIP_CHECK_RET(hipStreamSynchronize(st));
    u64 res[2];
    memcpy(res, c->pin[0], 16);
    const u64 in_len = res[0];
    if (res[1] || (!d_in && in_len)) return CJS_E_ARG;
    if (in_len / (cap / 2 + 1) + (u64)count + 2 > 0xFFFFFFF0ull) return CJS_E_ARG;     // block numbers are 32 bits wide
    rc = grow(&c->k0ws, &c->k0ws_bytes, k0_docs_bytes(in_len, count, cap));
    if (rc) return rc;
    K0Buf K;
    K0Docs D;
    k0_docs_carve(K, D, (const u8*)d_in, (const u64*)d_off, in_len, count, cap, c->k0ws);
    const K5Docs KD = {D.docFirst, D.blkDoc, (u64*)d_out_off, count, (u32)level};
    Pipe P0 = stream_pipe(c, d_out, out_cap);
    // as in cjs_bz2_compress_device: the output is zeroed on a sub-batch stream next to the pre-pass
    HIP_CHECK_RET(hipStreamWaitEvent(c->sub[0], c->ev0, 0));
    HIP_CHECK_RET(hipMemsetAsync(P0.out, 0, P0.outCapBytes, c->sub[0]));
    HIP_CHECK_RET(hipEventRecord(c->evDone[0], c->sub[0]));
    rc = k0_docs_prepass(K, D, cap, st);
    if (rc) { (void)hipStreamSynchronize(c->sub[0]); return rc; }
    HIP_CHECK_RET(hipStreamWaitEvent(st, c->evDone[0], 0));        // (k5_docs_begin writes the leading empty streams into the zeroed output)
    rc = k5_docs_begin(P0, KD, st);
    if (rc) { (void)hipStreamSynchronize(c->sub[0]); return rc; }
    HIP_CHECK_RET(hipEventRecord(c->evReady, st));
    HIP_CHECK_RET(hipMemcpyAsync(c->pin[0], K.nBlocks, 8, hipMemcpyDeviceToHost, st));
    HIP_CHECK_RET(hipStreamSynchronize(st));
    const u32 nblocks = c->pin[0][0];
    if (c->pin[0][1]) return CJS_E_ARG;                             // (more blocks than the plan has slots for: cannot happen for valid offsets)
    if (nblocks) {
        rc = issue_blocks(c, K, cap, 0, nblocks, d_out, out_cap, &KD);
        if (rc) return rc;
    }
    HIP_CHECK_RET(hipEventRecord(c->ev1, st));
    const int64_t bits = stream_bits(c, st, c->pin[0]);
    if (bits < 0 && bits != CJS_E_NOSPACE) return bits;
    HIP_CHECK_RET(hipEventElapsedTime(&c->last_ms, c->ev0, c->ev1));
    c->last_blocks = nblocks;
    return bits < 0 ? bits : bits >> 3;                             // (every stream ends on a byte)
}

extern "C" int64_t cjs_bz2_compress_batch(cjs_ctx* c, const uint8_t* in, const uint64_t* off, uint32_t count, int level,
                                          uint8_t* out, uint64_t out_cap, uint64_t* out_off) {
    if (!c) return CJS_E_ARG;
    if (level < 1 || level > 9) return CJS_E_LEVEL;
    if (count == 0) return 0;
    if (!off || !out || !out_off) return CJS_E_ARG;
    for (u32 d = 0; d < count; d++) if (off[d + 1] < off[d]) return CJS_E_ARG;
    const uint64_t total = off[count];
    if (!in && total) return CJS_E_ARG;
    HIP_CHECK_RET(hipSetDevice(c->device));
    // one upload (the documents, then their offsets behind them), one trip, one download
    const uint64_t need = (uint64_t)cjs_bz2_compress_batch_bound(total, count);
    const size_t off_at = (size_t)((total + 64 + 7) & ~(uint64_t)7), off_bytes = ((size_t)count + 1) * 8;
    int rc = grow(&c->din, &c->din_bytes, off_at + 2 * off_bytes);
    if (rc) return rc;
    rc = grow(&c->dout, &c->dout_bytes, need);
    if (rc) return rc;
    uint64_t* d_off = (uint64_t*)((char*)c->din + off_at);
    uint64_t* d_out_off = d_off + count + 1;
    if (total) HIP_CHECK_RET(hipMemcpyAsync(c->din, in, total, hipMemcpyHostToDevice, c->stream));
    HIP_CHECK_RET(hipMemcpyAsync(d_off, off, off_bytes, hipMemcpyHostToDevice, c->stream));
    const int64_t n = cjs_bz2_compress_batch_device(c, c->din, d_off, count, level, c->dout, c->dout_bytes, d_out_off);
    if (n < 0) return n;
    if ((uint64_t)n > out_cap) return CJS_E_NOSPACE;
    HIP_CHECK_RET(hipMemcpyAsync(out, c->dout, (size_t)n, hipMemcpyDeviceToHost, c->stream));
    HIP_CHECK_RET(hipMemcpyAsync(out_off, d_out_off, off_bytes, hipMemcpyDeviceToHost, c->stream));
    HIP_CHECK_RET(hipStreamSynchronize(c->stream));
    return n;
}
