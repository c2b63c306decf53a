// cjs_bwtc_compress_batch*: many independent documents in, one BWTC stream each out, in one call (declared in
// include/compressjs_amd.h).  The reference has no batched entry: stream d is what BWTC.compressFile(Buffer, null, level)
// (lib/BWTC.js:12-139, lib/Util.js:105-142) gives for document d alone, i.e. cjs_bwtc_compress with the size declared.
//
// Every level runs on the device: the plan, the block stages (K1 linear, K2 as cjs_bwtc_compress issues them, the rows gathered
// from many documents by k11_gather), the model of every block - K10 (FenwickModel) for levels 6-9, K13 (DefSumModel,
// lib/BWTC.js:107) for levels 1-5, both leaving (sy_f, lt_f, tot_f) triples in the same rows - the range coder of every document
// (k11_code) and the move of the streams to their places; the host issues launches and waits three times, whatever the level and
// the number of documents (cjs_dbg_bwtc_batch_syncs; K1's own small read-backs per sub-batch are the single call's and are not
// counted).  No host code runs between the upload and the download.
//   forward:  all k11_code launches go on the context's main stream in sub-batch order, each behind its sub-batch's K10 (evB10);
//   backward: the next sub-batch on a workspace waits for the k11_code that read its rows (evB11) - the triples live in K1's
//             round lists and would be overwritten otherwise.
// (The single call cjs_bwtc_compress keeps its host DefSumModel for levels 1-5.)
#include "cjs_ctx.h"

using namespace cjs;

extern "C" int64_t cjs_bwtc_compress_batch_bound(uint64_t total_len, uint32_t count) {
    return (int64_t)(total_len + total_len / 4 + (uint64_t)4096 * count);      // the sum of bwtc_bound over the documents
}

extern "C" int cjs_dbg_bwtc_batch_syncs(cjs_ctx* c) { return c ? c->bwtc_batch_syncs : 0; }

namespace {

hipError_t bsync(cjs_ctx* c, hipStream_t st) { c->bwtc_batch_syncs++; return hipStreamSynchronize(st); }

void drain(cjs_ctx* c) {                                          // (error paths: nothing of this call is left running)
    for (u32 i = 0; i < c->nstreams; i++) (void)hipStreamSynchronize(c->sub[i]);
    (void)hipStreamSynchronize(c->stream);
}

// the offsets checked and the plan made, both on the device: *in_len = off[count], *nblocks, *max_n = the longest block
int64_t plan_batch(cjs_ctx* c, const void* d_in, const u64* d_off, u32 count, int level, K11Plan& Q, u64* in_len, u32* nblocks, u32* max_n) {
    hipStream_t st = c->stream;
    u64* d_res = (u64*)((char*)c->d_ss + 64);
    int rc = k0_docs_check(d_off, count, d_res, st);
    if (rc) return rc;
    HIP_CHECK_RET(hipMemcpyAsync(c->pin[0], d_res, 16, hipMemcpyDeviceToHost, st));
    HIP_CHECK_RET(bsync(c, st));
    u64 res[2];
    memcpy(res, c->pin[0], 16);
    *in_len = res[0];
    if (res[1] || (!d_in && res[0])) return CJS_E_ARG;
    const u32 bs = (u32)level * 100000u;
    if (res[0] / bs + (u64)count + 2 > 0xFFFFFFF0ull) return CJS_E_ARG;         // block numbers are 32 bits wide
    rc = grow(&c->k0ws, &c->k0ws_bytes, k11_plan_bytes(res[0], count, bs));
    if (rc) return rc;
    k11_plan_carve(Q, (const u8*)d_in, d_off, res[0], count, level, c->k0ws);
    rc = k11_plan_run(Q, st);
    if (rc) return rc;
    HIP_CHECK_RET(hipMemcpyAsync(c->pin[0], Q.flags, K11_F_WORDS * 4, hipMemcpyDeviceToHost, st));
    HIP_CHECK_RET(bsync(c, st));
    if (c->pin[0][K11_F_BAD]) return CJS_E_ARG;                   // (cannot happen for valid offsets)
    *nblocks = c->pin[0][K11_F_NBLOCKS];
    *max_n = c->pin[0][K11_F_MAXLEN];
    return CJS_OK;
}

// one sub-batch through the rows, K1 (linear) and K2, as cjs_bwtc_compress issues them
int block_stages(cjs_ctx* c, const K11Plan& Q, const BatchGeom& g, u32 f, u32 nb, u32 si, u32 max_n, Pipe& P) {
    hipStream_t ss = c->sub[si];
    pipe_carve(P, g, c->ws[si]);
    P.g.nb = nb;
    P.k1.linear = 1;
    P.k1.hpin = c->pin[si]; P.k1.hpinWords = CJS_PIN_WORDS;
    int rc = k11_gather_run(Q, P, f, ss);
    if (!rc) rc = k1_run(P.k1, P.g, max_n, ss);
    if (!rc) rc = k2_run(P, max_n, ss);
    return rc;
}

// every level: K10 models the blocks of levels 6-9, K13 those of levels 1-5
int64_t batch_device_fast(cjs_ctx* c, const void* d_in, const u64* d_off, u32 count, int level, void* d_out, u64 out_cap, u64* d_out_off) {
    hipStream_t st = c->stream;
    HIP_CHECK_RET(hipEventRecord(c->ev0, st));
    K11Plan Q;
    u64 in_len = 0;
    u32 nblocks = 0, max_n = 0;
    const int64_t prc = plan_batch(c, d_in, d_off, count, level, Q, &in_len, &nblocks, &max_n);
    if (prc) return prc;
    const u32 ns = c->nstreams;
    for (u32 i = 0; i < ns; i++) {
        if (!c->evB10[i]) HIP_CHECK_RET(hipEventCreateWithFlags(&c->evB10[i], hipEventDisableTiming));
        if (!c->evB11[i]) HIP_CHECK_RET(hipEventCreateWithFlags(&c->evB11[i], hipEventDisableTiming));
    }
    HIP_CHECK_RET(hipEventRecord(c->evReady, st));                // the plan (and whatever put the input there on this stream)
    const BatchGeom g = make_geom(c->sub_blocks, Q.bs);
    const u32 ostride = 2u * g.stride;                            // K10's rows: the round lists of K1, free in linear mode - all of them
    u32 j = 0;
    for (u32 f = 0; f < nblocks; f += c->sub_blocks, j++) {
        const u32 si = j % ns;
        const u32 nb = nblocks - f < c->sub_blocks ? nblocks - f : c->sub_blocks;
        hipStream_t ss = c->sub[si];
        hipError_t e = hipStreamWaitEvent(ss, j < ns ? c->evReady : c->evB11[si], 0);
        if (e != hipSuccess) { drain(c); return CJS_E_HIP - (int)e; }
        Pipe P;
        int rc = block_stages(c, Q, g, f, nb, si, max_n, P);
        if (!rc) rc = (level <= 5 ? k13_defsum_run : k10_model_run)(P, (u32*)P.k1.rlist[0], (u32*)P.k1.rlist[1], P.ngroups, ostride, ostride, ss);
        if (!rc && (e = hipEventRecord(c->evB10[si], ss)) != hipSuccess) rc = CJS_E_HIP - (int)e;
        if (!rc && (e = hipStreamWaitEvent(st, c->evB10[si], 0)) != hipSuccess) rc = CJS_E_HIP - (int)e;
        const K11Sub S = {f, nb, P.nlen, P.pidx, P.used, P.ngroups, (const u32*)P.k1.rlist[0], (const u32*)P.k1.rlist[1], ostride};
        if (!rc) rc = k11_code_run(Q, S, st);
        if (!rc && (e = hipEventRecord(c->evB11[si], st)) != hipSuccess) rc = CJS_E_HIP - (int)e;
        if (rc) { drain(c); return rc; }
    }
    // long streams are moved by several workgroups each
    const u64 avg = in_len / count;
    const u32 split = avg < 65536u ? 1u : (avg / 65536u < 64u ? (u32)(avg / 65536u) : 64u);
    int rc = k11_finish_run(Q, (u8*)d_out, out_cap, d_out_off, split, st);
    if (rc) { drain(c); return rc; }
    HIP_CHECK_RET(hipMemcpyAsync(c->pin[0], Q.flags, K11_F_WORDS * 4, hipMemcpyDeviceToHost, st));
    HIP_CHECK_RET(hipMemcpyAsync(c->pin[0] + K11_F_WORDS, d_out_off + count, 8, hipMemcpyDeviceToHost, st));
    HIP_CHECK_RET(hipEventRecord(c->ev1, st));
    HIP_CHECK_RET(bsync(c, st));
    HIP_CHECK_RET(hipEventElapsedTime(&c->last_ms, c->ev0, c->ev1));
    c->last_blocks = nblocks;
    u64 total;
    memcpy(&total, c->pin[0] + K11_F_WORDS, 8);
    if (c->pin[0][K11_F_K10]) return CJS_E_UNSUPPORTED;           // a block's triples did not fit K10's rows: no bytes rather than wrong ones
    if (c->pin[0][K11_F_SCRATCH] || c->pin[0][K11_F_NOSPACE] || total > out_cap) return CJS_E_NOSPACE;
    return (int64_t)total;
}

}  // namespace

extern "C" int64_t cjs_bwtc_compress_batch_device(cjs_ctx* c, const void* d_in, const uint64_t* d_off, uint32_t count, int level,
                                                  void* d_out, uint64_t out_cap, uint64_t* d_out_off) {
    if (!c) return CJS_E_ARG;
    if (level < 1 || level > 9) level = 9;                        // lib/BWTC.js:16-19: bad props -> 9
    if (count == 0) return 0;
    if (!d_off || !d_out || !d_out_off) return CJS_E_ARG;
    if (hipSetDevice(c->device) != hipSuccess) return CJS_E_NOGPU;
    c->bwtc_batch_syncs = 0;
    return batch_device_fast(c, d_in, (const u64*)d_off, count, level, d_out, out_cap, (u64*)d_out_off);
}

extern "C" int64_t cjs_bwtc_compress_batch(cjs_ctx* c, const uint8_t* in, const uint64_t* off, uint32_t count, int level,
                                           uint8_t* out, uint64_t out_cap, uint64_t* out_off) {
    if (!c) return CJS_E_ARG;
    if (level < 1 || level > 9) level = 9;
    if (count == 0) return 0;
    if (!off || !out || !out_off) return CJS_E_ARG;
    for (u32 d = 0; d < count; d++) if (off[d + 1] < off[d]) return CJS_E_ARG;
    const uint64_t total = off[count];
    if (!in && total) return CJS_E_ARG;
    if (hipSetDevice(c->device) != hipSuccess) return CJS_E_NOGPU;
    c->bwtc_batch_syncs = 0;
    // one upload (the documents, then their offsets behind them), one trip, one download
    const uint64_t need = (uint64_t)cjs_bwtc_compress_batch_bound(total, count);
    const size_t off_at = (size_t)((total + 64 + 7) & ~(uint64_t)7), off_bytes = ((size_t)count + 1) * 8;
    int rc = grow(&c->din, &c->din_bytes, off_at + 2 * off_bytes);
    if (rc) return rc;
    uint64_t* d_off = (uint64_t*)((char*)c->din + off_at);
    uint64_t* d_out_off = d_off + count + 1;
    if (total) HIP_CHECK_RET(hipMemcpyAsync(c->din, in, total, hipMemcpyHostToDevice, c->stream));
    HIP_CHECK_RET(hipMemcpyAsync(d_off, off, off_bytes, hipMemcpyHostToDevice, c->stream));
    rc = grow(&c->dout, &c->dout_bytes, need + 64);
    if (rc) return rc;
    const int64_t n = batch_device_fast(c, c->din, (const u64*)d_off, count, level, c->dout, need, (u64*)d_out_off);
    if (n < 0 && n != CJS_E_NOSPACE) return n;
    HIP_CHECK_RET(hipMemcpyAsync(out_off, d_out_off, off_bytes, hipMemcpyDeviceToHost, c->stream));
    const bool fits = n >= 0 && (uint64_t)n <= out_cap;
    if (fits && n) HIP_CHECK_RET(hipMemcpyAsync(out, c->dout, (size_t)n, hipMemcpyDeviceToHost, c->stream));
    HIP_CHECK_RET(bsync(c, c->stream));
    return fits ? n : CJS_E_NOSPACE;
}
