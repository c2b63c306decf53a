// cjs_bwtc_compress_batch*: many independent documents in, one BWTC stream each out, in one call (declared in
// include/compressjs_amd.h).  The reference has no batched entry: stream d is what BWTC.compressFile(Buffer, null, level)
// (lib/BWTC.js:12-139, lib/Util.js:105-142) gives for document d alone, i.e. cjs_bwtc_compress with the size declared.
//
// Levels 6-9 - the fast path: the plan, the block stages (K1 linear, K2, K10 as cjs_bwtc_compress issues them, the rows
// gathered from many documents by k11_gather), the range coder of every document (k11_code) and the move of the streams to their
// places all run on the device; the host issues launches and waits three times, whatever the number of documents
// (cjs_dbg_bwtc_batch_syncs; K1's own small read-backs per sub-batch are the single call's and are not counted).
//   forward:  all k11_code launches go on the context's main stream in sub-batch order, each behind its sub-batch's K10 (evB10);
//   backward: the next sub-batch on a workspace waits for the k11_code that read its rows (evB11) - the triples live in K1's
//             round lists and would be overwritten otherwise.
//
// Levels 1-5 - NOT the fast path: the reference uses DefSumModel there (lib/BWTC.js:107), which this project runs on the host.
// The block stages still run batched on the GPU, sub-batch after sub-batch on one stream; the symbols go to the host and
// bwtc_block codes document after document.  The device form stages through the host for these levels.
#include "cjs_ctx.h"
#include "bwtc_host.h"

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

// levels 6-9
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
        if (!rc) rc = k10_model_run(P, (u32*)P.k1.rlist[0], (u32*)P.k1.rlist[1], P.ngroups, ostride, ostride, ss);
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

// levels 1-5: block stages on the GPU, DefSumModel and the range coder on the host.  d_in / d_off on the device, h_off their copy
// on the host; the streams go back to back into h_out, their offsets into h_out_off (complete also when they do not fit).
int64_t batch_host_tail(cjs_ctx* c, const void* d_in, const u64* d_off, const u64* h_off, u32 count, int level, u8* h_out, u64 out_cap,
                        u64* h_out_off) {
    hipStream_t st = c->stream;
    HIP_CHECK_RET(hipEventRecord(c->ev0, st));
    K11Plan Q;
    u64 in_len = 0;
    u32 nblocks = 0, max_n = 0;
    const int64_t prc = plan_batch(c, d_in, d_off, count, level, Q, &in_len, &nblocks, &max_n);
    if (prc) return prc;
    HIP_CHECK_RET(hipEventRecord(c->evReady, st));
    HIP_CHECK_RET(hipStreamWaitEvent(c->sub[0], c->evReady, 0));
    const u32 bs = Q.bs;
    const BatchGeom g = make_geom(c->sub_blocks, bs);
    std::vector<u32> hlen(c->sub_blocks), hpos(c->sub_blocks), hpidx(c->sub_blocks), hused((size_t)c->sub_blocks * 8);
    std::vector<u16> sym;
    std::vector<size_t> soff(c->sub_blocks);
    u32 d = 0;                                                    // the document the next block belongs to (or an empty one in front of it)
    u64 cursor = 0, left = 0;                                     // bytes laid down; blocks the open document still gets
    bool overflow = false;
    bwtc_coder* coder = nullptr;
    auto open_doc = [&]() {
        const u64 len = h_off[d + 1] - h_off[d];
        const u64 at = cursor < out_cap ? cursor : out_cap;
        h_out_off[d] = cursor;
        coder = bwtc_begin(h_out + at, out_cap - at, (int64_t)len, level);
        left = (len + bs - 1) / bs;
    };
    auto close_doc = [&]() {
        bool ov = false;
        cursor += bwtc_end_n(coder, &ov);
        overflow = overflow || ov;
        coder = nullptr;
        d++;
    };
    hipStream_t ss = c->sub[0];
    hipError_t e = hipSuccess;
#define TRYB(x) if ((e = (x)) != hipSuccess) { if (coder) { bool ov; (void)bwtc_end_n(coder, &ov); } drain(c); return CJS_E_HIP - (int)e; }
    for (u32 f = 0; f < nblocks; f += c->sub_blocks) {
        const u32 nb = nblocks - f < c->sub_blocks ? nblocks - f : c->sub_blocks;
        Pipe P;
        const int rc = block_stages(c, Q, g, f, nb, 0, max_n, P);
        if (rc) { if (coder) { bool ov; (void)bwtc_end_n(coder, &ov); } drain(c); return rc; }
        TRYB(hipMemcpyAsync(hlen.data(), P.nlen, nb * 4, hipMemcpyDeviceToHost, ss));
        TRYB(hipMemcpyAsync(hpos.data(), P.pos, nb * 4, hipMemcpyDeviceToHost, ss));
        TRYB(hipMemcpyAsync(hpidx.data(), P.pidx, nb * 4, hipMemcpyDeviceToHost, ss));
        TRYB(hipMemcpyAsync(hused.data(), P.used, (size_t)nb * 32, hipMemcpyDeviceToHost, ss));
        TRYB(bsync(c, ss));
        size_t total = 0;
        for (u32 b = 0; b < nb; b++) { soff[b] = total; total += (hpos[b] ? hpos[b] - 1u : 0u) + 1u; }   // K2 appends bzip2's EOB; BWTC has none
        if (sym.size() < total) sym.resize(total);
        for (u32 b = 0; b < nb; b++)
            if (hpos[b] > 1u) TRYB(hipMemcpyAsync(sym.data() + soff[b], P.A + (size_t)b * g.stride, (size_t)(hpos[b] - 1u) * 2, hipMemcpyDeviceToHost, ss));
        TRYB(bsync(c, ss));
        for (u32 b = 0; b < nb; b++) {
            while (left == 0) {                                   // the next document that has a block; empty ones on the way
                if (coder) close_doc();
                open_doc();
            }
            bwtc_block(coder, hlen[b], hpidx[b], hused.data() + (size_t)b * 8, sym.data() + soff[b], hpos[b] ? hpos[b] - 1u : 0u);
            left--;
        }
    }
#undef TRYB
    if (coder) close_doc();
    while (d < count) { open_doc(); close_doc(); }                // trailing empty documents (or a batch of nothing else)
    h_out_off[count] = cursor;
    HIP_CHECK_RET(hipEventRecord(c->ev1, st));
    HIP_CHECK_RET(bsync(c, st));
    HIP_CHECK_RET(hipEventElapsedTime(&c->last_ms, c->ev0, c->ev1));
    c->last_blocks = nblocks;
    return overflow || cursor > out_cap ? CJS_E_NOSPACE : (int64_t)cursor;
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
    if (level >= 6) return batch_device_fast(c, d_in, (const u64*)d_off, count, level, d_out, out_cap, (u64*)d_out_off);
    // levels 1-5 stage through the host: the offsets come down, the streams and their offsets go up
    std::vector<u64> h_off((size_t)count + 1), h_oo((size_t)count + 1);
    HIP_CHECK_RET(hipMemcpyAsync(h_off.data(), d_off, ((size_t)count + 1) * 8, hipMemcpyDeviceToHost, c->stream));
    HIP_CHECK_RET(bsync(c, c->stream));
    for (u32 d = 0; d < count; d++) if (h_off[d + 1] < h_off[d]) return CJS_E_ARG;
    const u64 need = (u64)cjs_bwtc_compress_batch_bound(h_off[count], count);
    std::vector<u8> h_out((size_t)(need < out_cap ? need : out_cap) + 1);
    const int64_t n = batch_host_tail(c, d_in, (const u64*)d_off, h_off.data(), count, level, h_out.data(), need < out_cap ? need : out_cap, h_oo.data());
    if (n < 0 && n != CJS_E_NOSPACE) return n;
    HIP_CHECK_RET(hipMemcpyAsync(d_out_off, h_oo.data(), ((size_t)count + 1) * 8, hipMemcpyHostToDevice, c->stream));
    if (n > 0) HIP_CHECK_RET(hipMemcpyAsync(d_out, h_out.data(), (size_t)n, hipMemcpyHostToDevice, c->stream));
    HIP_CHECK_RET(bsync(c, c->stream));
    return n;
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
    if (level <= 5) return batch_host_tail(c, c->din, (const u64*)d_off, (const u64*)off, count, level, out, out_cap, (u64*)out_off);
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
