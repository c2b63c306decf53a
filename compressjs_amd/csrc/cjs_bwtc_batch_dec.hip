// cjs_bwtc_decompress_batch*: many independent BWTC streams in, the decoded documents back to back out, in one call (declared in
// include/compressjs_amd.h).  The reference has no batched entry: result d is what BWTC.decompressFile (lib/BWTC.js:141-233) gives
// for document d alone, i.e. cjs_bwtc_decompress on it.
//
// The fast path - FenwickModel streams (levels 6-9) with their size declared, and with CJS_BWTC_DEC_DEFSUM_DEVICE in the `flags` of
// the _ex entries DefSumModel streams (levels 1-5) too: between upload and download everything runs on the device.  k12_plan reads
// the headers, cuts the scratch and counts the documents of either model, k12_decode (levels 6-9) and k14_decode (levels 1-5), each
// launched only if it has documents, run one range decoder per document (one wave each),
// k6_unbwt_batch inverts the BWT of all their blocks, group after group, and writes every block to its final place.  The host
// waits THREE times, whatever the number of documents (cjs_dbg_bwtc_dec_batch_syncs):
//   1  the plan's totals: how much scratch and how many block rows the admitted documents need (what is allocated);
//   2  the documents' statuses and block rows: who failed, who takes the host path, where every block goes (out_off is the
//      exclusive scan of the decoded sizes, made on the host from this one read-back);
//   3  the end: the documents are in place (device form) or on the host.
// The host path - DefSumModel streams (levels 1-5) without that flag, no size declared, more bytes or blocks than declared, a size beyond the scratch
// budget (CJS_BWTC_DEC_BUDGET bytes, 512 MiB unless set): bwtc_decode_one, what the single call runs, document after document,
// with its own waits.  The device form brings these documents to the host and their bytes back.
#include "cjs_ctx.h"
#include "bwtc_host.h"
#include <stdlib.h>

using namespace cjs;

extern "C" int cjs_dbg_bwtc_dec_batch_syncs(cjs_ctx* c) { return c ? c->bwtc_dec_batch_syncs : 0; }
extern "C" int cjs_dbg_bwtc_dec_batch_fallbacks(cjs_ctx* c) { return c ? c->bwtc_dec_batch_fallbacks : 0; }
static int g_k6_groups = 0;                                       // groups of the last run_groups (cjs_unbwt_linear_batch has no context)
extern "C" int cjs_dbg_k6_groups(void) { return g_k6_groups; }

namespace {

const size_t K6_WS_BUDGET_WORDS = (size_t)128 << 20;              // u32 of list-ranking workspace per group of blocks: 512 MiB

hipError_t dsync(cjs_ctx* c) { c->bwtc_dec_batch_syncs++; return hipStreamSynchronize(c->stream); }

u64 dec_budget() {                                                // (read per call: the tests shrink it)
    const char* ev = getenv("CJS_BWTC_DEC_BUDGET");
    u64 b = ev ? strtoull(ev, nullptr, 10) : (u64)512 << 20;
    return b < 0xFFFFFF00ull ? b : 0xFFFFFF00ull;                 // a document's scratch is 32 bits wide
}

struct Drain {                                                    // nothing of a call is left running when its host buffers go
    hipStream_t st;
    ~Drain() { (void)hipStreamSynchronize(st); }
};

// Blocks [first, rows.size()) cut into groups whose workspace stays inside the budget; wsAt is set per group.  -> group ends
void cut_groups(std::vector<K6Blk>& rows, std::vector<size_t>& ends, size_t* ws_words) {
    size_t g0 = 0, used = 0, most = 0;
    for (size_t k = 0; k < rows.size(); k++) {
        const size_t w = k6_ws_words(rows[k].n);
        if (k > g0 && (used + w > K6_WS_BUDGET_WORDS || k - g0 >= K6_GROUP_MAX)) { ends.push_back(k); g0 = k; used = 0; }
        rows[k].wsAt = used;
        used += w;
        if (used > most) most = used;
    }
    if (!rows.empty()) ends.push_back(rows.size());
    *ws_words = most;
}

int run_groups(const std::vector<K6Blk>& rows, const std::vector<size_t>& ends, const K6Blk* d_rows, const u8* dT, u8* dU, void* ws, hipStream_t st) {
    size_t g0 = 0;
    g_k6_groups = (int)ends.size();
    for (size_t e : ends) {
        u32 max_n = 0;
        for (size_t k = g0; k < e; k++) if (rows[k].n > max_n) max_n = rows[k].n;
        const int rc = k6_unbwt_batch(d_rows + g0, (u32)(e - g0), max_n, dT, dU, ws, st);
        if (rc) return rc;
        g0 = e;
    }
    return CJS_OK;
}

// d_in / d_off on the device.  h_in / h_off: the same on the host, or null (the device form: fetched when a document needs the host
// path).  dev: out / out_off / status / declared are device pointers, else host pointers.
int64_t dec_batch(cjs_ctx* c, const u8* d_in, const u64* d_off, const u8* h_in, const u64* h_off, u32 count, bool dev, u8* out, u64 out_cap,
                  u64* out_off, int32_t* status, int64_t* declared, u32 flags_in) {
    hipStream_t st = c->stream;
    c->bwtc_dec_batch_syncs = 0;
    c->bwtc_dec_batch_fallbacks = 0;
    if (!out) out_cap = 0;
    std::vector<K12Doc> hdoc(count);
    std::vector<K12Row> hrow;
    std::vector<u64> oo((size_t)count + 1), off_copy;
    std::vector<int32_t> hst(count);
    std::vector<int64_t> hdecl(count);
    std::vector<std::vector<u8>> fb;                              // the host path's documents, in order
    std::vector<u32> fb_doc;
    std::vector<u8> doc_in;
    std::vector<K6Blk> rows;
    std::vector<size_t> ends;
    Drain drain = {st};
    // ---- the plan
    const size_t doc_bytes = ((size_t)count * sizeof(K12Doc) + 255) & ~(size_t)255;
    int rc = grow(&c->bd[0], &c->bd_bytes[0], doc_bytes + K12_F_WORDS * 8);
    if (rc) return rc;
    K12Plan Q;
    memset(&Q, 0, sizeof Q);
    Q.in = d_in; Q.off = d_off; Q.count = count; Q.budget = dec_budget();
    Q.opt = (flags_in & CJS_BWTC_DEC_DEFSUM_DEVICE) ? K12_OPT_DEFSUM : 0u;
    Q.doc = (K12Doc*)c->bd[0];
    Q.flags = (u64*)((char*)c->bd[0] + doc_bytes);
    rc = k12_plan_run(Q, st);
    if (rc) return rc;
    u64 flags[K12_F_WORDS];
    HIP_CHECK_RET(hipMemcpyAsync(c->pin[0], Q.flags, sizeof flags, hipMemcpyDeviceToHost, st));
    HIP_CHECK_RET(dsync(c));                                      // 1
    memcpy(flags, c->pin[0], sizeof flags);
    if (flags[K12_F_BAD]) return CJS_E_ARG;
    if (flags[K12_F_SCR] > Q.budget + 4 || flags[K12_F_BLK] > (u64)count + Q.budget / 100000u + 1) return CJS_E_ARG;   // (cannot happen)
    const size_t nrows = (size_t)flags[K12_F_BLK];
    rc = grow(&c->bd[1], &c->bd_bytes[1], nrows * sizeof(K12Row) + 64);
    if (!rc) rc = grow(&c->bd[2], &c->bd_bytes[2], (size_t)flags[K12_F_SCR] + 64);
    if (rc) return rc;
    Q.row = (K12Row*)c->bd[1];
    Q.scr = (u8*)c->bd[2];
    // ---- one range decoder per document: the kernel of either model, if the plan admitted documents of it
    if (flags[K12_F_NFEN]) rc = k12_decode_run(Q, st);
    if (!rc && flags[K12_F_NDEF]) rc = k14_decode_run(Q, st);
    if (rc) return rc;
    hrow.resize(nrows);
    HIP_CHECK_RET(hipMemcpyAsync(hdoc.data(), Q.doc, (size_t)count * sizeof(K12Doc), hipMemcpyDeviceToHost, st));
    if (nrows) HIP_CHECK_RET(hipMemcpyAsync(hrow.data(), Q.row, nrows * sizeof(K12Row), hipMemcpyDeviceToHost, st));
    HIP_CHECK_RET(dsync(c));                                      // 2
    // ---- the host path, document after document
    BwtcDecBufs bufs;
    struct FreeBufs { BwtcDecBufs& b; ~FreeBufs() { bwtc_dec_bufs_free(b); } } free_bufs = {bufs};
    for (u32 d = 0; d < count; d++) {
        hst[d] = hdoc[d].status;
        hdecl[d] = hdoc[d].declared;
        if (hdoc[d].status != K12_HOST) continue;
        if (!h_off) {                                             // the device form: the offsets, once
            off_copy.resize((size_t)count + 1);
            HIP_CHECK_RET(hipMemcpyAsync(off_copy.data(), d_off, ((size_t)count + 1) * 8, hipMemcpyDeviceToHost, st));
            HIP_CHECK_RET(dsync(c));
            h_off = off_copy.data();
        }
        const u64 len = h_off[d + 1] - h_off[d];
        const u8* src = h_in ? h_in + h_off[d] : nullptr;
        if (!h_in) {
            doc_in.resize((size_t)len + 1);
            if (len) HIP_CHECK_RET(hipMemcpyAsync(doc_in.data(), d_in + h_off[d], (size_t)len, hipMemcpyDeviceToHost, st));
            HIP_CHECK_RET(dsync(c));
            src = doc_in.data();
        }
        if (!bufs.ws && (rc = bwtc_dec_bufs_alloc(bufs)) != 0) return rc;
        fb.emplace_back();
        fb_doc.push_back(d);
        int64_t decl = -1;
        rc = bwtc_decode_one(c, bufs, src, len, &decl, fb.back());
        if (rc && rc != BWTC_E_MAGIC && rc != BWTC_E_CORRUPT) return rc;
        hst[d] = rc;
        hdecl[d] = decl;
        c->bwtc_dec_batch_fallbacks++;
    }
    // ---- where every document goes
    {
        size_t f = 0;
        u64 at = 0;
        for (u32 d = 0; d < count; d++) {
            oo[d] = at;
            if (f < fb_doc.size() && fb_doc[f] == d) at += fb[f++].size();
            else if (hst[d] == 0) at += hdoc[d].size;
        }
        oo[count] = at;
    }
    const u64 total = oo[count];
    const bool fits = total <= out_cap;
    u8* dst = out;
    if (!dev || !fits) {                                          // assembled in the context's own buffer: on its way to the host, or retained
        rc = grow(&c->dout, &c->dout_bytes, (size_t)total + 64);
        if (rc) return rc;
        dst = (u8*)c->dout;
    }
    // ---- the inverse BWT of every block, straight to its place
    for (u32 d = 0; d < count; d++) {
        if (hdoc[d].status != 0) continue;
        for (u32 b = 0; b < hdoc[d].nblk; b++) {
            const K12Row& r = hrow[(size_t)hdoc[d].blk0 + b];
            if (r.len == 0) continue;
            K6Blk k;
            k.tAt = hdoc[d].scrAt + r.place; k.uAt = oo[d] + r.place; k.wsAt = 0; k.n = r.len; k.pidx = r.pidx;
            rows.push_back(k);
        }
    }
    if (!rows.empty()) {
        size_t ws_words = 0;
        cut_groups(rows, ends, &ws_words);
        rc = grow(&c->bd[3], &c->bd_bytes[3], rows.size() * sizeof(K6Blk));
        if (!rc) rc = grow(&c->bd[4], &c->bd_bytes[4], ws_words * 4);
        if (rc) return rc;
        HIP_CHECK_RET(hipMemcpyAsync(c->bd[3], rows.data(), rows.size() * sizeof(K6Blk), hipMemcpyHostToDevice, st));
        rc = run_groups(rows, ends, (const K6Blk*)c->bd[3], Q.scr, dst, c->bd[4], st);
        if (rc) return rc;
    }
    for (size_t f = 0; f < fb.size(); f++)
        if (!fb[f].empty()) HIP_CHECK_RET(hipMemcpyAsync(dst + oo[fb_doc[f]], fb[f].data(), fb[f].size(), hipMemcpyHostToDevice, st));
    // ---- delivery
    if (dev) {
        HIP_CHECK_RET(hipMemcpyAsync(out_off, oo.data(), ((size_t)count + 1) * 8, hipMemcpyHostToDevice, st));
        HIP_CHECK_RET(hipMemcpyAsync(status, hst.data(), (size_t)count * 4, hipMemcpyHostToDevice, st));
        if (declared) HIP_CHECK_RET(hipMemcpyAsync(declared, hdecl.data(), (size_t)count * 8, hipMemcpyHostToDevice, st));
    } else {
        memcpy(out_off, oo.data(), ((size_t)count + 1) * 8);
        memcpy(status, hst.data(), (size_t)count * 4);
        if (declared) memcpy(declared, hdecl.data(), (size_t)count * 8);
        if (fits && total) HIP_CHECK_RET(hipMemcpyAsync(out, dst, (size_t)total, hipMemcpyDeviceToHost, st));
    }
    if (!fits) {                                                  // retained for cjs_bwtc_last_size / cjs_bwtc_fetch
        c->bwtc_out.resize((size_t)total);
        HIP_CHECK_RET(hipMemcpyAsync(c->bwtc_out.data(), dst, (size_t)total, hipMemcpyDeviceToHost, st));
    }
    HIP_CHECK_RET(dsync(c));                                      // 3
    return fits ? (int64_t)total : CJS_E_NOSPACE;
}

}  // namespace

extern "C" int64_t cjs_bwtc_decompress_batch_device_ex(cjs_ctx* c, const void* d_in, const uint64_t* d_off, uint32_t count, void* d_out,
                                                       uint64_t out_cap, uint64_t* d_out_off, int32_t* d_status, int64_t* d_declared, uint32_t flags) {
    if (!c || (flags & ~CJS_BWTC_DEC_DEFSUM_DEVICE)) return CJS_E_ARG;
    if (count == 0) return 0;
    if (!d_off || !d_out_off || !d_status) return CJS_E_ARG;
    if (hipSetDevice(c->device) != hipSuccess) return CJS_E_NOGPU;
    return dec_batch(c, (const u8*)d_in, (const u64*)d_off, nullptr, nullptr, count, true, (u8*)d_out, out_cap, (u64*)d_out_off, d_status, d_declared, flags);
}

extern "C" int64_t cjs_bwtc_decompress_batch_ex(cjs_ctx* c, const uint8_t* in, const uint64_t* off, uint32_t count, uint8_t* out,
                                                uint64_t out_cap, uint64_t* out_off, int32_t* status, int64_t* declared, uint32_t flags) {
    if (!c || (flags & ~CJS_BWTC_DEC_DEFSUM_DEVICE)) return CJS_E_ARG;
    if (count == 0) return 0;
    if (!off || !out_off || !status) return CJS_E_ARG;
    for (u32 d = 0; d < count; d++) if (off[d + 1] < off[d]) return CJS_E_ARG;
    const uint64_t base = off[0], total = off[count] - off[0];    // (the documents need not start at in[0])
    if (!in && total) return CJS_E_ARG;
    if (hipSetDevice(c->device) != hipSuccess) return CJS_E_NOGPU;
    // one upload: the streams, then their offsets behind them
    const size_t off_at = (size_t)((total + 64 + 7) & ~(uint64_t)7), off_bytes = ((size_t)count + 1) * 8;
    int rc = grow(&c->din, &c->din_bytes, off_at + off_bytes);
    if (rc) return rc;
    std::vector<u64> rel((size_t)count + 1);
    for (u32 d = 0; d <= count; d++) rel[d] = off[d] - base;
    u64* d_off = (u64*)((char*)c->din + off_at);
    if (total) HIP_CHECK_RET(hipMemcpyAsync(c->din, in + base, total, hipMemcpyHostToDevice, c->stream));
    HIP_CHECK_RET(hipMemcpyAsync(d_off, rel.data(), off_bytes, hipMemcpyHostToDevice, c->stream));
    const int64_t n = dec_batch(c, (const u8*)c->din, d_off, in ? in + base : nullptr, rel.data(), count, false, out, out_cap, (u64*)out_off, status, declared, flags);
    (void)hipStreamSynchronize(c->stream);                        // (`rel` is on its way up until the call's first wait; error paths included)
    return n;
}

// the entries without a flags word: flags = 0, levels 1-5 on the host path
extern "C" int64_t cjs_bwtc_decompress_batch_device(cjs_ctx* c, const void* d_in, const uint64_t* d_off, uint32_t count, void* d_out,
                                                    uint64_t out_cap, uint64_t* d_out_off, int32_t* d_status, int64_t* d_declared) {
    return cjs_bwtc_decompress_batch_device_ex(c, d_in, d_off, count, d_out, out_cap, d_out_off, d_status, d_declared, 0u);
}
extern "C" int64_t cjs_bwtc_decompress_batch(cjs_ctx* c, const uint8_t* in, const uint64_t* off, uint32_t count, uint8_t* out,
                                             uint64_t out_cap, uint64_t* out_off, int32_t* status, int64_t* declared) {
    return cjs_bwtc_decompress_batch_ex(c, in, off, count, out, out_cap, out_off, status, declared, 0u);
}

// BWT.unbwtransform (lib/BWT.js:352-363) of `count` blocks in one call: block k = T[off[k] .. off[k+1]) with primary index
// pidx[k], its text to U at the same place.  Host pointers; what cjs_unbwt_linear gives for every block alone.
extern "C" int32_t cjs_unbwt_linear_batch(const uint8_t* T, const uint64_t* off, const uint32_t* pidx, uint32_t count, uint8_t* U) {
    if (count == 0) return CJS_OK;
    if (!off || !pidx) return CJS_E_ARG;
    std::vector<K6Blk> rows;
    std::vector<size_t> ends;
    for (u32 k = 0; k < count; k++) {
        if (off[k + 1] < off[k] || off[k + 1] - off[k] > 0xFFFFFFF0ull || pidx[k] > off[k + 1] - off[k]) return CJS_E_ARG;
        if (off[k + 1] == off[k]) continue;
        K6Blk b;
        b.tAt = off[k] - off[0]; b.uAt = b.tAt; b.wsAt = 0; b.n = (u32)(off[k + 1] - off[k]); b.pidx = pidx[k];
        rows.push_back(b);
    }
    if (rows.empty()) return CJS_OK;
    if (!T || !U) return CJS_E_ARG;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return CJS_E_NOGPU;
    const size_t total = (size_t)(off[count] - off[0]);
    size_t ws_words = 0;
    cut_groups(rows, ends, &ws_words);
    u8 *dT = nullptr, *dU = nullptr; void *ws = nullptr, *dB = nullptr;
    hipStream_t st = nullptr;
    hipError_t e;
    int rc = CJS_OK;
#define TRY(x) if ((e = (x)) != hipSuccess) { rc = CJS_E_HIP - (int)e; goto done; }
    TRY(hipStreamCreate(&st));
    TRY(hipMalloc((void**)&dT, total));
    TRY(hipMalloc((void**)&dU, total));
    TRY(hipMalloc(&ws, ws_words * 4));
    TRY(hipMalloc(&dB, rows.size() * sizeof(K6Blk)));
    TRY(hipMemcpyAsync(dT, T + off[0], total, hipMemcpyHostToDevice, st));
    TRY(hipMemcpyAsync(dB, rows.data(), rows.size() * sizeof(K6Blk), hipMemcpyHostToDevice, st));
    TRY(hipMemsetAsync(dU, 0, total, st));
    rc = run_groups(rows, ends, (const K6Blk*)dB, dT, dU, ws, st);
    if (rc) goto done;
    TRY(hipStreamSynchronize(st));
    TRY(hipMemcpy(U + off[0], dU, total, hipMemcpyDeviceToHost));
done:
#undef TRY
    if (st) { (void)hipStreamSynchronize(st); (void)hipStreamDestroy(st); }
    (void)hipFree(dT); (void)hipFree(dU); (void)hipFree(ws); (void)hipFree(dB);
    return rc;
}
