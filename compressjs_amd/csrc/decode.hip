// Host side of the GPU bzip2 decoder: Bunzip.decode / decodeBlock / table (lib/Bzip2.js:454-548).
//
// The reference is strictly sequential: block k+1's header is read where block k's last symbol
// ended.  Here every occurrence of the block magic is a *candidate* (k7_scan_magic), candidates are
// entropy-decoded in parallel batches (k7_decode), and this file then walks the real chain through
// the results exactly in the reference's order - stream header, block, block, ..., end-of-stream
// magic, stream CRC, next stream if `multistream` - so that the outcome (bytes, or which error is
// raised first) is the reference's.  Blocks on the chain go through K8 (inverse BWT) and K9
// (un-RLE1, CRC) in the same batches.  There is no CPU decode path.
#include "decode.h"
#include "decode_host.h"
#include <algorithm>
#include <atomic>
#include <vector>
#include <string.h>
#include <stdio.h>
#include <stdlib.h>

#define WHOLEPI 0x314159265359ull
#define SQRTPI 0x177245385090ull

struct DecState {
    u32 slots = 0;
    u8* d_in = nullptr; size_t in_cap = 0;
    u64* d_cand = nullptr; size_t cand_cap = 0; u32* d_ncand = nullptr;      // (cand_cap, dcand_cap: candidates, not bytes)
    void* slab = nullptr;            // per-slot arrays
    DecBuf D = {};
    u64* d_bcand = nullptr; u32* d_slotOf = nullptr; u64* d_outOff = nullptr; u32* d_crcOut = nullptr;
    u8* d_out = nullptr; size_t out_cap = 0; u64 out_size = 0;
    int detail = 0; u32 crc_got = 0, crc_want = 0;
    std::vector<u64> tab_pos, tab_size;
    // a batch of documents (dec_batch): grow-only
    u8* d_raw = nullptr; size_t raw_cap = 0;          // the host form's packed documents
    void* d_meta = nullptr; size_t meta_cap = 0;      // bases, offsets, heads, chunk -> document, outcome records
    DecCand* d_dcand = nullptr; size_t dcand_cap = 0;
    u32* d_blim = nullptr;                            // [slots] limit chunk of the candidates of a k7_decode launch (in the slab)
};

// host<->device synchronisations of the last decode call of the process (cjs_dbg_dec_syncs): stream syncs and synchronous copies
static std::atomic<int> g_dec_syncs{0};
int dec_sync_count() { return g_dec_syncs.load(); }
void dec_sync_note() { g_dec_syncs++; }
static hipError_t dec_sync(hipStream_t st) { g_dec_syncs++; return hipStreamSynchronize(st); }

#define TRYH(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) return CJS_E_HIP - (int)e_; } while (0)

static size_t al(size_t v) { return (v + 255) & ~(size_t)255; }

// a grow-only device array of `elem`-byte items with room for `need` of them: a quarter more with `slack`, else exactly `need`
// (d_in and the candidate arrays, which are sized by the input alone)
static int grow_dev(void** p, size_t* have, size_t need, size_t elem = 1, bool slack = true) {
    if (need <= *have) return CJS_OK;
    (void)hipFree(*p); *p = nullptr; *have = 0;
    if (slack) need += need / 4;
    TRYH(hipMalloc(p, need * elem));
    *have = need;
    return CJS_OK;
}

static int dec_alloc(DecState& S, u32 slots) {
    if (S.slab) { (void)hipFree(S.slab); S.slab = nullptr; }
    S.slots = 0;                                  // nothing usable until the new slab exists
    const size_t n = slots;
    size_t tot = 0;
    const size_t o_tt = tot;        tot += al(n * DEC_STRIDE);
    const size_t o_res = tot;       tot += al(n * sizeof(DecResult));
    const size_t o_sel = tot;       tot += al(n * 4160 * 4);
    const size_t o_word = tot;      tot += al(n * DEC_STRIDE * 4);
    const size_t o_hist = tot;      tot += al(n * DEC_TILES * 256 * 4);
    const size_t o_succ = tot;      tot += al(n * DEC_MAXSPL * 4);
    const size_t o_len = tot;       tot += al(n * DEC_MAXSPL * 4);
    const size_t o_off = tot;       tot += al(n * DEC_MAXSPL * 4);
    const size_t o_flags = tot;     tot += al(n * 4);
    const size_t o_pre = tot;       tot += al(n * DEC_STRIDE);
    const size_t o_fn = tot;        tot += al(n * DEC_TILES * 4);
    const size_t o_state = tot;     tot += al(n * DEC_TILES);
    const size_t o_isc = tot;       tot += al(n * (DEC_STRIDE / 32) * 4);
    const size_t o_tlen = tot;      tot += al(n * DEC_TILES * 4);
    const size_t o_bout = tot;      tot += al(n * 4);
    const size_t o_bcand = tot;     tot += al(n * 8);
    const size_t o_slotof = tot;    tot += al(n * 4);
    const size_t o_outoff = tot;    tot += al(n * 8);
    const size_t o_crc = tot;       tot += al(n * 4);
    const size_t o_blim = tot;      tot += al(n * 4);
    TRYH(hipMalloc(&S.slab, tot));
    S.slots = slots;
    u8* b = (u8*)S.slab;
    { const u32* keep_in = S.D.in32; const u64 keep_zc = S.D.zeroChunk; memset(&S.D, 0, sizeof S.D); S.D.in32 = keep_in; S.D.zeroChunk = keep_zc; }
    S.D.tt = b + o_tt; S.D.ttStride = DEC_STRIDE;
    S.D.res = (DecResult*)(b + o_res);
    S.D.sel = (u32*)(b + o_sel);
    S.D.word = (u32*)(b + o_word);
    S.D.tileHist = (u32*)(b + o_hist);
    S.D.splSucc = (u32*)(b + o_succ); S.D.splLen = (u32*)(b + o_len); S.D.splOff = (u32*)(b + o_off);
    S.D.flags = (u32*)(b + o_flags);
    S.D.pre = b + o_pre;
    S.D.tileFn = (u32*)(b + o_fn); S.D.tileState = b + o_state;
    S.D.isCount = (u32*)(b + o_isc); S.D.tileLen = (u32*)(b + o_tlen); S.D.blkOut = (u32*)(b + o_bout);
    S.d_bcand = (u64*)(b + o_bcand); S.d_slotOf = (u32*)(b + o_slotof);
    S.d_outOff = (u64*)(b + o_outoff); S.d_crcOut = (u32*)(b + o_crc);
    S.d_blim = (u32*)(b + o_blim);
    S.D.cand = S.d_bcand; S.D.slotOf = S.d_slotOf; S.D.outOff = S.d_outOff; S.D.crcOut = S.d_crcOut;
    if (!S.d_ncand) TRYH(hipMalloc((void**)&S.d_ncand, 256));
    return CJS_OK;
}

// slots for the blocks of this stream: as many as it has candidates, within [min_slots, DEC_MAX_SLOTS].
// One k7_decode wave set per block is latency-bound, so throughput comes from the number of blocks in flight
// (4 per CU fit); 5.7 MB of HBM per slot.
#define DEC_MAX_SLOTS 4096u
// The slab never shrinks while the context lives, so its size is capped: CJS_DEC_MAX_SLOTS (env), else what fits
// a quarter of the HBM that is free right now (a 400 MB level-1 stream, or a small stream stuffed with fake
// block magics, has thousands of candidates: 4096 slots would pin 23 GB).  Fewer slots only mean more batches.
static u32 dec_slot_limit(u32 min_slots) {
    const u32 env_cap = []() -> u32 { const char* e = getenv("CJS_DEC_MAX_SLOTS"); return e ? (u32)strtoul(e, nullptr, 10) : 0u; }();   // (read per call)
    u32 lim = DEC_MAX_SLOTS;
    if (env_cap) lim = env_cap;
    else {
        size_t fr = 0, tot = 0;
        if (hipMemGetInfo(&fr, &tot) == hipSuccess && fr) {
            const size_t per = (size_t)DEC_STRIDE * 6 + 4160 * 4 + DEC_TILES * 1040 + DEC_MAXSPL * 12 + 4096;
            const size_t fit = fr / 4 / per;
            if (fit < lim) lim = (u32)fit;
        }
    }
    return lim < min_slots ? min_slots : lim;
}
static int dec_fit_slots(DecState& S, u32 min_slots, size_t ncand) {
    u32 want = (u32)std::min<size_t>(dec_slot_limit(min_slots), ncand);
    if (want < min_slots) want = min_slots;
    if (want <= S.slots) return CJS_OK;
    want = (want + 63u) & ~63u;
    for (;;) {                                   // out of memory: halve, down to the minimum the caller can work with
        const int rc = dec_alloc(S, want);
        if (rc == CJS_OK || want <= ((min_slots + 63u) & ~63u)) return rc;
        want = ((want / 2 > min_slots ? want / 2 : min_slots) + 63u) & ~63u;
    }
}

void dec_free(DecState* S) {
    if (!S) return;
    (void)hipFree(S->d_in); (void)hipFree(S->d_cand); (void)hipFree(S->d_ncand); (void)hipFree(S->slab); (void)hipFree(S->d_out);
    (void)hipFree(S->d_raw); (void)hipFree(S->d_meta); (void)hipFree(S->d_dcand);
    delete S;
}

// every decode call starts here: the state, made on first use, with the last call's outcome cleared
static int dec_begin(DecState** ps, u32 slots) {
    if (!*ps) {
        DecState* S = new DecState();
        const int rc = dec_alloc(*S, slots);
        if (rc) { dec_free(S); return rc; }
        *ps = S;
    }
    DecState& S = **ps;
    g_dec_syncs = 0;
    S.out_size = 0; S.detail = 0; S.crc_got = S.crc_want = 0;
    S.tab_pos.clear(); S.tab_size.clear();
    return CJS_OK;
}

static int ensure_out(DecState& S, u64 need, hipStream_t st) {
    if (need <= S.out_cap) return CJS_OK;
    size_t cap = S.out_cap ? S.out_cap * 2 : (size_t)64 << 20;
    if (cap < need) cap = need;
    cap = (cap + ((size_t)1 << 20)) & ~(((size_t)1 << 20) - 1);
    u8* p = nullptr;
    TRYH(hipMalloc((void**)&p, cap));
    if (S.out_size) {
        hipError_t e = hipMemcpyAsync(p, S.d_out, S.out_size, hipMemcpyDeviceToDevice, st);
        if (e == hipSuccess) e = dec_sync(st);
        if (e != hipSuccess) { (void)hipFree(p); return CJS_E_HIP - (int)e; }
    }
    (void)hipFree(S.d_out);
    S.d_out = p; S.out_cap = cap;
    return CJS_OK;
}

// the stream, padded with zeros (bits past EOF read as 0, lib/BitStream.js:84), resident in HBM
static int stage_input(DecState& S, const u8* in, u64 len, bool in_dev, hipStream_t st) {
    const size_t need = ((len + 255) & ~(size_t)255) + 1024;
    int rc = grow_dev((void**)&S.d_in, &S.in_cap, need, 1, false);
    if (rc) return rc;
    TRYH(hipMemsetAsync(S.d_in + (len & ~(u64)255), 0, need - (len & ~(u64)255), st));
    if (len) TRYH(hipMemcpyAsync(S.d_in, in, len, in_dev ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, st));
    // a 48-bit pattern cannot occur more often than every 6 bytes
    rc = grow_dev((void**)&S.d_cand, &S.cand_cap, (size_t)std::min<u64>(len / 4 + 16, 1u << 27), 8, false);
    if (rc) return rc;
    S.D.in32 = (const u32*)S.d_in;
    S.D.zeroChunk = ((len + 255) >> 8) + 1;          // [zeroChunk*256, +256) is inside the 1024 zero bytes
    S.D.candLim = nullptr;                           // one stream: every block reads zeros from zeroChunk on
    return CJS_OK;
}

struct Walker {
    DecState& S;
    hipStream_t st;
    const u8* host_in;     // non-null when the caller's buffer is host memory
    u64 len;
    int rd_err;
    // up to 64 bits at absolute bit position p, zero extended
    u64 rd(u64 p, int n) {
        u8 b[16];
        memset(b, 0, sizeof b);
        const u64 byte = p >> 3;
        if (byte < len) {
            const size_t k = (size_t)std::min<u64>(16, len - byte);
            if (host_in) memcpy(b, host_in + byte, k);
            else {
                hipError_t e = hipMemcpyAsync(b, S.d_in + byte, k, hipMemcpyDeviceToHost, st);
                if (e == hipSuccess) e = dec_sync(st);
                if (e != hipSuccess) rd_err = CJS_E_HIP - (int)e;
            }
        }
        u64 v = 0;
        for (int i = 0; i < n; i++) {
            const u64 q = (p & 7u) + (u64)i;
            v = (v << 1) | ((b[q >> 3] >> (7 - (q & 7u))) & 1u);
        }
        return v;
    }
};

static int fail(DecState& S, int code, int detail, u32 got = 0, u32 want = 0) {
    S.detail = detail; S.crc_got = got; S.crc_want = want;
    return code;
}

// the 4-byte stream header `h` (lib/Bzip2.js:137-152); have: the document holds all 4 bytes.  0 or an error
static int check_header(DecState& S, bool have, u32 h, u32* dbufSize) {
    if (!have || (h >> 8) != 0x425a68u) return fail(S, DEC_NOT_BZIP, DEC_DETAIL_BAD_MAGIC);
    const int level = (int)(h & 0xffu) - '0';
    if (level < 1 || level > 9) return fail(S, DEC_NOT_BZIP, DEC_DETAIL_LEVEL);
    *dbufSize = 100000u * (u32)level;
    return 0;
}
// the same on the 4 bytes at byte `base` of the single stream, fetched only when it holds them
static int read_header(DecState& S, Walker& W, u64 base, u32* dbufSize) {
    const bool have = W.len >= base + 4;
    return check_header(S, have, have ? (u32)W.rd(base * 8, 32) : 0, dbufSize);
}

// the reference's per-block checks, in its order, on a k7_decode result
static int block_error(DecState& S, const DecResult& r, u32 dbufSize) {
    if (r.status == DEC_OBSOLETE) return fail(S, DEC_OBSOLETE, DEC_DETAIL_NONE);                // :174-175
    if (r.origPtr > dbufSize) return fail(S, DEC_DATA_ERROR, DEC_DETAIL_ORIGPTR);                // :177-178
    if (r.status) return fail(S, r.status, DEC_DETAIL_NONE);
    if (r.n > dbufSize) return fail(S, DEC_DATA_ERROR, DEC_DETAIL_NONE);                         // :342,:360 with this stream's dbufSize
    return 0;
}

struct ValidBlk { u32 slot, crc; u64 pos; };       // a block on the chain: its slot, its stored CRC, its bit position

// K8 + K9 of the chain blocks of one slot batch: their bytes go to S.d_out from S.out_size on, in the order of `valid`.  Gives
// per block its decoded size, the CRC of its bytes and its offset in S.d_out, and decides nothing: S.out_size, the table and
// what a CRC that differs means are the caller's.  Returns 0 or an error.
static int run_k8k9(DecState& S, hipStream_t st, const std::vector<ValidBlk>& valid, std::vector<u32>& size, std::vector<u32>& crc,
                    std::vector<u64>& outOff) {
    const u32 nv = (u32)valid.size();
    size.resize(nv); crc.resize(nv); outOff.resize(nv);
    if (!nv) return 0;
    std::vector<u32> slotOf(nv);
    for (u32 k = 0; k < nv; k++) slotOf[k] = valid[k].slot;
    TRYH(hipMemcpyAsync(S.d_slotOf, slotOf.data(), nv * 4, hipMemcpyHostToDevice, st));
    int rc = k8_run(S.D, nv, st);
    if (rc) return rc;
    rc = k9_sizes(S.D, nv, st);
    if (rc) return rc;
    std::vector<u32> blkOut(S.slots);
    TRYH(hipMemcpyAsync(blkOut.data(), S.D.blkOut, S.slots * 4, hipMemcpyDeviceToHost, st));
    TRYH(dec_sync(st));
    u64 o = S.out_size;
    for (u32 k = 0; k < nv; k++) { size[k] = blkOut[valid[k].slot]; outOff[k] = o; o += size[k]; }
    rc = ensure_out(S, o + 64, st);
    if (rc) return rc;
    S.D.out = S.d_out;
    TRYH(hipMemcpyAsync(S.d_outOff, outOff.data(), nv * 8, hipMemcpyHostToDevice, st));
    rc = k9_expand(S.D, nv, st);
    if (rc) return rc;
    TRYH(hipMemcpyAsync(crc.data(), S.d_crcOut, nv * 4, hipMemcpyDeviceToHost, st));
    TRYH(dec_sync(st));
    return 0;
}

// the single stream's K8/K9 step: the blocks in the reference's order, up to the first whose CRC differs
static int append_blocks(DecState& S, hipStream_t st, std::vector<ValidBlk>& valid) {
    std::vector<u32> size, crc;
    std::vector<u64> outOff;
    const int rc = run_k8k9(S, st, valid, size, crc, outOff);
    if (rc) return rc;
    for (size_t k = 0; k < valid.size(); k++) {
        S.out_size += size[k];                     // the reference has written the block before it compares the CRC (:437-445)
        if (crc[k] != valid[k].crc) return fail(S, DEC_DATA_ERROR, DEC_DETAIL_BLOCK_CRC, crc[k], valid[k].crc);
        S.tab_pos.push_back(valid[k].pos);
        S.tab_size.push_back(size[k]);
    }
    valid.clear();
    return 0;
}

// lim (a batch of documents): the limit chunk of every candidate
static int decode_batch(DecState& S, hipStream_t st, const u64* pos, u32 count, std::vector<DecResult>& res, const u32* lim = nullptr) {
    std::vector<u64> enc(count);
    for (u32 i = 0; i < count; i++) enc[i] = pos[i] << 1;
    TRYH(hipMemcpyAsync(S.d_bcand, enc.data(), (size_t)count * 8, hipMemcpyHostToDevice, st));
    if (lim) TRYH(hipMemcpyAsync(S.d_blim, lim, (size_t)count * 4, hipMemcpyHostToDevice, st));
    const int rc = k7_run(S.D, 0, count, st);
    if (rc) return rc;
    res.resize(count);
    TRYH(hipMemcpyAsync(res.data(), S.D.res, (size_t)count * sizeof(DecResult), hipMemcpyDeviceToHost, st));
    TRYH(dec_sync(st));
    if (getenv("CJS_DEC_TRACE")) {
        u64 cy = 0, sy = 0, by = 0, pw = 0, cw = 0;
        for (u32 i = 0; i < count; i++) { cy += res[i].cycles; sy += res[i].symbols; by += res[i].n; pw += res[i].pwait; cw += res[i].cwait; }
        fprintf(stderr, "[k7] %u blocks: %.1f Mcycles/block, %.0f symbols/block, %.0f bytes/block, %.1f cycles/symbol (boundary wave waits %.1f, symbol wave waits %.1f)\n",
                count, cy / 1e6 / count, (double)sy / count, (double)by / count, sy ? (double)cy / sy : 0.0,
                sy ? (double)pw / sy : 0.0, sy ? (double)cw / sy : 0.0);
        u64 pf[14] = {0};
        for (u32 i = 0; i < count; i++) for (int k = 0; k < 14; k++) pf[k] += res[i].prof[k];
        if (pf[2] && sy)                                           // a -DK7_PROF build
            fprintf(stderr, "[k7] clocks/symbol  A: group set-up %.1f, row fill + row end %.1f, walk %.1f, group end + hand-over %.1f | B: wait %.1f, symbols %.1f, "
                    "rows %.1f | C: MTF %.1f, wait %.1f | D: expand %.1f, wait %.1f\n", (double)pf[0] / sy, (double)pf[1] / sy, (double)pf[2] / sy, (double)pf[3] / sy,
                    (double)pf[5] / sy, (double)pf[6] / sy, (double)pf[7] / sy, (double)pf[10] / sy, (double)pf[11] / sy, (double)pf[12] / sy, (double)pf[13] / sy);
    }
    return 0;
}

// the block candidates of a call, and the slot batch of them that k7_decode decoded last
struct Slots {
    std::vector<u64> bpos;               // bit positions of the block magics, ascending
    std::vector<u32> blim;               // (a batch of documents) their limit chunks
    std::vector<DecResult> res;          // of candidates [first, first + count)
    u32 first = 0, count = 0;
};
static int decode_from(DecState& S, hipStream_t st, Slots& w, u32 need) {
    w.first = need;
    w.count = (u32)std::min<size_t>(S.slots, w.bpos.size() - need);
    return decode_batch(S, st, w.bpos.data() + need, w.count, w.res, w.blim.empty() ? nullptr : w.blim.data() + need);
}

// Where a walk finds its document's candidates and the words behind an end-of-stream magic.  A source has B and len - the
// document's first bit among the candidates' positions and its length in bytes -, find(bit): -1 when no magic starts at that bit,
// else whether it is the end-of-stream one - and for the end magic found last stream_crc(p) and header(base): the 32 bits behind
// it and the 4 bytes at the next byte boundary.
static u64 cand_key(u64 c) { return c; }
static u64 cand_key(const DecCand& c) { return c.key; }
template <class C> static const C* cand_at(const std::vector<C>& cand, u64 bit) {       // cand: ascending by key = (bit << 1) | end
    const auto it = std::lower_bound(cand.begin(), cand.end(), bit << 1, [](const C& x, u64 k) { return cand_key(x) < k; });
    return it != cand.end() && (cand_key(*it) >> 1) == bit ? &*it : nullptr;
}
// The single stream reads the words where the chain meets an end magic (Walker::rd: a copy and a wait each in the device form;
// fetched for every candidate, a stream stuffed with fake end magics would pay for all of them).
struct StreamSrc {
    Walker& W; const std::vector<u64>& cand; u64 B, len;
    int find(u64 bit) const { const u64* at = cand_at(cand, bit); return at ? (int)(*at & 1u) : -1; }
    u32 stream_crc(u64 p) { return (u32)W.rd(p + 48, 32); }
    u32 header(u64 base) { return (u32)W.rd(base * 8, 32); }
};
// A document of a batch has them in the candidate's record (k7_scan_docs); cand: of the whole batch.
struct BatchSrc {
    const std::vector<DecCand>& cand; u64 B, len; const DecCand* at;
    int find(u64 bit) { at = cand_at(cand, bit); return at ? (int)(at->key & 1u) : -1; }
    u32 stream_crc(u64) const { return at->a; }
    u32 header(u64) const { return at->b; }
};

struct Chain { u64 p; u32 dbufSize, streamCRC; };      // a walk in progress: bit position in the document, the stream's dbufSize and CRC so far

// One document's chain from c.p on, in the reference's order: block, block, ..., end-of-stream magic, stream CRC, and with
// `multistream` the next stream's header and so on.  The blocks on the chain are appended to `valid`.  Returns 0 when the
// document is finished, an Err code when it fails (through fail()), 1 when the next block - candidate *need - is outside the
// decoded slot batch.
template <class Src>
static int walk_chain(DecState& S, Src& src, Chain& c, int multistream, bool check_stream_crc, const Slots& w,
                      std::vector<ValidBlk>& valid, u32* need) {
    const auto eof = [&src](u64 q) { return ((q + 7) >> 3) >= src.len; };        // lib/Util.js:30 on the coerced buffer stream
    while (!eof(c.p)) {                                                          // :462
        const int end = src.find(src.B + c.p);
        if (end < 0) return fail(S, DEC_NOT_BZIP, DEC_DETAIL_NONE);              // :160-161
        if (end) {                                                               // end of stream :157-159,:465-477
            const u32 target = src.stream_crc(c.p);
            if (check_stream_crc && target != c.streamCRC) return fail(S, DEC_DATA_ERROR, DEC_DETAIL_STREAM_CRC, c.streamCRC, target);
            if (!multistream || eof(c.p + 80)) return 0;
            const u64 base = (c.p + 80 + 7) >> 3;
            const bool have = src.len >= base + 4;
            const int rc = check_header(S, have, have ? src.header(base) : 0, &c.dbufSize);
            if (rc) return rc;
            c.p = (base + 4) * 8;
            c.streamCRC = 0;
            continue;
        }
        const u32 idx = (u32)(std::lower_bound(w.bpos.begin(), w.bpos.end(), src.B + c.p) - w.bpos.begin());
        if (idx < w.first || idx >= w.first + w.count) { *need = idx; return 1; }
        const DecResult& r = w.res[idx - w.first];
        c.streamCRC = r.crc ^ ((c.streamCRC << 1) | (c.streamCRC >> 31));        // :163-164
        const int rc = block_error(S, r, c.dbufSize);
        if (rc) return rc;
        valid.push_back({idx - w.first, r.crc, src.B + c.p});
        c.p = r.endbit - src.B;
    }
    return 0;
}

int64_t dec_stream(DecState** ps, u32 slots, hipStream_t st, const u8* in, u64 len, bool in_dev, int multistream,
                   bool check_stream_crc) {
    int rc = dec_begin(ps, slots);
    if (rc) return rc;
    DecState& S = **ps;
    Walker W = {S, st, in_dev ? nullptr : in, len, 0};
    rc = stage_input(S, in, len, in_dev, st);
    if (rc) return rc;
    Chain c = {32, 0, 0};
    rc = read_header(S, W, 0, &c.dbufSize);                                      // :137-152, before anything else
    if (rc) return rc;
    // candidates
    rc = k7_scan(S.d_in, len, 32, S.d_cand, S.d_ncand, (u32)S.cand_cap, st);
    if (rc) return rc;
    u32 nc = 0;
    TRYH(hipMemcpyAsync(&nc, S.d_ncand, 4, hipMemcpyDeviceToHost, st));
    TRYH(dec_sync(st));
    if (nc > S.cand_cap) return CJS_E_UNSUPPORTED;                               // only when the 2^27 cap on candidates is hit
    std::vector<u64> cand(nc);
    if (nc) { g_dec_syncs++; TRYH(hipMemcpy(cand.data(), S.d_cand, (size_t)nc * 8, hipMemcpyDeviceToHost)); }
    std::sort(cand.begin(), cand.end());
    Slots w;
    for (u64 x : cand) if (!(x & 1u)) w.bpos.push_back(x >> 1);
    rc = dec_fit_slots(S, slots, w.bpos.size());
    if (rc) return rc;

    StreamSrc src = {W, cand, 0, len};
    std::vector<ValidBlk> valid;
    for (;;) {
        u32 need = 0;
        const int term = walk_chain(S, src, c, multistream, check_stream_crc, w, valid, &need);
        if (W.rd_err) return W.rd_err;
        // A CRC error of the blocks in front of the point where the walk stopped comes first.  Without one the walk's own error
        // stands as it is: the step writes S.detail and the CRC pair only through that fail().
        rc = append_blocks(S, st, valid);
        if (rc) return rc;
        if (term < 0) return term;
        if (term == 0) return (int64_t)S.out_size;
        rc = decode_from(S, st, w, need);
        if (rc) return rc;
    }
}

// Bunzip.decodeBlock (lib/Bzip2.js:482-503)
int64_t dec_block(DecState** ps, u32 slots, hipStream_t st, const u8* in, u64 len, u64 bitpos) {
    int rc = dec_begin(ps, slots);
    if (rc) return rc;
    DecState& S = **ps;
    Walker W = {S, st, in, len, 0};
    u32 dbufSize = 0;
    rc = read_header(S, W, 0, &dbufSize);
    if (rc) return rc;
    const u64 h = W.rd(bitpos, 48);
    if (h == SQRTPI) return 0;
    if (h != WHOLEPI) return fail(S, DEC_NOT_BZIP, DEC_DETAIL_NONE);
    rc = stage_input(S, in, len, false, st);
    if (rc) return rc;
    std::vector<DecResult> res;
    rc = decode_batch(S, st, &bitpos, 1, res);
    if (rc) return rc;
    rc = block_error(S, res[0], dbufSize);
    if (rc) return rc;
    std::vector<ValidBlk> valid = {{0, res[0].crc, bitpos}};
    rc = append_blocks(S, st, valid);
    if (rc) return rc;
    return (int64_t)S.out_size;
}

// ---------------------------------------------------------------------------------------------
// A batch of documents (cjs_bz2_decompress_batch): document d decodes as Bzip2.decompressFile (lib/Bzip2.js:454-481) does on it
// alone.  One staging pass, one scan and shared slot batches for all of them (k7_docs.hip).  The chain walk is walk_chain, the one
// dec_stream runs, once per document against the document's base and length, over the sorted candidates of the whole batch; only
// its source differs (BatchSrc): everything the walk reads - headers, stream CRCs, follow-on headers - came to the host in bulk
// with the candidates.
// ---------------------------------------------------------------------------------------------
struct DocOut { int status; u32 detail, got, want; u64 src, size; bool crc_bad; };

static void doc_fail(DecState& S, DocOut& o, int code) { o.status = code; o.detail = (u32)S.detail; o.got = S.crc_got; o.want = S.crc_want; }

// The batch's K8/K9 step: the chain blocks of one slot batch, whatever documents they belong to (vdoc[k]: the document of
// valid[k]; `valid` is in document order, so the decoded bytes of a document are contiguous).  A block whose CRC differs fails its
// document unless an earlier block already has: the reference meets block CRCs in stream order, and every block listed here lies
// in front of the point where the walk stopped.
static int append_docs(DecState& S, hipStream_t st, std::vector<ValidBlk>& valid, std::vector<u32>& vdoc, std::vector<DocOut>& R) {
    std::vector<u32> size, crc;
    std::vector<u64> outOff;
    const int rc = run_k8k9(S, st, valid, size, crc, outOff);
    if (rc) return rc;
    for (size_t k = 0; k < valid.size(); k++) {
        DocOut& d = R[vdoc[k]];
        if (!d.size) d.src = outOff[k];
        d.size += size[k];
        S.out_size += size[k];
        if (crc[k] != valid[k].crc && !d.crc_bad) {
            d.crc_bad = true;
            d.status = DEC_DATA_ERROR; d.detail = DEC_DETAIL_BLOCK_CRC; d.got = crc[k]; d.want = valid[k].crc;
        }
    }
    valid.clear(); vdoc.clear();
    return 0;
}

// The outcome records of a call's documents (requests): failed ones contribute nothing and the gaps they left in the decoded bytes are
// closed; out_off / status / detail go to the caller's arrays (dev: device pointers, through d_rec).  Returns the total.
static int64_t docs_deliver(DecState& S, hipStream_t st, const std::vector<DocOut>& R, DecDocRec* d_rec, bool dev, u64* out_off,
                            int* status, u32* detail) {
    const u32 count = (u32)R.size();
    int rc = 0;
    // failed documents contribute nothing; the gaps they left are closed
    std::vector<DecDocRec> rec((size_t)count + 1);
    u64 total = 0;
    bool gap = false;
    for (u32 k = 0; k < count; k++) {
        const DocOut& o = R[k];
        const u64 n = o.status ? 0 : o.size;
        if (n && o.src != total) gap = true;
        rec[k] = {o.src, total, o.status, o.detail, o.got, o.want};
        total += n;
    }
    rec[count] = {0, total, 0, 0, 0, 0};
    if (dev || gap) TRYH(hipMemcpyAsync(d_rec, rec.data(), rec.size() * sizeof(DecDocRec), hipMemcpyHostToDevice, st));
    if (gap) {
        u8* q = nullptr;
        TRYH(hipMalloc((void**)&q, S.out_cap));
        rc = k9_docs_compact(d_rec, count, S.d_out, q, total, st);
        const hipError_t e = dec_sync(st);
        if (rc || e != hipSuccess) { (void)hipFree(q); return rc ? rc : CJS_E_HIP - (int)e; }
        (void)hipFree(S.d_out);
        S.d_out = q;
    }
    S.out_size = total;
    if (dev) {
        rc = k9_docs_finish(d_rec, count, out_off, status, detail, st);
        if (rc) return rc;
    } else {
        for (u32 k = 0; k <= count; k++) out_off[k] = rec[k].dst;
        for (u32 k = 0; k < count; k++) {
            status[k] = rec[k].status;
            if (detail) { detail[3 * (size_t)k] = rec[k].detail; detail[3 * (size_t)k + 1] = rec[k].got; detail[3 * (size_t)k + 2] = rec[k].want; }
        }
    }
    return (int64_t)total;
}

int64_t dec_batch(DecState** ps, u32 slots, hipStream_t st, const u8* in, const u64* off, u32 count, bool dev, int multistream,
                  u64* out_off, int* status, u32* detail) {
    int rc = dec_begin(ps, slots);
    if (rc) return rc;
    DecState& S = **ps;
    // the offsets on the host; the staged layout
    std::vector<u64> offh((size_t)count + 1);
    if (dev) {
        TRYH(hipMemcpyAsync(offh.data(), off, offh.size() * 8, hipMemcpyDeviceToHost, st));
        TRYH(dec_sync(st));
    } else memcpy(offh.data(), off, offh.size() * 8);
    for (u32 d = 0; d < count; d++) if (offh[d + 1] < offh[d]) return CJS_E_ARG;
    const u64 in_first = offh[0], in_len = offh[count] - offh[0];
    if (!in && in_len) return CJS_E_ARG;
    std::vector<u64> base((size_t)count + 1);
    base[0] = 0;
    for (u32 d = 0; d < count; d++) base[d + 1] = al(base[d] + (offh[d + 1] - offh[d]) + 8);
    const u64 staged = base[count];
    const size_t nchunk = (size_t)(staged >> 8);
    // device side: bases | offsets (host form) | heads | chunk -> document | outcome records
    const size_t o_base = 0, o_off = al(((size_t)count + 1) * 8), o_head = o_off + al(((size_t)count + 1) * 8);
    const size_t o_cdoc = o_head + al((size_t)count * 4), o_rec = o_cdoc + al(nchunk * 4);
    rc = grow_dev(&S.d_meta, &S.meta_cap, o_rec + al(((size_t)count + 1) * sizeof(DecDocRec)));
    if (rc) return rc;
    u8* M = (u8*)S.d_meta;
    u64* d_base = (u64*)(M + o_base);
    const u64* d_off = off;
    u32* d_head = (u32*)(M + o_head);
    u32* d_cdoc = (u32*)(M + o_cdoc);
    DecDocRec* d_rec = (DecDocRec*)(M + o_rec);
    const u8* d_src = in;
    TRYH(hipMemcpyAsync(d_base, base.data(), base.size() * 8, hipMemcpyHostToDevice, st));
    std::vector<u64> offr;
    if (!dev) {                                  // one upload of the packed documents, offsets relative to the first
        rc = grow_dev((void**)&S.d_raw, &S.raw_cap, (size_t)in_len + 256);
        if (rc) return rc;
        if (in_len) TRYH(hipMemcpyAsync(S.d_raw, in + in_first, (size_t)in_len, hipMemcpyHostToDevice, st));
        offr.resize(offh.size());
        for (size_t d = 0; d < offh.size(); d++) offr[d] = offh[d] - in_first;
        TRYH(hipMemcpyAsync(M + o_off, offr.data(), offr.size() * 8, hipMemcpyHostToDevice, st));
        d_off = (const u64*)(M + o_off);
        d_src = S.d_raw;
    }
    rc = grow_dev((void**)&S.d_in, &S.in_cap, (size_t)staged + 1024, 1, false);
    if (rc) return rc;
    TRYH(hipMemsetAsync(S.d_in + staged, 0, 1024, st));
    rc = grow_dev((void**)&S.d_dcand, &S.dcand_cap, (size_t)std::min<u64>(staged / 4 + 16, 1u << 27), sizeof(DecCand), false);
    if (rc) return rc;
    S.D.in32 = (const u32*)S.d_in;
    S.D.zeroChunk = (staged >> 8) + 1;              // inside the 1024 zero bytes behind the last document
    rc = k7_stage(d_src, d_off, d_base, count, staged, S.d_in, d_cdoc, d_head, st);
    if (rc) return rc;
    rc = k7_scan_batch(S.d_in, staged, d_off, d_base, d_cdoc, S.d_dcand, S.d_ncand, (u32)S.dcand_cap, st);
    if (rc) return rc;
    std::vector<u32> head(count);
    u32 nc = 0;
    TRYH(hipMemcpyAsync(&nc, S.d_ncand, 4, hipMemcpyDeviceToHost, st));
    if (count) TRYH(hipMemcpyAsync(head.data(), d_head, (size_t)count * 4, hipMemcpyDeviceToHost, st));
    TRYH(dec_sync(st));
    if (nc > S.dcand_cap) return CJS_E_UNSUPPORTED;
    std::vector<DecCand> cand(nc);
    if (nc) {
        TRYH(hipMemcpyAsync(cand.data(), S.d_dcand, (size_t)nc * sizeof(DecCand), hipMemcpyDeviceToHost, st));
        TRYH(dec_sync(st));
    }
    std::sort(cand.begin(), cand.end(), [](const DecCand& x, const DecCand& y) { return x.key < y.key; });
    Slots w;
    for (const DecCand& x : cand) if (!(x.key & 1u)) { w.bpos.push_back(x.key >> 1); w.blim.push_back(x.a); }
    rc = dec_fit_slots(S, slots, w.bpos.size());
    if (rc) return rc;
    S.D.candLim = S.d_blim;

    std::vector<DocOut> R(count, DocOut{0, 0, 0, 0, 0, 0, false});
    std::vector<ValidBlk> valid;
    std::vector<u32> vdoc;         // the document of valid[k]
    u32 d = 0;
    bool fresh = true;             // document d has not been started
    Chain c = {0, 0, 0};
    for (;;) {
        u32 need = 0;
        while (d < count) {
            if (R[d].status) { d++; fresh = true; continue; }                    // a block CRC of an earlier slot batch has failed it
            BatchSrc src = {cand, base[d] * 8, offh[d + 1] - offh[d], nullptr};
            int term = 0;
            if (fresh) {
                c = {32, 0, 0};
                term = check_header(S, src.len >= 4, head[d], &c.dbufSize);      // :137-152, before anything else
                fresh = false;
            }
            if (!term) term = walk_chain(S, src, c, multistream, true, w, valid, &need);
            vdoc.resize(valid.size(), d);
            if (term > 0) break;                         // document d waits for the slot batch from `need` on
            if (term) doc_fail(S, R[d], term);           // (a block CRC found by append_docs in front of it still wins)
            d++; fresh = true;
        }
        rc = append_docs(S, st, valid, vdoc, R);
        if (rc) return rc;
        if (d == count) break;
        if (R[d].status) continue;                       // the document waiting for blocks has failed meanwhile: no batch for it
        rc = decode_from(S, st, w, need);
        if (rc) return rc;
    }
    S.detail = 0; S.crc_got = S.crc_want = 0;            // (cjs_bz2_last_detail is the single call's; a batch reports per document)
    return docs_deliver(S, st, R, d_rec, dev, out_off, status, detail);
}

// ---------------------------------------------------------------------------------------------
// A list of blocks of one stream (cjs_bz2_decompress_blocks): request k decodes as Bunzip.decodeBlock (lib/Bzip2.js:482-503) does at
// bitpos[k] alone.  The stream is staged once; k7_blocks.hip classifies the requests and compacts the block requests into the
// candidate list on the device, so neither form reads 48 bits per request through the host; the block requests then go through
// shared slot batches (k7_decode, the reference's block checks, K8/K9, CRC) and the outcome records of a batch of documents.
// Waits: one for the probe, then one k7 and two K8/K9 waits per slot batch.
// ---------------------------------------------------------------------------------------------
int64_t dec_blocks(DecState** ps, u32 slots, hipStream_t st, const u8* in, u64 len, const u64* bitpos, u32 count, bool dev,
                   u64* out_off, int* status, u32* detail) {
    int rc = dec_begin(ps, slots);
    if (rc) return rc;
    DecState& S = **ps;
    if (count > (1u << 27)) return CJS_E_UNSUPPORTED;                            // the cap on candidates
    rc = stage_input(S, in, len, dev, st);                                       // (candLim = null: a single stream)
    if (rc) return rc;
    // device side: positions (host form) | classes | workgroup totals | candidates | request of candidate | head | outcome records
    const size_t nwg = ((size_t)count + 255) / 256;
    const size_t o_pos = 0, o_cls = al((size_t)count * 8), o_wg = o_cls + al(count), o_cand = o_wg + al(nwg * 4);
    const size_t o_req = o_cand + al((size_t)count * 8), o_head = o_req + al((size_t)count * 4), o_rec = o_head + al(8);
    rc = grow_dev(&S.d_meta, &S.meta_cap, o_rec + al(((size_t)count + 1) * sizeof(DecDocRec)));
    if (rc) return rc;
    u8* M = (u8*)S.d_meta;
    const u64* d_pos = bitpos;
    if (!dev) {
        TRYH(hipMemcpyAsync(M + o_pos, bitpos, (size_t)count * 8, hipMemcpyHostToDevice, st));
        d_pos = (const u64*)(M + o_pos);
    }
    u64* d_cand = (u64*)(M + o_cand);
    rc = k7_blocks(S.D.in32, len, d_pos, count, M + o_cls, (u32*)(M + o_wg), d_cand, (u32*)(M + o_req), (u32*)(M + o_head), st);
    if (rc) return rc;
    u32 head[2] = {0, 0};
    std::vector<u8> cls(count);
    std::vector<u32> reqOf(count);
    TRYH(hipMemcpyAsync(head, M + o_head, 8, hipMemcpyDeviceToHost, st));
    TRYH(hipMemcpyAsync(cls.data(), M + o_cls, count, hipMemcpyDeviceToHost, st));
    TRYH(hipMemcpyAsync(reqOf.data(), M + o_req, (size_t)count * 4, hipMemcpyDeviceToHost, st));
    TRYH(dec_sync(st));
    const u32 nblk = std::min(head[0], count);

    std::vector<DocOut> R(count, DocOut{0, 0, 0, 0, 0, 0, false});
    u32 dbufSize = 0;
    const int hrc = check_header(S, len >= 4, head[1], &dbufSize);               // :137-152 (new Bunzip), before anything else
    if (hrc) for (DocOut& o : R) doc_fail(S, o, hrc);
    else for (u32 k = 0; k < count; k++) if (cls[k] == DEC_REQ_NEITHER) doc_fail(S, R[k], fail(S, DEC_NOT_BZIP, DEC_DETAIL_NONE));   // :160-161
    if (!hrc && nblk) {
        rc = dec_fit_slots(S, slots, nblk);
        if (rc) return rc;
        struct CandOf {                                  // k7_decode reads the compacted list; every other caller its own upload
            DecState& S;
            ~CandOf() { S.D.cand = S.d_bcand; }
        } restore = {S};
        S.D.cand = d_cand;
        S.D.candLim = nullptr;
        std::vector<DecResult> res;
        std::vector<ValidBlk> valid;
        std::vector<u32> size, crc;
        std::vector<u64> outOff;
        for (u32 first = 0; first < nblk; first += S.slots) {
            const u32 n = std::min(S.slots, nblk - first);
            rc = k7_run(S.D, first, n, st);
            if (rc) return rc;
            res.resize(n);
            TRYH(hipMemcpyAsync(res.data(), S.D.res, (size_t)n * sizeof(DecResult), hipMemcpyDeviceToHost, st));
            TRYH(dec_sync(st));
            valid.clear();
            for (u32 i = 0; i < n; i++) {
                const int e = block_error(S, res[i], dbufSize);
                if (e) doc_fail(S, R[reqOf[first + i]], e);
                else valid.push_back({i, res[i].crc, 0});
            }
            rc = run_k8k9(S, st, valid, size, crc, outOff);
            if (rc) return rc;
            for (size_t v = 0; v < valid.size(); v++) {
                DocOut& o = R[reqOf[first + valid[v].slot]];
                o.src = outOff[v]; o.size = size[v];
                S.out_size += size[v];
                if (crc[v] != valid[v].crc) { o.status = DEC_DATA_ERROR; o.detail = DEC_DETAIL_BLOCK_CRC; o.got = crc[v]; o.want = valid[v].crc; }
            }
        }
    }
    S.detail = 0; S.crc_got = S.crc_want = 0;            // (cjs_bz2_last_detail is the single call's; a list reports per request)
    return docs_deliver(S, st, R, (DecDocRec*)(M + o_rec), dev, out_off, status, detail);
}

const u8* dec_output(DecState* S, u64* size) { *size = S ? S->out_size : 0; return S ? S->d_out : nullptr; }
void dec_error_info(DecState* S, int* detail, u32* got, u32* want) {
    *detail = S ? S->detail : 0; *got = S ? S->crc_got : 0; *want = S ? S->crc_want : 0;
}
u32 dec_table(DecState* S, const u64** pos, const u64** size) {
    if (!S) return 0;
    *pos = S->tab_pos.data(); *size = S->tab_size.data();
    return (u32)S->tab_pos.size();
}
