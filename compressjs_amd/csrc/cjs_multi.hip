// C ABI of libcompressjs_amd.so: one stream over several contexts - cjs_bz2_compress_multi from one process, and the plan /
// encode entries that compressjs_amd/dist.py drives across processes.
#include "cjs_ctx.h"
#include "cjs_chain.h"
#include <atomic>
#include <chrono>
#include <stdlib.h>

using namespace cjs;

// ---- Bzip2.compressFile over several GPUs of one node, from ONE process (the Node addon's path to N devices) -----
// The input is cut at the nominal segment ends E_k = (k+1) * seg_bytes; segment k goes to device k mod n.  Round 4: the plan of
// a segment no longer waits for the plan of the segment before it (the reference's `do { readBlock } while`, lib/Bzip2.js:913-922,
// is serial; rounds 2-3 kept it serial across the segments).  Segments are taken in waves of n (one per device), and per wave:
//   A. every device uploads its window - the segment and the margin BEHIND it, [E_(k-1), E_k + W) - and scans it (K0's RLE1 cost
//      prefix, cjs_bz2_plan_scan): the segment's cost total; the host reads the segment's first and last run off the input;
//   B. from those summaries (the integer arithmetic of compressjs_amd/dist.py:plan_bases, restated in cjs_chain.h) every segment gets the
//      phase of the block boundaries inside it, plans the blocks that START in it (cjs_bz2_plan_phase) and encodes them from bit 0
//      into a buffer of its own, the margin completing the last one.
// When all bit lengths are known the segments are shifted on their devices to their bit offsets and copied side by side into the
// caller's buffer (parallel D2H, no peer traffic); the bytes two segments share are OR-ed on the host, which also folds the
// combined CRC (linear over GF(2)) and writes header and trailer.  A segment that cannot be planned on its own (a block boundary
// inside a run of four or more bytes that straddles a cut, a block longer than the margin, a boundary run beyond 4 KB) makes the
// call fall back to one device.  = SURVEY.md 8(e) without torch.distributed.
static std::atomic<int> g_multi_mallocs{0};        // hipMalloc calls of cjs_bz2_compress_multi's segment buffers (cjs_dbg_multi_mallocs: none after warm-up)
extern "C" int cjs_dbg_multi_mallocs(void) { return g_multi_mallocs.load(); }
static std::atomic<int> g_multi_replans{0};        // segments of cjs_bz2_compress_multi planned a second time (the chain carried a shift to them)
extern "C" int cjs_dbg_multi_replans(void) { return g_multi_replans.load(); }
static std::atomic<int> g_multi_fallbacks{0};      // calls of cjs_bz2_compress_multi that took the replicated plan (a segment that cannot be planned on its own)
extern "C" int cjs_dbg_multi_fallbacks(void) { return g_multi_fallbacks.load(); }

// Slot `slot` of the context's pool of segment buffers, at least `need` bytes: grow-only and kept across calls, allocated with a
// surplus of 1/8 so that a slightly longer segment of a later call still fits.
static int seg_buffer(cjs_ctx* c, size_t slot, uint64_t need, u8** buf) {
    if (c->segpool.size() <= slot) c->segpool.resize(slot + 1, std::pair<void*, size_t>(nullptr, 0));
    std::pair<void*, size_t>& pr = c->segpool[slot];
    if (pr.second < need) {
        if (hipSetDevice(c->device) != hipSuccess) return CJS_E_NOGPU;
        (void)hipFree(pr.first);
        pr = std::pair<void*, size_t>(nullptr, 0);
        void* pnew = nullptr;
        g_multi_mallocs++;
        if (hipMalloc(&pnew, need + (need >> 3)) != hipSuccess) return CJS_E_HIP - (int)hipErrorOutOfMemory;
        pr = std::pair<void*, size_t>(pnew, need + (need >> 3));
    }
    *buf = (u8*)pr.first;
    return CJS_OK;
}

extern "C" int64_t cjs_bz2_compress_multi(cjs_ctx** ctxs, uint32_t n, const uint8_t* in, uint64_t in_len, int level,
                                          uint8_t* out, uint64_t out_cap) {
    if (!ctxs || n == 0 || !ctxs[0] || (!in && in_len) || !out) return CJS_E_ARG;
    if (level < 1 || level > 9) return CJS_E_LEVEL;
    for (u32 i = 0; i < n; i++) if (!ctxs[i]) return CJS_E_ARG;
    const u32 cap = block_cap(level);
    const uint64_t seg_bytes = seg_bytes_for(ctxs[0], cap);
    uint64_t nseg = (in_len + seg_bytes - 1) / seg_bytes;
    if (n == 1 || nseg <= 1) return cjs_bz2_compress(ctxs[0], in, in_len, level, out, out_cap);
    const uint64_t W = plan_margin(cap);
    std::vector<MSeg> S(nseg);
    for (uint64_t k = 0; k < nseg; k++) {
        S[k].lo = k * seg_bytes;
        S[k].e = (k + 1) * seg_bytes < in_len ? (k + 1) * seg_bytes : in_len;
    }
    std::mutex mu;
    const auto t_begin = std::chrono::steady_clock::now();
    std::atomic<int> err{0};        // first error; 1 = take the replicated plan (the workers read it without the lock)
    auto fail = [&](int code) { std::lock_guard<std::mutex> g(mu); if (!err.load()) err.store(code); };
    // phase A of one segment on its context: window into HBM, cost scan
    auto scan_seg = [&](uint64_t k) {
        cjs_ctx* c = ctxs[k % n];
        MSeg& g = S[k];
        if (hipSetDevice(c->device) != hipSuccess) { fail(CJS_E_NOGPU); return; }
        const uint64_t we = g.e + W < in_len ? g.e + W : in_len, wlen = we - g.lo;
        int rc = grow(&c->din, &c->din_bytes, wlen + 64);
        if (rc) { fail(rc); return; }
        hipError_t e2 = hipMemcpyAsync(c->din, in + g.lo, wlen, hipMemcpyHostToDevice, c->stream);
        if (e2 != hipSuccess) { fail(CJS_E_HIP - (int)e2); return; }
        int64_t v = cjs_bz2_plan_scan(c, c->din, wlen, level);
        if (v >= 0) v = cjs_bz2_plan_cost(c, g.e - g.lo);
        if (v < 0) { (void)hipStreamSynchronize(c->stream); fail((int)v); return; }     // (the window's upload reads the caller's buffer: not left pending - ADVICE r4)
        g.cost = (uint64_t)v;
    };
    // phase B1: the blocks that START in the segment, planned from the target g.t0 (round 6: a link of the chain - cjs_bz2_plan_chain;
    // the segments of a wave plan at once from speculative targets, the calling thread validates the chain and plans a segment whose
    // target was wrong again)
    auto plan_seg = [&](uint64_t k) {
        cjs_ctx* c = ctxs[k % n];
        MSeg& g = S[k];
        if (hipSetDevice(c->device) != hipSuccess) { fail(CJS_E_NOGPU); return; }
        const uint64_t we = g.e + W < in_len ? g.e + W : in_len;
        uint64_t tn = g.t0;
        const int64_t nb = cjs_bz2_plan_chain(c, g.e - g.lo, g.t0, we >= in_len ? 1 : 0, &tn);
        if (nb == CJS_E_SPEC) { fail(1); return; }
        if (nb < 0) { fail((int)nb); return; }
        g.nb = nb; g.tnext = tn;
    };
    // phase B2: the segment's blocks of its context's plan, encoded from bit 0
    auto encode_seg = [&](uint64_t k) {
        cjs_ctx* c = ctxs[k % n];
        MSeg& g = S[k];
        if (g.nb == 0) return;
        if (hipSetDevice(c->device) != hipSuccess) { fail(CJS_E_NOGPU); return; }
        if (!g.dseg) { fail(CJS_E_HIP - (int)hipErrorOutOfMemory); return; }
        u32 fold = 0, cnt = 0;
        const int64_t bits = cjs_bz2_encode_blocks(c, g.first_blk, (u32)g.nb, g.dseg, g.dseg_cap, &fold, &cnt);
        if (bits < 0) { fail((int)bits); return; }
        g.bits = (uint64_t)bits; g.fold = fold; g.count = cnt;
    };
    // phase 2: shift to the bit offset, copy the inner bytes into place, fetch the two seam bytes
    auto place_seg = [&](uint64_t k) {
        cjs_ctx* c = ctxs[k % n];
        MSeg& g = S[k];
        if (!g.bits) return;
        if (hipSetDevice(c->device) != hipSuccess) { fail(CJS_E_NOGPU); return; }
        const uint64_t nbytes = (g.bits + 7) >> 3, sh = g.off & 7u;
        const uint64_t fb = g.off >> 3, lb = (g.off + g.bits - 1) >> 3, span = lb - fb + 1;
        int rc = grow(&c->dout, &c->dout_bytes, nbytes + 64);
        if (rc) { fail(rc); return; }
        rc = cjs_shift_bits(c, g.dseg, nbytes, (u32)sh, (u8*)c->dout);
        if (rc) { fail(rc); return; }
        hipError_t e2 = hipMemcpy(&g.first, c->dout, 1, hipMemcpyDeviceToHost);
        if (e2 == hipSuccess) e2 = hipMemcpy(&g.last, (u8*)c->dout + span - 1, 1, hipMemcpyDeviceToHost);
        if (e2 == hipSuccess && span > 2) e2 = hipMemcpy(out + fb + 1, (u8*)c->dout + 1, span - 2, hipMemcpyDeviceToHost);
        if (e2 != hipSuccess) fail(CJS_E_HIP - (int)e2);
    };
    // one PERSISTENT worker thread per device (the context's io[0] helper: created at its first job, kept until cjs_destroy) - until
    // round 5 a std::thread per device per phase per wave
    auto run_range = [&](uint64_t k0, uint64_t k1, const std::function<void(uint64_t)>& fn) {
#ifdef CJS_CPU_DEBUG_BUILD
        for (uint64_t k = k0; k < k1 && !err; k++) fn(k);             // the CPU logic-debug build runs kernels on one thread
#else
        const u32 nw = k1 - k0 < n ? (u32)(k1 - k0) : n;
        for (u32 d = 1; d < nw; d++) {
            cjs_ctx* c = ctxs[(k0 + d) % n];
            c->io[0].post([&, d]() { for (uint64_t k = k0 + d; k < k1 && !err; k += n) fn(k); });
        }
        for (uint64_t k = k0; k < k1 && !err; k += n) fn(k);          // (the calling thread takes the first device's share)
        for (u32 d = 1; d < nw; d++) ctxs[(k0 + d) % n]->io[0].wait();
#endif
    };
    auto run_all = [&](const std::function<void(uint64_t)>& fn) { run_range(0, nseg, fn); };
    {
        PlanChain pc;
        uint64_t tau = 0;                                             // stream-wide target of the next block boundary (the chain)
        int64_t shift = 0;                                            // what the boundaries in front of the wave have moved by so far (a guess for its later segments)
        for (uint64_t k0 = 0; k0 < nseg && !err; k0 += n) {           // a wave: one segment per device
            const uint64_t k1 = k0 + n < nseg ? k0 + n : nseg;
            run_range(k0, k1, scan_seg);
            if (err) break;
            for (uint64_t k = k0; k < k1; k++) {
                plan_base(pc, S[k], edge_runs(in, S[k].lo, S[k].e), cap);
                if (!S[k].ok) fail(1);
                const int64_t guess = (int64_t)S[k].phase + shift;
                S[k].t0 = (uint64_t)(guess < 0 ? guess + (int64_t)cap : guess);
            }
            if (!err && !seg_target(S[k0], tau)) fail(1);             // (the wave's first segment: its target is known)
            if (err) break;
            run_range(k0, k1, plan_seg);
            if (err) break;
            // the chain through the wave's segments: a segment planned from a wrong target (a boundary inside a run of four or more equal
            // bytes in a segment before it: ordinary text has them) is planned again, here and now - 0.1 ms, one job in some dozens
            for (uint64_t k = k0; k < k1 && !err; k++) {
                const uint64_t planned = S[k].t0;
                if (!seg_target(S[k], tau)) { fail(1); break; }
                if (S[k].t0 != planned) { g_multi_replans++; plan_seg(k); }
                if (err) break;
                shift = (int64_t)S[k].t0 - (int64_t)S[k].phase;
                tau = S[k].base + S[k].tnext;
            }
            if (err) break;
            // Every device's buffer for its segment of this wave, from the context's pool (grow-only, kept across calls: a hipMalloc per
            // segment and a hipFree - a device-wide sync - per segment in every call was what rounds 2-4 did).  Taken HERE, on the calling
            // thread and for every segment of the wave: inside the workers it depended on which of them saw another one's fallback flag
            // first, and a slot skipped in one call was a hipMalloc in the next (round 5: the test that counts them failed one run in eight).
            for (uint64_t k = k0; k < k1 && !err; k++) {
                S[k].dseg_cap = ((uint64_t)cjs_bz2_compress_bound(S[k].e - S[k].lo + W) + 3) & ~(uint64_t)3;
                const int rc = seg_buffer(ctxs[k % n], (size_t)(k / n), S[k].dseg_cap, &S[k].dseg);
                if (rc) fail(rc);
            }
            if (err) break;
            run_range(k0, k1, encode_seg);
        }
    }
    bool replicated = false;
    if (err == 1) {
        // A segment that cannot be planned on its own - a block longer than the margin, a run that fills a block or reaches beyond 4 KB at a
        // cut, a boundary inside a run that straddles a cut (round 5 also: any block boundary inside a run of four or more equal bytes - one
        // call in twenty-five at 7*10^7 bytes of text; round 6 carries those through the chain): the REPLICATED plan.  Every device takes
        // the whole input and plans it with the serial chain (cjs_bz2_plan: 0.5 ms per 10^8 bytes; the uploads run on the devices' own
        // links), then encodes its share of the blocks - what compressjs_amd/dist.py::sharded_compress does across processes.
        err.store(0);
        replicated = true;
        g_multi_fallbacks++;
        std::vector<int64_t> nbv(n, 0);
        run_range(0, n, [&](uint64_t d) {
            cjs_ctx* c = ctxs[d];
            if (hipSetDevice(c->device) != hipSuccess) { fail(CJS_E_NOGPU); return; }
            int rc = grow(&c->din, &c->din_bytes, in_len + 64);
            if (rc) { fail(rc); return; }
            hipError_t e2 = hipMemcpyAsync(c->din, in, in_len, hipMemcpyHostToDevice, c->stream);
            if (e2 != hipSuccess) { fail(CJS_E_HIP - (int)e2); return; }
            nbv[d] = cjs_bz2_plan(c, c->din, in_len, level);               // (synchronises the stream)
            if (nbv[d] < 0) { (void)hipStreamSynchronize(c->stream); fail((int)nbv[d]); }
        });
        for (u32 d = 1; d < n && !err; d++) if (nbv[d] != nbv[0]) fail(CJS_E_ARG);      // (cannot happen: the same bytes, the same plan)
        if (!err) {
            const uint64_t nb = (uint64_t)nbv[0];
            nseg = n;
            S.assign(nseg, MSeg());
            for (u32 d = 0; d < n && !err; d++) {
                MSeg& g = S[d];
                g.first_blk = (u32)(nb * d / n);
                g.nb = (int64_t)((u32)(nb * (d + 1) / n) - g.first_blk);
                if (!g.nb) continue;
                g.dseg_cap = ((uint64_t)cjs_bz2_compress_bound((uint64_t)g.nb * (cap + 19u)) + 3) & ~(uint64_t)3;
                const int rc = seg_buffer(ctxs[d], 0, g.dseg_cap, &g.dseg);
                if (rc) fail(rc);
            }
            if (!err) run_all(encode_seg);
        }
    }
    // the replicated plan needs the whole input and its K0 workspace on EVERY device: when that does not fit (a HIP / out-of-memory
    // error), the call degrades to one device's segmented path, whose device memory is bounded
    if (replicated && err.load() <= CJS_E_HIP) return cjs_bz2_compress(ctxs[0], in, in_len, level, out, out_cap);
    int64_t result = 0;
    if (!err) {
        uint64_t pos = 32;
        u32 crc = 0;
        for (uint64_t k = 0; k < nseg; k++) {
            S[k].off = pos;
            pos += S[k].bits;
            crc = rotl32(crc, S[k].count) ^ S[k].fold;                // lib/Bzip2.js:917 over the segment's blocks
        }
        const uint64_t end = pos + 80, total = (end + 7) >> 3;
        if (total > out_cap) err = CJS_E_NOSPACE;
        else {
            for (uint64_t k = 0; k < nseg; k++)
                if (S[k].bits) { out[S[k].off >> 3] = 0; out[(S[k].off + S[k].bits - 1) >> 3] = 0; }
            for (uint64_t b = pos >> 3; b < total; b++) out[b] = 0;
            run_all(place_seg);
            if (!err) {
                out[0] = 'B'; out[1] = 'Z'; out[2] = 'h'; out[3] = (u8)('0' + level);       // lib/Bzip2.js:903-906
                for (uint64_t k = 0; k < nseg; k++)
                    if (S[k].bits) { out[S[k].off >> 3] |= S[k].first; out[(S[k].off + S[k].bits - 1) >> 3] |= S[k].last; }
                // end-of-stream magic + combined CRC at bit `pos` (lib/Bzip2.js:925-926), zero-padded to a byte
                const u8 tr[10] = {0x17, 0x72, 0x45, 0x38, 0x50, 0x90, (u8)(crc >> 24), (u8)(crc >> 16), (u8)(crc >> 8), (u8)crc};
                const u32 sh = (u32)(pos & 7u);
                for (u32 i = 0; i < 10; i++) {
                    out[(pos >> 3) + i] |= (u8)(tr[i] >> sh);
                    if (sh) out[(pos >> 3) + i + 1] |= (u8)(tr[i] << (8u - sh));
                }
                result = (int64_t)total;
            }
        }
    }
    if (err) return err;
    u32 blocks = 0;
    for (uint64_t k = 0; k < nseg; k++) blocks += S[k].count;
    ctxs[0]->last_blocks = blocks;
    // (cjs_last_device_ms: this path has no single device interval; it reports the wall time of the call)
    ctxs[0]->last_ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t_begin).count();
    return result;
}

// ---- sharded encoding (multi-GPU): plan once, then encode a block range bit-aligned at 0 ----------
// cjs_bz2_plan runs the K0 pre-pass over the whole input (kept in the context) and returns the
// number of bzip2 blocks.  cjs_bz2_encode_blocks encodes blocks [first, first+count) into d_seg
// WITHOUT stream header/trailer, first block starting at bit 0; returns the number of bits and the
// partial combined-CRC fold  P = XOR_i rotl^(count-1-i)(crc_i)  so that the caller can chain
// S' = rotl^count(S) ^ P across shards (lib/Bzip2.js:917 is linear over GF(2)).
extern "C" int64_t cjs_bz2_plan(cjs_ctx* c, const void* d_in, uint64_t in_len, int level) {
    if (!c || (!d_in && in_len)) return CJS_E_ARG;
    if (level < 1 || level > 9) return CJS_E_LEVEL;
    HIP_CHECK_RET(hipSetDevice(c->device));
    const u32 cap = block_cap(level);
    invalidate_plan(c);                              // no valid plan while this one is being made; c->plan is re-carved: an earlier cjs_bz2_plan_scan's tables are gone
    int rc = grow(&c->planws, &c->planws_bytes, k0_bytes(in_len, cap));
    if (rc) return rc;
    k0_carve(c->plan, (const u8*)d_in, in_len, cap, c->planws);
    rc = k0_prepass(c->plan, cap, c->stream);
    if (rc) return rc;
    u32 nblocks = 0;
    HIP_CHECK_RET(hipMemcpyAsync(&nblocks, c->plan.nBlocks, 4, hipMemcpyDeviceToHost, c->stream));
    HIP_CHECK_RET(hipStreamSynchronize(c->stream));
    c->plan_blocks = nblocks;
    c->plan_level = level;
    return (int64_t)nblocks;
}

// ---- parallel plan of a slice (multi-GPU): see k0_rle1.hip "the blocks of a SLICE of a longer stream" and compressjs_amd/dist.py ----
// cjs_bz2_plan_scan: K0's tile scans over d_in (the rank's slice followed by the margin it holds of what comes after); returns
// the input's own RLE1 cost total.  cjs_bz2_plan_cost: that cost prefix at byte `pos`.  cjs_bz2_plan_phase: the blocks that
// START in [0, own_len), given that boundaries lie where the prefix reaches phase + m * cap; returns their number (they are
// then blocks 0 .. n-1 for cjs_bz2_encode_blocks), or CJS_E_SPEC when the slice cannot be planned on its own (a boundary
// inside a long run, a block longer than the margin): the caller falls back to the chained / replicated plan.
extern "C" int64_t cjs_bz2_plan_scan(cjs_ctx* c, const void* d_in, uint64_t in_len, int level) {
    if (!c || (!d_in && in_len)) return CJS_E_ARG;
    if (level < 1 || level > 9) return CJS_E_LEVEL;
    HIP_CHECK_RET(hipSetDevice(c->device));
    const u32 cap = block_cap(level);
    invalidate_plan(c);
    int rc = grow(&c->planws, &c->planws_bytes, k0_bytes(in_len, cap));
    if (rc) return rc;
    k0_carve(c->plan, (const u8*)d_in, in_len, cap, c->planws);
    uint64_t total = 0;
    if (in_len) {
        rc = k0_scans(c->plan, c->stream);
        if (rc) return rc;
        HIP_CHECK_RET(hipMemcpyAsync(&total, c->plan.tileC + c->plan.ntiles, 8, hipMemcpyDeviceToHost, c->stream));
        HIP_CHECK_RET(hipStreamSynchronize(c->stream));
    }
    c->scan_level = level;
    c->scan_total = total;
    return (int64_t)total;
}

extern "C" int64_t cjs_bz2_plan_cost(cjs_ctx* c, uint64_t pos) {
    if (!c || !c->scan_level) return CJS_E_ARG;
    if (pos >= c->plan.in_len) return (int64_t)c->scan_total;
    if (pos == 0) return 0;
    HIP_CHECK_RET(hipSetDevice(c->device));
    const int rc = k0_eval(c->plan, pos, c->stream);
    if (rc) return rc;
    uint64_t v = 0;
    HIP_CHECK_RET(hipMemcpyAsync(&v, c->plan.specC, 8, hipMemcpyDeviceToHost, c->stream));
    HIP_CHECK_RET(hipStreamSynchronize(c->stream));
    return (int64_t)v;
}

// Round 6: the slice's plan as a link of a CHAIN.  t0 = the value this input's own cost prefix reaches at the slice's first block boundary
// (the previous slice's *t_next after a change of origin; phase = (-G(lo)) mod cap when nothing in front of the slice moved a boundary).
// A block boundary inside a run of four or more equal bytes no longer refuses: the slice goes on serially from there (k0_phase_chain)
// and *t_next - the target of the first boundary at or beyond own_len - carries the shift to the slices behind it.  CJS_E_SPEC is left
// for what a slice cannot do on its own: a block longer than the margin, a run that fills a block.
extern "C" int64_t cjs_bz2_plan_chain(cjs_ctx* c, uint64_t own_len, uint64_t t0, int last, uint64_t* t_next) {
    if (!c || !c->scan_level || own_len > c->plan.in_len) return CJS_E_ARG;
    HIP_CHECK_RET(hipSetDevice(c->device));
    const u32 cap = block_cap(c->scan_level);
    c->plan_level = 0;
    c->plan_blocks = 0;
    if (t_next) *t_next = t0;
    if (c->plan.in_len == 0) { c->plan_level = c->scan_level; return 0; }
    const int rc = k0_phase_plan(c->plan, cap, t0, own_len, last ? 1u : 0u, c->scan_total, c->stream);
    if (rc) return rc;
    // (pinned: a pageable read-back costs tens of microseconds more; pin[0] is free here - no sub-batch is running on this context)
    HIP_CHECK_RET(hipMemcpyAsync(c->pin[0], c->plan.nBlocks, 16, hipMemcpyDeviceToHost, c->stream));
    HIP_CHECK_RET(hipStreamSynchronize(c->stream));
    const u32 nblocks = c->pin[0][0];
    uint64_t tn = 0;
    memcpy(&tn, c->pin[0] + 2, 8);
    if (nblocks == K0_PHASE_FAIL) return CJS_E_SPEC;
    if (t_next) *t_next = tn;
    c->plan_blocks = nblocks;
    c->plan_level = c->scan_level;
    return (int64_t)nblocks;
}

// The round-3 entry: boundaries where the prefix reaches phase + m * cap and NOTHING carried - a slice whose plan moves the
// boundaries behind it (a boundary inside a long run) is refused, as before, unless the stream ends in it.
extern "C" int64_t cjs_bz2_plan_phase(cjs_ctx* c, uint64_t own_len, uint64_t phase, int last) {
    if (!c || !c->scan_level) return CJS_E_ARG;
    const u32 cap = block_cap(c->scan_level);
    if (phase >= cap) return CJS_E_ARG;
    uint64_t tn = 0;
    const int64_t nb = cjs_bz2_plan_chain(c, own_len, phase, last, &tn);
    if (nb < 0) return nb;
    if (!last && tn >= phase && (tn - phase) % cap != 0) { c->plan_level = 0; c->plan_blocks = 0; return CJS_E_SPEC; }
    return nb;
}

// first input byte (relative to the planned input) of block k of the current plan; k == number of blocks: the input length
extern "C" int64_t cjs_bz2_plan_block_start(cjs_ctx* c, uint32_t k) {
    if (!c || !c->plan_level || k > c->plan_blocks) return CJS_E_ARG;
    if (k == c->plan_blocks) return (int64_t)c->plan.in_len;
    if (hipSetDevice(c->device) != hipSuccess) return CJS_E_NOGPU;
    uint64_t v = 0;
    const hipError_t e = hipMemcpy(&v, c->plan.blkStart + k, 8, hipMemcpyDeviceToHost);
    return e == hipSuccess ? (int64_t)v : CJS_E_HIP - (int)e;
}

extern "C" int64_t cjs_bz2_encode_blocks(cjs_ctx* c, uint32_t first, uint32_t count, void* d_seg,
                                         uint64_t seg_cap, uint32_t* crc_fold, uint32_t* n_done) {
    if (!c || !d_seg || !c->plan_level || ((uintptr_t)d_seg & 3) || seg_cap < 64) return CJS_E_ARG;
    if (first > c->plan_blocks) return CJS_E_ARG;
    if (count > c->plan_blocks - first) count = c->plan_blocks - first;   // no uint32 wrap for count = 0xFFFFFFFF ("all remaining")
    HIP_CHECK_RET(hipSetDevice(c->device));
    const u32 cap = block_cap(c->plan_level);
    hipStream_t st = c->stream;
    Pipe P0 = stream_pipe(c, d_seg, seg_cap);
    HIP_CHECK_RET(hipEventRecord(c->ev0, st));
    int rc = k5_stream_begin(P0, -1, st);                // level < 0: no "BZh" header, cursor at bit 0
    if (rc) return rc;
    HIP_CHECK_RET(hipEventRecord(c->evReady, st));
    rc = issue_blocks(c, c->plan, cap, first, count, d_seg, seg_cap);
    if (rc) return rc;
    HIP_CHECK_RET(hipEventRecord(c->ev1, st));
    u32 crc = 0;                                     // k5 folded from 0: exactly P
    const int64_t bits = stream_bits(c, st, nullptr, &crc);
    if (bits < 0 && bits != CJS_E_NOSPACE) return bits;
    HIP_CHECK_RET(hipEventElapsedTime(&c->last_ms, c->ev0, c->ev1));
    c->last_blocks = count;
    if (bits < 0) return bits;
    if (crc_fold) *crc_fold = crc;
    if (n_done) *n_done = count;
    return bits;
}
