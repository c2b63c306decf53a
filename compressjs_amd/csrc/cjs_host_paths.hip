// cjs_bz2_compress on host buffers that do not go through the GPU in one piece: the segmented path (inputs of more than a
// batch and a half) and the overlapped path (CJS_SLICE_BLOCKS, off by default).  Both are reached from cjs_abi.hip only.
#include "cjs_ctx.h"
#include "cjs_chain.h"
#include <atomic>
#include <chrono>
#include <stdlib.h>

namespace cjs {
// Host buffers in, host buffers out, input longer than ~1.5 batches: the input is cut into SEGMENTS of about one batch
// of blocks.  A segment is planned as an input of its own (a bzip2 block always starts with a fresh RLE1 state,
// lib/Bzip2.js:636-667, so planning from a block start is exact); all of its blocks but the last are encoded, and
// the next segment starts where that last, possibly incomplete, block started.  Two helper threads move data on
// their own non-blocking streams: the uploader keeps H2D a segment ahead of the encoder, the downloader copies the
// bytes of the stream that are final (everything before the bit cursor) while the next segment is being encoded.
namespace {
struct SegCopy {
    std::mutex mu;
    std::condition_variable cv;
    uint64_t uploaded = 0;          // input bytes resident in HBM
    uint64_t want = 0;              // downloader: copy the stream up to this byte
    bool quit = false;
    int err = 0;
};
// The uploader of both paths: src into dst in order, `chunk` bytes at a time on a copy stream, every chunk waited for.
// progress(bytes resident) publishes how far it got and says whether to go on.
template <class Progress>
int upload_chunked(u8* dst, const u8* src, uint64_t len, uint64_t chunk, hipStream_t st, Progress progress) {
    for (uint64_t off = 0; off < len; off += chunk) {
        const uint64_t n = len - off < chunk ? len - off : chunk;
        HIP_CHECK_RET(hipMemcpyAsync(dst + off, src + off, n, hipMemcpyHostToDevice, st));
        HIP_CHECK_RET(hipStreamSynchronize(st));
        if (!progress(off + n)) break;
    }
    return CJS_OK;
}
}

int64_t compress_segmented(cjs_ctx* c, const uint8_t* in, uint64_t in_len, int level, uint8_t* out, uint64_t out_cap,
                           uint64_t seg_bytes) {
    hipError_t e;
#define TRYR(x) if ((e = (x)) != hipSuccess) { rc = CJS_E_HIP - (int)e; goto done; }
    const u32 cap = block_cap(level);
    int64_t rc = 0;
    SegCopy sc;
    hipStream_t sIn = nullptr, sOut = nullptr;
    std::thread up, down;
    uint64_t copied = 0;            // bytes of the stream already in `out` (downloader's own)
    const int dev = c->device;
    u8* din = (u8*)c->din;
    u8* dout = (u8*)c->dout;
    const uint64_t dout_cap = c->dout_bytes;
    float total_ms = 0.f;
    u32 total_blocks = 0;
    Pipe P0 = stream_pipe(c, dout, dout_cap);
    if (hipStreamCreateWithFlags(&sIn, hipStreamNonBlocking) != hipSuccess || hipStreamCreateWithFlags(&sOut, hipStreamNonBlocking) != hipSuccess) {
        if (sIn) (void)hipStreamDestroy(sIn);
        return CJS_E_HIP;
    }
    up = std::thread([&]() {
        int rcu = hipSetDevice(dev) == hipSuccess ? CJS_OK : CJS_E_NOGPU;
        if (!rcu) rcu = upload_chunked(din, in, in_len, (uint64_t)32 << 20, sIn, [&](uint64_t resident) {
            std::lock_guard<std::mutex> g(sc.mu);
            sc.uploaded = resident;
            sc.cv.notify_all();
            return !sc.quit;
        });
        if (rcu) { std::lock_guard<std::mutex> g(sc.mu); sc.err = rcu; sc.cv.notify_all(); }
    });
    down = std::thread([&]() {
        if (hipSetDevice(dev) != hipSuccess) return;
        for (;;) {
            uint64_t to;
            {
                std::unique_lock<std::mutex> g(sc.mu);
                sc.cv.wait(g, [&]() { return sc.quit || sc.want > copied; });
                if (sc.want <= copied) return;          // quit and nothing left
                to = sc.want;
            }
            if (to > out_cap) { std::lock_guard<std::mutex> g(sc.mu); sc.err = CJS_E_NOSPACE; return; }
            hipError_t e2 = hipMemcpyAsync(out + copied, dout + copied, to - copied, hipMemcpyDeviceToHost, sOut);
            if (e2 == hipSuccess) e2 = hipStreamSynchronize(sOut);
            if (e2 != hipSuccess) { std::lock_guard<std::mutex> g(sc.mu); sc.err = CJS_E_HIP - (int)e2; return; }
            copied = to;
        }
    });
    {
        hipStream_t st = c->stream;
        int rci = k5_stream_begin(P0, level, st);
        if (rci) { rc = rci; goto done; }
        uint64_t s = 0;
        u32 seg = 0;
        while (s < in_len || (in_len == 0 && seg == 0)) {
            uint64_t eoff = s + seg_bytes < in_len ? s + seg_bytes : in_len;
            {   // wait until the uploader has brought the segment in
                std::unique_lock<std::mutex> g(sc.mu);
                sc.cv.wait(g, [&]() { return sc.err || sc.uploaded >= eoff; });
                if (sc.err) { rc = sc.err; goto done; }
            }
            void** kws = seg & 1 ? &c->planws : &c->k0ws;            // alternate: the previous segment's tables may still be read
            size_t* kwb = seg & 1 ? &c->planws_bytes : &c->k0ws_bytes;
            if (seg & 1) invalidate_plan(c);
            rci = grow(kws, kwb, k0_bytes(eoff - s, cap));
            if (rci) { rc = rci; goto done; }
            K0Buf K;
            k0_carve(K, din + s, eoff - s, cap, *kws);
            TRYR(hipEventRecord(c->ev0, st));
            rci = k0_prepass(K, cap, st);
            if (rci) { rc = rci; goto done; }
            TRYR(hipEventRecord(c->evReady, st));
            u32 nblocks = 0;
            TRYR(hipMemcpyAsync(&nblocks, K.nBlocks, 4, hipMemcpyDeviceToHost, st));
            TRYR(hipStreamSynchronize(st));
            u32 keep = nblocks;
            uint64_t next = in_len;
            if (eoff < in_len) {
                if (nblocks < 2) { seg_bytes *= 2; continue; }       // run-heavy input: one block swallowed the segment
                keep = nblocks - 1;
                uint64_t bs = 0;
                TRYR(hipMemcpy(&bs, K.blkStart + keep, 8, hipMemcpyDeviceToHost));
                next = s + bs;
            }
            rci = issue_blocks(c, K, cap, 0, keep, dout, dout_cap);
            if (rci) { rc = rci; goto done; }
            TRYR(hipEventRecord(c->ev1, st));
            const int64_t bits = stream_bits(c, st);
            if (bits < 0 && bits != CJS_E_NOSPACE) { rc = bits; goto done; }
            float ms = 0.f;
            TRYR(hipEventElapsedTime(&ms, c->ev0, c->ev1));
            total_ms += ms;
            total_blocks += keep;
            if (bits < 0) { rc = bits; goto done; }
            {   // everything before the bit cursor is final
                std::lock_guard<std::mutex> g(sc.mu);
                if (sc.err) { rc = sc.err; goto done; }
                sc.want = (uint64_t)bits >> 3;
                sc.cv.notify_all();
            }
            s = next;
            seg++;
            if (in_len == 0) break;
        }
        rci = k5_stream_end(P0, st);
        if (rci) { rc = rci; goto done; }
        rc = stream_bits(c, st);
        if (rc < 0) goto done;
        rc = (rc + 7) >> 3;
        if ((uint64_t)rc > out_cap) { rc = CJS_E_NOSPACE; goto done; }
        {
            std::lock_guard<std::mutex> g(sc.mu);
            sc.want = (uint64_t)rc;
            sc.cv.notify_all();
        }
    }
done:
    {
        std::lock_guard<std::mutex> g(sc.mu);
        sc.quit = true;
        sc.cv.notify_all();
    }
    if (up.joinable()) up.join();
    if (down.joinable()) down.join();
    (void)hipStreamDestroy(sIn);
    (void)hipStreamDestroy(sOut);
    if (rc >= 0 && sc.err) rc = sc.err;
    c->last_ms = total_ms;
    c->last_blocks = total_blocks;
    return rc;
#undef TRYR
}

// ---- host buffers in, host buffers out, ONE call, copies under the kernels (round 5) ----------------------------------------------
// lib/Bzip2.js:879-929 + lib/Util.js:9-103 define the product as host Buffer -> host Buffer.  Until round 4 a call that fits a batch and a
// half was upload-everything, encode, download-everything: 2.6 ms of PCIe around an 8.4 ms step (0.78 of the device-resident rate), and
// cutting it into the segments of compress_segmented cost more than their overlap saved (every segment a pre-pass, three read-backs and a
// drained GPU of its own).  Here the input is cut into SLICES of a few dozen blocks that flow through the context's streams without a gap:
//   uploader    (thread, own stream) brings the input in, in order, 8 MB at a time;
//   planner     (the caller's thread) - as soon as a slice and the margin behind it are resident: K0's tile scans over that window, the
//               slice's RLE1 cost, and from the cost prefix of the stream so far (plan_base: the arithmetic of the multi-device plan) the
//               phase of the block boundaries inside it: the blocks that START in the slice (k0_phase_plan); no chain through earlier plans;
//   encoders    (one thread per stream) run slice after slice as ONE sub-batch each, alternating streams; the only dependency between
//               slices is the bit cursor (k5_blockscan of slice j waits for that of slice j - 1: an event), as between sub-batches before;
//   downloader  (thread, own stream) copies every byte in front of the cursor a finished slice left (k5_blockscan drops it into pinned
//               memory) while later slices are encoded.
// A slice that cannot be planned on its own (a boundary inside a run that straddles a cut, a block longer than the margin) sends the
// call down the one-piece path.  Same bytes as cjs_bz2_compress_device on the whole input (tests/test_gpu_parity.py).
namespace {
struct OvSlice {
    uint64_t lo = 0, e = 0, wend = 0;   // bytes [lo, e), window end (margin included)
    K0Buf K;
    u32 nblocks = 0;
    hipEvent_t evScan = nullptr, evDone = nullptr;
    float t_up = 0, t_plan = 0, t_iss0 = 0, t_iss1 = 0, t_done = 0, t_copied = 0;   // CJS_OV_TRACE: ms since the call began
};
}
#ifndef CJS_CPU_DEBUG_BUILD
int64_t compress_overlapped(cjs_ctx* c, const uint8_t* in, uint64_t in_len, int level, uint8_t* out, uint64_t out_cap,
                            u32 slice_blocks) {
    const u32 cap = block_cap(level);
    const uint64_t W = plan_margin(cap);
    if (slice_blocks > c->sub_blocks) slice_blocks = c->sub_blocks;
    // the first slice is half a slice: the encoders start after 1/8 ... of the upload instead of 1/4
    std::vector<OvSlice> S;
    {
        const uint64_t sb = (uint64_t)slice_blocks * cap;
        uint64_t lo = 0, len = sb / 2 > W ? sb / 2 : sb;
        // CJS_SLICE_LIST="64,48": explicit slice lengths in blocks (experiments); the last one takes the rest
        std::vector<uint64_t> lens;
        if (const char* ev = getenv("CJS_SLICE_LIST"))
            for (const char* q = ev; *q;) { lens.push_back((uint64_t)strtoul(q, (char**)&q, 10) * cap); if (*q == ',') q++; }
        size_t li = 0;
        if (!lens.empty()) len = lens[li++];
        while (lo < in_len) {
            OvSlice sl;
            sl.lo = lo;
            sl.e = lo + len < in_len ? lo + len : in_len;
            if (lens.empty() && in_len - sl.e < sb / 4) sl.e = in_len;          // no stub at the end
            sl.wend = sl.e + W < in_len ? sl.e + W : in_len;
            S.push_back(sl);
            lo = sl.e;
            len = lens.empty() ? sb : (li < lens.size() ? lens[li++] : in_len);
        }
    }
    const u32 ns = (u32)S.size();
    if (ns < 2 || ns > CJS_SNAP_SLOTS) return CJS_OV_NOT_STARTED;      // (nothing uploaded: the caller must not take the input for resident - ADVICE r5)
    if (!c->sIn) HIP_CHECK_RET(hipStreamCreateWithFlags(&c->sIn, hipStreamNonBlocking));
    if (!c->sOut) HIP_CHECK_RET(hipStreamCreateWithFlags(&c->sOut, hipStreamNonBlocking));
    if (!c->snapPin) HIP_CHECK_RET(hipHostMalloc((void**)&c->snapPin, CJS_SNAP_SLOTS * 8));
    while (c->evPool.size() < 2u * ns) {
        hipEvent_t ev;
        HIP_CHECK_RET(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
        c->evPool.push_back(ev);
    }
    size_t k0each = 0;
    for (u32 k = 0; k < ns; k++) { const size_t b = (k0_bytes(S[k].wend - S[k].lo, cap) + 255) & ~(size_t)255; k0each = b > k0each ? b : k0each; }
    int rc = grow(&c->k0sl, &c->k0sl_bytes, k0each * ns);
    if (rc) return rc;
    invalidate_plan(c);
    u8* din = (u8*)c->din;
    u8* dout = (u8*)c->dout;
    const uint64_t dout_cap = c->dout_bytes;
    const int dev = c->device;
    const u32 nst = c->nstreams;
    const auto t_begin = std::chrono::steady_clock::now();
    auto now_ms = [&]() { return std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t_begin).count(); };
    static const bool ov_trace = getenv("CJS_OV_TRACE") != nullptr;

    std::mutex mu;
    std::condition_variable cv;
    uint64_t uploaded = 0;
    u32 planned = 0;                    // slices whose plan is ready
    u32 issued = 0;                     // slices whose launches are all enqueued (evDone recorded)
    bool stop = false;                  // error or fall-back: everybody winds down
    int err = 0;
    auto fail = [&](int code) { std::lock_guard<std::mutex> g(mu); if (!err) err = code; stop = true; cv.notify_all(); };

    // ---- uploader
    c->io[0].post([&]() {
        int rcu = hipSetDevice(dev) == hipSuccess ? CJS_OK : CJS_E_NOGPU;
        if (!rcu) rcu = upload_chunked(din, in, in_len, (uint64_t)8 << 20, c->sIn, [&](uint64_t resident) {
            std::lock_guard<std::mutex> g(mu);
            uploaded = resident;
            cv.notify_all();
            return !err;                                   // (not `stop`: a fall-back still wants the whole input resident)
        });
        if (rcu) fail(rcu);
    });
    // ---- downloader: the bytes in front of the cursor of every finished slice
    uint64_t copied = 0;
    int64_t result = -1;
    c->io[1].post([&]() {
        if (hipSetDevice(dev) != hipSuccess) { fail(CJS_E_NOGPU); return; }
        for (u32 k = 0; k < ns; k++) {
            {
                std::unique_lock<std::mutex> g(mu);
                cv.wait(g, [&]() { return stop || issued > k; });
                if (stop) return;
            }
            hipError_t e2 = hipEventSynchronize(S[k].evDone);
            if (e2 != hipSuccess) { fail(CJS_E_HIP - (int)e2); return; }
            S[k].t_done = now_ms();
            const uint64_t to = c->snapPin[k] >> 3;
            if (to > out_cap) { fail(CJS_E_NOSPACE); return; }
            if (to > copied) {
                e2 = hipMemcpyAsync(out + copied, dout + copied, to - copied, hipMemcpyDeviceToHost, c->sOut);
                if (e2 == hipSuccess) e2 = hipStreamSynchronize(c->sOut);
                if (e2 != hipSuccess) { fail(CJS_E_HIP - (int)e2); return; }
                copied = to;
            }
            S[k].t_copied = now_ms();
        }
    });
    // ---- encoders: stream si takes slices si, si + nst, ...; the cursor events are recorded and waited for in slice order
    std::atomic<u32> recorded(0);
    const BatchGeom g = make_geom(c->sub_blocks, cap);
    auto encoder = [&](u32 si) {
        if (hipSetDevice(dev) != hipSuccess) { fail(CJS_E_NOGPU); return; }
        for (u32 k = si; k < ns; k += nst) {
            {
                std::unique_lock<std::mutex> gq(mu);
                cv.wait(gq, [&]() { return stop || planned > k; });
                if (stop) return;
            }
            OvSlice& sl = S[k];
            int r2 = CJS_OK;
            Pipe P;
            sl.t_iss0 = now_ms();
            if (sl.nblocks) {
                if (k < nst) r2 = hipStreamWaitEvent(c->sub[si], c->evReady, 0) == hipSuccess ? CJS_OK : CJS_E_HIP;
                if (!r2) r2 = run_sub_batch(c, sl.K, g, cap, 0, sl.nblocks, si, dout, dout_cap, P, sl.nblocks);
            }
            while (recorded.load(std::memory_order_acquire) != k) {
                std::this_thread::yield();
                std::lock_guard<std::mutex> gq(mu);
                if (stop) return;
            }
            if (!r2) {
                if (sl.nblocks) {
                    P.snap = c->snapPin + k;
                    r2 = k5_run(P, cap, c->sub[si], k ? S[k - 1].evScan : nullptr, sl.evScan, c->side ? c->evCrc[si] : nullptr);
                } else {
                    // (a slice in which no block starts: the cursor stays where it is)
                    // (the cursor is carried IN STREAM ORDER behind the previous slice's k5_blockscan: read on the host at issue time, slot k - 1
                    // may not have been written yet, and the downloader would take stale bytes for final - ADVICE r5)
                    if (k && hipStreamWaitEvent(c->sub[si], S[k - 1].evScan, 0) != hipSuccess) r2 = CJS_E_HIP;
                    if (!k) c->snapPin[0] = 32u;
                    else if (!r2 && hipMemcpyAsync(c->snapPin + k, c->snapPin + k - 1, 8, hipMemcpyHostToHost, c->sub[si]) != hipSuccess) r2 = CJS_E_HIP;
                    if (!r2 && hipEventRecord(sl.evScan, c->sub[si]) != hipSuccess) r2 = CJS_E_HIP;
                }
            }
            if (!r2 && hipEventRecord(sl.evDone, c->sub[si]) != hipSuccess) r2 = CJS_E_HIP;
            sl.t_iss1 = now_ms();
            recorded.store(k + 1, std::memory_order_release);
            if (r2) { fail(r2); return; }
            std::lock_guard<std::mutex> gq(mu);
            if (k + 1 > issued) issued = k + 1;             // (slices finish issuing in any order; the downloader walks them in order and waits per slice)
            cv.notify_all();
        }
    };
    // (issued > k implies that slice k's evDone is recorded: a later slice only gets past `recorded` behind it)
    c->io[2].post([&]() { encoder(0); });
    for (u32 i = 1; i < nst; i++) c->helper[i].post([&, i]() { encoder(i); });

    // ---- planner (this thread)
    hipStream_t st = c->stream;
    bool fallback = false;
    Pipe P0 = stream_pipe(c, dout, dout_cap);
    {
        rc = k5_stream_begin(P0, level, st, true);
        if (!rc && hipEventRecord(c->evReady, st) != hipSuccess) rc = CJS_E_HIP;
        if (rc) fail(rc);
        PlanChain pc;
        uint64_t tau = 0;                                   // stream-wide target of the next block boundary (round 6: carried from slice to slice)
        for (u32 k = 0; k < ns && !rc; k++) {
            OvSlice& sl = S[k];
            sl.evScan = c->evPool[2 * k];
            sl.evDone = c->evPool[2 * k + 1];
            {
                std::unique_lock<std::mutex> gq(mu);
                cv.wait(gq, [&]() { return stop || uploaded >= sl.wend; });
                if (stop) break;
            }
            sl.t_up = now_ms();
            const uint64_t wlen = sl.wend - sl.lo, own = sl.e - sl.lo;
            k0_carve(sl.K, din + sl.lo, wlen, cap, (char*)c->k0sl + (size_t)k * k0each);
            rc = k0_scans(sl.K, st);
            if (!rc && own < wlen) rc = k0_eval(sl.K, own, st);
            if (rc) break;
            u64 tot[2] = {0, 0};                            // [0] cost of the window, [1] of the slice
            if (hipMemcpyAsync(&tot[0], sl.K.tileC + sl.K.ntiles, 8, hipMemcpyDeviceToHost, st) != hipSuccess) { rc = CJS_E_HIP; break; }
            if (own < wlen && hipMemcpyAsync(&tot[1], sl.K.specC, 8, hipMemcpyDeviceToHost, st) != hipSuccess) { rc = CJS_E_HIP; break; }
            if (hipStreamSynchronize(st) != hipSuccess) { rc = CJS_E_HIP; break; }
            MSeg ms;
            ms.lo = sl.lo; ms.e = sl.e;
            ms.cost = own < wlen ? tot[1] : tot[0];
            plan_base(pc, ms, edge_runs(in, sl.lo, sl.e), cap);
            if (!ms.ok || !seg_target(ms, tau)) { fallback = true; break; }
            rc = k0_phase_plan(sl.K, cap, ms.t0, own, sl.wend >= in_len ? 1u : 0u, tot[0], st);
            if (rc) break;
            u64 nbt[2] = {0, 0};                            // blocks, the target handed on (k0_phase_chain)
            if (hipMemcpyAsync(nbt, sl.K.nBlocks, 16, hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess) { rc = CJS_E_HIP; break; }
            const u32 nb = (u32)nbt[0];
            if (nb == K0_PHASE_FAIL || nb > c->sub_blocks) { fallback = true; break; }
            tau = ms.base + nbt[1];                         // the slices are planned in order: the chain needs no speculation here
            sl.nblocks = nb;
            sl.t_plan = now_ms();
            std::lock_guard<std::mutex> gq(mu);
            planned = k + 1;
            cv.notify_all();
        }
        if (rc) fail(rc);
        if (fallback) { std::lock_guard<std::mutex> gq(mu); stop = true; cv.notify_all(); }
    }
    // ---- wind down
    c->io[2].wait();
    for (u32 i = 1; i < nst; i++) c->helper[i].wait();
    c->io[1].wait();
    if (!stop) {
        // trailer behind the last slice, then the rest of the stream
        for (u32 i = 0; i < nst && i < ns; i++) if (hipStreamWaitEvent(st, S[ns - 1 - i].evDone, 0) != hipSuccess) rc = CJS_E_HIP;
        if (!rc) rc = k5_stream_end(P0, st);
        const int64_t bits = rc ? rc : stream_bits(c, st);
        if (bits < 0) rc = (int)bits;
        if (!rc) {
            const uint64_t total = ((uint64_t)bits + 7) >> 3;
            if (total > out_cap) rc = CJS_E_NOSPACE;
            else if (total > copied && hipMemcpy(out + copied, dout + copied, total - copied, hipMemcpyDeviceToHost) != hipSuccess) rc = CJS_E_HIP;
            result = (int64_t)total;
        }
        if (rc) fail(rc);
    }
    c->io[0].wait();                                       // (the uploader reads the caller's buffer: never leave it running)
    (void)hipDeviceSynchronize();
    u32 blocks = 0;
    for (u32 k = 0; k < ns; k++) blocks += S[k].nblocks;
    c->last_blocks = blocks;
    c->last_ms = now_ms();
    if (ov_trace) {
        fprintf(stderr, "[ov] %u slices, %.2f ms:", ns, c->last_ms);
        for (u32 k = 0; k < ns; k++) fprintf(stderr, " [%u: %u blk up %.2f plan %.2f issue %.2f-%.2f done %.2f copied %.2f]", k, S[k].nblocks, S[k].t_up, S[k].t_plan, S[k].t_iss0, S[k].t_iss1, S[k].t_done, S[k].t_copied);
        fprintf(stderr, "\n");
    }
    if (err) return err;
    if (fallback || stop) return CJS_E_SPEC;
    return result;
}
#endif
}
