// C ABI of libcompressjs_amd.so: BWTC.compressFile / BWTC.decompressFile - the block stages on the GPU, the adaptive range
// coder on the host (bwtc_host.hip).
#include "cjs_ctx.h"
#include "bwtc_host.h"
#include <chrono>
#include <stdlib.h>

using namespace cjs;

// ---------------------------------------------------------------------------------------------
// BWTC.compressFile(input, null, level), level 6..9 (lib/BWTC.js:12-139): BWT + MTF/RLE2 on the
// GPU per 100000*level-byte block, adaptive range coder on the host (serial by construction).
// Levels 1-5 use DefSumModel (lib/BWTC.js:107), levels 6-9 FenwickModel; both coders run on the host.
// ---------------------------------------------------------------------------------------------
extern "C" int64_t cjs_bwtc_compress_bound(uint64_t in_len) { return (int64_t)bwtc_bound(in_len); }

extern "C" int64_t cjs_bwtc_compress(cjs_ctx* c, const uint8_t* in, uint64_t in_len, int level, uint8_t* out,
                                     uint64_t out_cap, int64_t declared_size) {
    if (!c || (!in && in_len) || !out) return CJS_E_ARG;
    if (level < 1 || level > 9) level = 9;                         // lib/BWTC.js:16-19: bad props -> 9
    hipError_t e;
    HIP_CHECK_RET(hipSetDevice(c->device));
    const u32 bs = (u32)level * 100000u;
    int rc = grow(&c->din, &c->din_bytes, in_len + 64);
    if (rc) return rc;
    hipStream_t st = c->stream;
    if (in_len) HIP_CHECK_RET(hipMemcpyAsync(c->din, in, in_len, hipMemcpyHostToDevice, st));
    const u64 nblocks = (in_len + bs - 1) / bs;
    BatchGeom g = make_geom(c->sub_blocks, bs);
    bwtc_coder* coder = bwtc_begin(out, out_cap, declared_size, level);
    // levels 6..9: the adaptive FenwickModel of every block runs on the GPU too (K10, one wave per block: a serial
    // recurrence, ~170 ms per launch whatever the number of blocks), the host keeps the range coder.
    // CJS_BWTC_GPU_MODEL=0: model on the host as in round 1 (A/B runs).
    const bool gpu_model = []() { const char* ev = getenv("CJS_BWTC_GPU_MODEL"); return !ev || atoi(ev) != 0; }();          // (read per call)
    // rows of K10's triples: 2 x stride per block in the round lists of K1 (free in linear mode); CJS_K10_CAP (tests) shrinks them
    const u32 k10_ostride = 2u * make_geom(c->sub_blocks, (u32)level * 100000u).stride;
    const u32 k10_cap = []() -> u32 { const char* ev = getenv("CJS_K10_CAP"); return ev ? (u32)strtoul(ev, nullptr, 10) : 0xFFFFFFFFu; }() < k10_ostride
                            ? (u32)strtoul(getenv("CJS_K10_CAP"), nullptr, 10) : k10_ostride;
    const bool tri = gpu_model && level >= 6;
    // Sub-batches are processed in GROUPS of one per stream: their GPU stages are issued back to back on different
    // streams (the K10 launches of a group overlap), then everything the coder needs is copied to host vectors and
    // handed to the coder thread, which works through group g while the GPU runs group g + 1.
    typedef BwtcBlockJob BlockJob;
    typedef BwtcGroupJob GroupJob;
    for (int i = 0; i < 2; i++) c->bwtc_jobs[i].busy = false;
    std::mutex mu;
    std::condition_variable cv;
    std::vector<GroupJob*> queue;
    bool done_issuing = false;
    const bool btrace = getenv("CJS_BWTC_TRACE") != nullptr;
    const auto tb0 = std::chrono::steady_clock::now();
    auto msnow = [&]() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - tb0).count(); };
    double coder_busy = 0, coder_first = 0, ncalls_total = 0;
    std::thread coder_thread([&]() {
        for (;;) {
            GroupJob* job = nullptr;
            {
                std::unique_lock<std::mutex> lk(mu);
                cv.wait(lk, [&]() { return done_issuing || !queue.empty(); });
                if (queue.empty()) return;
                job = queue.front();
                queue.erase(queue.begin());
            }
            const double tj0 = msnow();
            if (coder_first == 0) coder_first = tj0;
            for (size_t bi = 0; bi < job->blocks.size(); bi++) {
                {   // the copies of a group land stream by stream: start on what is there
                    std::unique_lock<std::mutex> lk(mu);
                    cv.wait(lk, [&]() { return bi < job->nready || done_issuing; });
                    if (bi >= job->nready) return;                     // (error path: the issuer gave up)
                }
                const BlockJob& bj = job->blocks[bi];
                if (tri && !bj.host) bwtc_block_triples(coder, bj.len, bj.pidx, bj.used, job->a.data() + bj.off, job->t.data() + bj.off, bj.ntri);
                else bwtc_block(coder, bj.len, bj.pidx, bj.used, job->sym.data() + (tri ? bj.soff : bj.off), bj.nsym);
            }
            coder_busy += msnow() - tj0;
            { std::lock_guard<std::mutex> lk(mu); job->busy = false; cv.notify_all(); }
        }
    });
    auto stop_coder = [&]() {
        { std::lock_guard<std::mutex> lk(mu); done_issuing = true; cv.notify_all(); }
        if (coder_thread.joinable()) coder_thread.join();
    };
#define TRYR(x) if ((e = (x)) != hipSuccess) { stop_coder(); (void)bwtc_end(coder); return CJS_E_HIP - (int)e; }
    const u32 ns = c->nstreams;
    std::vector<u32> nl((size_t)c->sub_blocks * ns), hpos((size_t)c->sub_blocks * ns), hpidx((size_t)c->sub_blocks * ns),
        hused((size_t)c->sub_blocks * ns * 8), hntri((size_t)c->sub_blocks * ns);
    TRYR(hipStreamSynchronize(st));                                // the input is resident
    TRYR(hipEventRecord(c->ev0, st));
    float gpu_ms = 0.f;
    try {
    for (u64 first = 0; first < nblocks; first += (u64)c->sub_blocks * ns) {
        Pipe Ps[CJS_NSTREAMS];
        u32 nbs[CJS_NSTREAMS] = {0, 0, 0, 0};
        for (u32 si = 0; si < ns; si++) {
            const u64 f = first + (u64)si * c->sub_blocks;
            if (f >= nblocks) break;
            const u32 nb = (u32)(nblocks - f < c->sub_blocks ? nblocks - f : c->sub_blocks);
            nbs[si] = nb;
            hipStream_t ss = c->sub[si];
            Pipe& P = Ps[si];
            pipe_carve(P, g, c->ws[si]);
            P.g.nb = nb;
                    P.k1.linear = 1;
            u32* nls = nl.data() + (size_t)si * c->sub_blocks;
            u32 max_n = 0;
            for (u32 b = 0; b < nb; b++) {
                const u64 off = (f + b) * bs;
                nls[b] = (u32)(in_len - off < bs ? in_len - off : bs);
                if (nls[b] > max_n) max_n = nls[b];
            }
            // T_ext rows: block bytes followed by zeros (linear mode pads with the smallest symbol)
            TRYR(hipMemsetAsync(P.T, 0, (size_t)nb * g.tstride, ss));
            const u32 full = (nls[nb - 1] == bs) ? nb : nb - 1;
            if (full) TRYR(hipMemcpy2DAsync(P.T, g.tstride, (const u8*)c->din + f * bs, bs, bs, full, hipMemcpyDeviceToDevice, ss));
            if (full < nb) TRYR(hipMemcpyAsync(P.T + (size_t)full * g.tstride, (const u8*)c->din + (f + full) * bs, nls[nb - 1], hipMemcpyDeviceToDevice, ss));
            TRYR(hipMemcpyAsync(P.nlen, nls, nb * 4, hipMemcpyHostToDevice, ss));
            rc = k1_run(P.k1, P.g, max_n, ss);
            if (!rc) rc = k2_run(P, max_n, ss);
            if (!rc && tri) {
                if (si == 0 && first == 0) { if (!c->evK10[0]) { TRYR(hipEventCreate(&c->evK10[0])); TRYR(hipEventCreate(&c->evK10[1])); } TRYR(hipEventRecord(c->evK10[0], ss)); }
                rc = k10_model_run(P, (u32*)P.k1.rlist[0], (u32*)P.k1.rlist[1], P.ngroups, k10_ostride, k10_cap, ss);
                if (si == 0 && first == 0) TRYR(hipEventRecord(c->evK10[1], ss));
            }
            if (rc) { stop_coder(); (void)bwtc_end(coder); return rc; }
        }
        // the per-block results, only now: a device-to-host copy into pageable memory blocks the HOST until the stream has
        // drained, i.e. for the 132 ms of that stream's K10 - issued inside the loop above it kept the next stream's K1 / K2 /
        // K10 from even being launched (kernel trace of round 2: the two K10 launches ran back to back, 264 ms)
        for (u32 si = 0; si < ns && nbs[si]; si++) {
            hipStream_t ss = c->sub[si];
            Pipe& P = Ps[si];
            const u32 nb = nbs[si];
            const size_t o = (size_t)si * c->sub_blocks;
            if (tri) TRYR(hipMemcpyAsync(hntri.data() + o, P.ngroups, nb * 4, hipMemcpyDeviceToHost, ss));
            TRYR(hipMemcpyAsync(hpos.data() + o, P.pos, nb * 4, hipMemcpyDeviceToHost, ss));
            TRYR(hipMemcpyAsync(hpidx.data() + o, P.pidx, nb * 4, hipMemcpyDeviceToHost, ss));
            TRYR(hipMemcpyAsync(hused.data() + o * 8, P.used, (size_t)nb * 32, hipMemcpyDeviceToHost, ss));
        }
        GroupJob* job = nullptr;
        {   // a buffer the coder thread is done with
            std::unique_lock<std::mutex> lk(mu);
            cv.wait(lk, [&]() { return !c->bwtc_jobs[0].busy || !c->bwtc_jobs[1].busy; });
            job = !c->bwtc_jobs[0].busy ? &c->bwtc_jobs[0] : &c->bwtc_jobs[1];
            job->busy = true;
        }
        if (btrace) fprintf(stderr, "[bwtc] group issued at %.1f ms\n", msnow());
        job->blocks.clear();
        size_t total = 0, stotal = 0;
        for (u32 si = 0; si < ns && nbs[si]; si++) {
            TRYR(hipStreamSynchronize(c->sub[si]));
            const size_t o = (size_t)si * c->sub_blocks;
            for (u32 b = 0; b < nbs[si]; b++) {
                BlockJob bj;
                bj.len = nl[o + b]; bj.pidx = hpidx[o + b];
                bj.nsym = hpos[o + b] - 1;                         // K2 appends bzip2's EOB; BWTC has none
                bj.ntri = tri ? hntri[o + b] : 0;
                bj.host = tri && bj.ntri > k10_cap;                 // K10_OVERFLOW (or anything beyond the row: never copied)
                bj.soff = 0;
                if (bj.host) { bj.ntri = 0; bj.soff = stotal; stotal += (size_t)bj.nsym + 1; }
                memcpy(bj.used, hused.data() + (o + b) * 8, 32);
                bj.off = total;
                total += (tri ? bj.ntri : bj.nsym) + 1;
                ncalls_total += tri ? bj.ntri : bj.nsym;
                job->blocks.push_back(bj);
            }
        }
        if (btrace) fprintf(stderr, "[bwtc] K1 + K2 + K10 of the group done at %.1f ms\n", msnow());
        if (tri) {
            rc = job->a.reserve(total);
            if (!rc) rc = job->t.reserve(total);
            if (rc) { stop_coder(); (void)bwtc_end(coder); return rc; }
            if (job->sym.size() < stotal) job->sym.resize(stotal);
        }
        else if (job->sym.size() < total) job->sym.resize(total);
        size_t k = 0;
        for (u32 si = 0; si < ns && nbs[si]; si++)
            for (u32 b = 0; b < nbs[si]; b++, k++) {
                const BlockJob& bj = job->blocks[k];
                Pipe& P = Ps[si];
                if (tri && bj.host) {
                    if (bj.nsym) TRYR(hipMemcpyAsync(job->sym.data() + bj.soff, P.A + (size_t)b * g.stride, (size_t)bj.nsym * 2, hipMemcpyDeviceToHost, c->sub[si]));
                } else if (tri && bj.ntri) {
                    TRYR(hipMemcpyAsync(job->a.data() + bj.off, (u32*)P.k1.rlist[0] + (size_t)b * k10_ostride, (size_t)bj.ntri * 4, hipMemcpyDeviceToHost, c->sub[si]));
                    TRYR(hipMemcpyAsync(job->t.data() + bj.off, (u32*)P.k1.rlist[1] + (size_t)b * k10_ostride, (size_t)bj.ntri * 4, hipMemcpyDeviceToHost, c->sub[si]));
                } else if (!tri && bj.nsym) {
                    TRYR(hipMemcpyAsync(job->sym.data() + bj.off, P.A + (size_t)b * g.stride, (size_t)bj.nsym * 2, hipMemcpyDeviceToHost, c->sub[si]));
                }
            }
        if (btrace) fprintf(stderr, "[bwtc] copies issued at %.1f ms\n", msnow());
        { std::lock_guard<std::mutex> lk(mu); job->nready = 0; queue.push_back(job); cv.notify_all(); }
        for (u32 si = 0; si < ns && nbs[si]; si++) {
            TRYR(hipStreamSynchronize(c->sub[si]));
            { std::lock_guard<std::mutex> lk(mu); job->nready += nbs[si]; cv.notify_all(); }
        }
    }
    } catch (const std::exception&) {                              // e.g. std::bad_alloc while sizing a job: the coder thread must be joined
        stop_coder();
        (void)bwtc_end(coder);
        return CJS_E_NOSPACE;
    }
    const double t_issued = msnow();
    stop_coder();
    {
        float k10ms = 0.f;
        if (tri && nblocks && c->evK10[0]) (void)hipEventElapsedTime(&k10ms, c->evK10[0], c->evK10[1]);
        c->bwtc_times[0] = k10ms; c->bwtc_times[1] = (float)t_issued; c->bwtc_times[2] = (float)coder_busy; c->bwtc_times[3] = (float)msnow();
        c->bwtc_times[4] = (float)ncalls_total;
    }
    if (btrace) fprintf(stderr, "[bwtc] %llu blocks: GPU stages + copies issued and done at %.1f ms, coder started at %.1f ms, busy %.1f ms, all done at %.1f ms\n",
                        (unsigned long long)nblocks, t_issued, coder_first, coder_busy, msnow());
    TRYR(hipEventRecord(c->ev1, st));
    TRYR(hipStreamSynchronize(st));
    TRYR(hipEventElapsedTime(&gpu_ms, c->ev0, c->ev1));
    c->last_ms = gpu_ms;
    c->last_blocks = (u32)nblocks;
    {
        bwtc_coder* cc = coder;
        coder = nullptr;
        return bwtc_end(cc);
    }
#undef TRYR
}

// (bench.py) phases of the last cjs_bwtc_compress: out[0] = ms of the first K10 launch, [1] = ms until every triple was on the host,
// [2] = ms the range coder was busy, [3] = ms of the whole call, [4] = encodeFreq calls (model symbols + escapes)
extern "C" int cjs_bwtc_last_times(cjs_ctx* c, float* out5) {
    if (!c || !out5) return CJS_E_ARG;
    for (int i = 0; i < 5; i++) out5[i] = c->bwtc_times[i];
    return CJS_OK;
}

// ---------------------------------------------------------------------------------------------
// BWTC.decompressFile (lib/BWTC.js:141-233): host range decoder (serial), inverse BWT of every block on
// the GPU (K6).  The decoded bytes are retained for cjs_bwtc_fetch when `out_cap` is too small.
// ---------------------------------------------------------------------------------------------
struct BwtcSink {
    cjs_ctx* c; u8 *dT, *dU; void* ws; std::vector<u8>* out; int err;
};
static int bwtc_on_block(void* user, const uint8_t* T, uint32_t length, uint32_t pidx) {
    BwtcSink* k = (BwtcSink*)user;
    if (length == 0) return 0;
    hipStream_t st = k->c->stream;
    hipError_t e = hipMemcpyAsync(k->dT, T, length, hipMemcpyHostToDevice, st);
    if (e != hipSuccess) return CJS_E_HIP - (int)e;
    const int rc = k6_unbwt_linear(k->dT, k->dU, length, pidx, k->ws, st);     // BWT.unbwtransform :224
    if (rc) return rc;
    const size_t at = k->out->size();
    k->out->resize(at + length);
    e = hipMemcpyAsync(k->out->data() + at, k->dU, length, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    return e == hipSuccess ? 0 : CJS_E_HIP - (int)e;
}
// the three device buffers of one decode (a 900000-byte block at most), and one stream through bwtc_decode with them: what
// cjs_bwtc_decompress runs, and the host path of cjs_bwtc_decompress_batch document after document
int cjs::bwtc_dec_bufs_alloc(BwtcDecBufs& B) {
    const u32 bs = 900000u;
    const size_t wsb = (size_t)bs * 20 + ((size_t)(bs + 4095) / 4096) * 1024 + 256;
    hipError_t e;
    if ((e = hipMalloc((void**)&B.dT, bs)) != hipSuccess || (e = hipMalloc((void**)&B.dU, bs)) != hipSuccess ||
        (e = hipMalloc(&B.ws, wsb)) != hipSuccess) return CJS_E_HIP - (int)e;
    return CJS_OK;
}
void cjs::bwtc_dec_bufs_free(BwtcDecBufs& B) {
    (void)hipFree(B.dT); (void)hipFree(B.dU); (void)hipFree(B.ws);
    B.dT = B.dU = nullptr; B.ws = nullptr;
}
int cjs::bwtc_decode_one(cjs_ctx* c, const BwtcDecBufs& B, const uint8_t* in, uint64_t in_len, int64_t* declared_size, std::vector<u8>& out) {
    out.clear();
    BwtcSink k = {c, B.dT, B.dU, B.ws, &out, 0};
    const int rc = bwtc_decode(in, in_len, declared_size, &k, bwtc_on_block);
    (void)hipStreamSynchronize(c->stream);
    if (rc) out.clear();
    return rc;
}
extern "C" int64_t cjs_bwtc_decompress(cjs_ctx* c, const uint8_t* in, uint64_t in_len, uint8_t* out, uint64_t out_cap,
                                       int64_t* declared_size) {
    if (!c || (!in && in_len)) return CJS_E_ARG;
    if (hipSetDevice(c->device) != hipSuccess) return CJS_E_NOGPU;
    c->bwtc_out.clear();
    BwtcDecBufs B;
    int rc = bwtc_dec_bufs_alloc(B);
    if (!rc) rc = bwtc_decode_one(c, B, in, in_len, declared_size, c->bwtc_out);
    else (void)hipStreamSynchronize(c->stream);
    bwtc_dec_bufs_free(B);
    if (rc) { c->bwtc_out.clear(); return rc; }
    return cjs_bwtc_fetch(c, out, out_cap);
}
extern "C" int64_t cjs_bwtc_last_size(cjs_ctx* c) { return c ? (int64_t)c->bwtc_out.size() : 0; }
extern "C" int64_t cjs_bwtc_fetch(cjs_ctx* c, uint8_t* out, uint64_t out_cap) {
    if (!c) return CJS_E_ARG;
    const u64 n = c->bwtc_out.size();
    if (n > out_cap) return CJS_E_NOSPACE;
    if (n) memcpy(out, c->bwtc_out.data(), n);
    return (int64_t)n;
}
