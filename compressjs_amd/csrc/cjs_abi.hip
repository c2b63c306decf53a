// C ABI of libcompressjs_amd.so (declared in include/compressjs_amd.h): the context, the block pipeline behind every bzip2
// compress call (issue_blocks), the device-resident and the host-buffer entry, the decoder entries, accessors and profile readers.
#include "cjs_ctx.h"
#include <atomic>
#include <stdlib.h>

using namespace cjs;

extern "C" int32_t cjs_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n < 0) return 0;
    return n;
}

extern "C" cjs_ctx* cjs_create(int device, uint32_t batch_blocks) {
    if (cjs_device_count() <= 0) return nullptr;
    if (hipSetDevice(device) != hipSuccess) return nullptr;
    cjs_ctx* c = new cjs_ctx();
    c->device = device;
    c->batch_blocks = batch_blocks ? batch_blocks : 128;
    // Two streams by default, each driven by its own host thread (issue_blocks): the latency-bound kernels of one half of
    // the batch (K3/K4: four workgroups per block, the sparse rounds, the small scans, K1's read-backs) overlap with
    // the bandwidth-bound ones of the other.  Measured, 10^8 bytes, ms per step with 1 / 2 / 3 / 4 streams: enwik
    // 14.86 / 14.35 / 14.73 / 17.72, E8S-A 23.94 / 21.45 / 21.90 / 27.48, random ASCII 12.81 / 12.07 / 12.58 / 15.35 (round 2;
    // round 3, enwik: one stream 9.4, two 8.7, three 8.7, four 11.6 - the main stream and four more share four hardware queues).
    // CJS_STREAMS=1 gives every kernel the GPU to itself: what per-kernel timings (bench.py's roofline leg, rocprof
    // summaries) are taken with.
    c->nstreams = batch_blocks && batch_blocks < 32 ? 1 : 2;
    if (const char* ev = getenv("CJS_STREAMS")) {
        const int v = atoi(ev);
        if (v >= 1 && v <= CJS_NSTREAMS) c->nstreams = (u32)v;
    }
#ifdef CJS_CPU_DEBUG_BUILD
    c->nstreams = 1;                             // the CPU logic-debug build runs kernels as fibers of one thread
#endif
    for (u32 i = 0; i < c->nstreams; i++) c->share[i] = 1000u / c->nstreams + (i < 1000u % c->nstreams ? 1u : 0u);
    if (const char* ev = getenv("CJS_SHARES")) {        // "300,700": unequal sub-batches (the streams then leave K1 at different times)
        u32 v[CJS_NSTREAMS], n = 0, sum = 0;
        for (const char* q = ev; *q && n < CJS_NSTREAMS; ) {
            v[n] = (u32)strtoul(q, (char**)&q, 10); sum += v[n++];
            if (*q == ',' || *q == ':') q++;
        }
        bool good = n >= 1 && sum == 1000u;
        for (u32 i = 0; i < n; i++) good = good && v[i] >= 50u;
#ifndef CJS_CPU_DEBUG_BUILD
        if (good) { c->nstreams = n; for (u32 i = 0; i < n; i++) c->share[i] = v[i]; }
#endif
    }
    {
        u32 mx = 0;
        for (u32 i = 0; i < c->nstreams; i++) mx = c->share[i] > mx ? c->share[i] : mx;
        c->sub_blocks = (u32)(((u64)c->batch_blocks * mx + 999u) / 1000u);
    }
    bool ok = hipStreamCreate(&c->stream) == hipSuccess;
    BatchGeom g = make_geom(c->sub_blocks, block_cap(9));
    c->ws_bytes = pipe_bytes(g);
    for (u32 i = 0; ok && i < c->nstreams; i++) {
        ok = ok && hipStreamCreate(&c->sub[i]) == hipSuccess;
        ok = ok && hipMalloc(&c->ws[i], c->ws_bytes) == hipSuccess;
        ok = ok && hipEventCreateWithFlags(&c->evScan[i], hipEventDisableTiming) == hipSuccess;
        ok = ok && hipEventCreateWithFlags(&c->evDone[i], hipEventDisableTiming) == hipSuccess;
        ok = ok && hipHostMalloc((void**)&c->pin[i], CJS_PIN_WORDS * 4) == hipSuccess;
        ok = ok && hipEventCreateWithFlags(&c->evPad[i], hipEventDisableTiming) == hipSuccess;
        ok = ok && hipEventCreateWithFlags(&c->evCrc[i], hipEventDisableTiming) == hipSuccess;
    }
#ifndef CJS_CPU_DEBUG_BUILD
    if (ok && !getenv("CJS_NO_SIDE_CRC")) ok = hipStreamCreate(&c->side) == hipSuccess;
#endif
    ok = ok && hipEventCreateWithFlags(&c->evReady, hipEventDisableTiming) == hipSuccess;
    ok = ok && hipMalloc((void**)&c->d_ss, 256) == hipSuccess;
    ok = ok && hipEventCreate(&c->ev0) == hipSuccess && hipEventCreate(&c->ev1) == hipSuccess;
    if (!ok) { cjs_destroy(c); return nullptr; }
    return c;
}

extern "C" void cjs_destroy(cjs_ctx* c) {
    if (!c) return;
    (void)hipSetDevice(c->device);
    (void)hipDeviceSynchronize();
    for (int i = 0; i < CJS_NSTREAMS; i++) {
        (void)hipFree(c->ws[i]);
        if (c->evScan[i]) (void)hipEventDestroy(c->evScan[i]);
        if (c->evDone[i]) (void)hipEventDestroy(c->evDone[i]);
        if (c->pin[i]) (void)hipHostFree(c->pin[i]);
        if (c->evPad[i]) (void)hipEventDestroy(c->evPad[i]);
        if (c->evCrc[i]) (void)hipEventDestroy(c->evCrc[i]);
        c->helper[i].stop();                               // (before the stream it issues to goes)
        if (c->sub[i]) (void)hipStreamDestroy(c->sub[i]);
    }
    (void)hipFree(c->d_ss); (void)hipFree(c->k0ws); (void)hipFree(c->planws); (void)hipFree(c->din); (void)hipFree(c->dout);
    if (c->evReady) (void)hipEventDestroy(c->evReady);
    if (c->ev0) (void)hipEventDestroy(c->ev0);
    if (c->ev1) (void)hipEventDestroy(c->ev1);
    for (int i = 0; i < 2; i++) if (c->evK10[i]) (void)hipEventDestroy(c->evK10[i]);
    for (int i = 0; i < CJS_NSTREAMS; i++) { if (c->evB10[i]) (void)hipEventDestroy(c->evB10[i]); if (c->evB11[i]) (void)hipEventDestroy(c->evB11[i]); }
    for (int i = 0; i < 5; i++) (void)hipFree(c->bd[i]);
    k1_prof_destroy(c->prof);
    dec_free(c->dec);
    for (int i = 0; i < 3; i++) c->io[i].stop();
    for (hipEvent_t ev : c->evPool) (void)hipEventDestroy(ev);
    if (c->snapPin) (void)hipHostFree(c->snapPin);
    (void)hipFree(c->k0sl);
    for (auto& pr : c->segpool) (void)hipFree(pr.first);
    if (c->side) (void)hipStreamDestroy(c->side);
    if (c->sIn) (void)hipStreamDestroy(c->sIn);
    if (c->sOut) (void)hipStreamDestroy(c->sOut);
    if (c->stream) (void)hipStreamDestroy(c->stream);
    delete c;
}

extern "C" int64_t cjs_bz2_compress_bound(uint64_t in_len) {
    // RLE1 expands by at most 5/4, Huffman codes are at most 20 bits per symbol; headers per block
    return (int64_t)(in_len + in_len / 2 + (in_len / 100000 + 2) * 24576 + 4096);
}

int cjs::grow(void** p, size_t* have, size_t need) {
    if (*have >= need) return CJS_OK;
    (void)hipFree(*p);
    *p = nullptr; *have = 0;
    need = (need + (1u << 20)) & ~(size_t)((1u << 20) - 1);
    hipError_t e = hipMalloc(p, need);
    if (e != hipSuccess) return CJS_E_HIP - (int)e;
    *have = need;
    return CJS_OK;
}

// Issue blocks [first, first+count) of the planned input K as sub-batches round-robin over the
// context's streams.  Stream 0 must already hold the pre-pass + output zeroing (evReady).
// One sub-batch = up to sub_blocks blocks through K0 (materialise) .. K5 on one stream.  The only
// cross-stream dependency is the stream cursor: k5_blockscan of sub-batch j needs the cursor left by
// sub-batch j-1 (an event); everything before it overlaps freely.
int cjs::run_sub_batch(cjs_ctx* c, const K0Buf& K, const BatchGeom& g, u32 cap, u32 f, u32 nb, u32 si, void* d_out,
                       uint64_t out_cap, Pipe& P, u32 total_blocks) {
    hipStream_t st = c->sub[si];
    pipe_carve(P, g, c->ws[si]);
    P.ss = c->d_ss;
    P.out = (u32*)d_out;
    P.outCapBytes = out_cap & ~(uint64_t)3;
    P.k1.prof = c->prof.enabled ? &c->prof : nullptr;
    P.k1.hpin = c->pin[si]; P.k1.hpinWords = CJS_PIN_WORDS;
    P.g.nb = nb;
    // (CRC workgroups per block: one per 2 MB of input a block of this call consumes on average - long runs make that tens of megabytes;
    // total_blocks = the blocks the planned input K holds, so that windows with a margin and sub-ranges count their own bytes)
    const u64 per_block = K.in_len / (total_blocks ? total_blocks : 1u);
    int rc = k0_batch(K, P, f, cap, st, (u32)(1u + per_block / (2u << 20)), c->side, c->side ? c->evPad[si] : nullptr, c->side ? c->evCrc[si] : nullptr);
    if (rc) return rc;
    return pipe_run_block_stages(P, cap, st, 4);
}

int cjs::issue_blocks(cjs_ctx* c, const K0Buf& K, u32 cap, u32 first, u32 count, void* d_out, uint64_t out_cap, const K5Docs* docs) {
    BatchGeom g = make_geom(c->sub_blocks, cap);
    if (c->prof.enabled) c->prof_g = g;                   // (once, before the workers start: they only read it)
    // The blocks go out in batches of batch_blocks; a batch is cut into one sub-batch per stream by the streams' shares
    // (when it has at least 16 blocks per stream: below that one stream takes it whole, or sub_blocks at a time).
    std::vector<u32> sfirst, scount;
    for (u32 f = 0; f < count; ) {
        const u32 wave = count - f < c->batch_blocks ? count - f : c->batch_blocks;
        if (c->nstreams > 1 && wave >= 16 * c->nstreams) {
            u32 acc = 0, done = 0;
            for (u32 i = 0; i < c->nstreams; i++) {
                acc += c->share[i];
                const u32 upto = i + 1 == c->nstreams ? wave : (u32)(((u64)wave * acc + 500u) / 1000u);
                if (upto > done) { sfirst.push_back(first + f + done); scount.push_back(upto - done); }
                done = upto;
            }
            f += wave;
        } else {
            const u32 take = wave < c->sub_blocks ? wave : c->sub_blocks;
            sfirst.push_back(first + f); scount.push_back(take);
            f += take;
        }
    }
    const u32 nsub = (u32)sfirst.size();
    const u32 ns = c->nstreams < nsub ? c->nstreams : nsub;
    for (u32 i = 0; i < ns; i++) HIP_CHECK_RET(hipStreamWaitEvent(c->sub[i], c->evReady, 0));
    // K1 steers itself with small read-backs (stream syncs), so every stream gets its own host thread:
    // while one sub-batch waits for its counters the other keeps the GPU fed.  The cursor events are
    // recorded and waited for in sub-batch order (`recorded` hands the order from thread to thread).
    std::atomic<u32> recorded(0);
    std::atomic<int> err(0);
    auto worker = [&](u32 si) {
        if (hipSetDevice(c->device) != hipSuccess) { int z = 0; err.compare_exchange_strong(z, CJS_E_NOGPU); }   // (it still walks its slots below, work skipped: the hand-off chain must complete - ADVICE r4)
        for (u32 j = si; j < nsub; j += ns) {
            const u32 f = sfirst[j], nb = scount[j];
            Pipe P;
            int rc = err.load() ? err.load() : run_sub_batch(c, K, g, cap, f, nb, si, d_out, out_cap, P, first + count);
            while (recorded.load(std::memory_order_acquire) != j) std::this_thread::yield();
            if (!rc && !err.load()) rc = k5_run(P, cap, c->sub[si], j ? c->evScan[(j - 1) % ns] : nullptr, c->evScan[si], c->side ? c->evCrc[si] : nullptr, docs, f);
            if (rc) { int z = 0; err.compare_exchange_strong(z, rc); }
            recorded.store(j + 1, std::memory_order_release);
        }
    };
    if (ns <= 1) worker(0);
    else {
        for (u32 i = 1; i < ns; i++) {
            c->helper[i].post([&worker, i]() { worker(i); });
        }
        worker(0);
        for (u32 i = 1; i < ns; i++) c->helper[i].wait();
    }
    if (err.load()) {
        // (the block CRCs run on c->side and only k5_run joins them back: on an error between the two, k0_crc may still be reading the input and
        // XOR-ing into the workspace when the call returns - ADVICE r5)
        if (c->side) (void)hipStreamSynchronize(c->side);
        return err.load();
    }
    for (u32 i = 0; i < ns; i++) {
        HIP_CHECK_RET(hipEventRecord(c->evDone[i], c->sub[i]));
        HIP_CHECK_RET(hipStreamWaitEvent(c->stream, c->evDone[i], 0));
    }
    return CJS_OK;
}

extern "C" int64_t cjs_bz2_compress_device(cjs_ctx* c, const void* d_in, uint64_t in_len, int level,
                                           void* d_out, uint64_t out_cap) {
    if (!c || (!d_in && in_len) || !d_out) return CJS_E_ARG;
    if (level < 1 || level > 9) return CJS_E_LEVEL;                  // lib/Bzip2.js:888-890
    if (out_cap < 64 || ((uintptr_t)d_out & 3)) return CJS_E_ARG;
    HIP_CHECK_RET(hipSetDevice(c->device));
    const u32 cap = block_cap(level);
    hipStream_t st = c->stream;
    int rc = grow(&c->k0ws, &c->k0ws_bytes, k0_bytes(in_len, cap));
    if (rc) return rc;
    K0Buf K;
    k0_carve(K, (const u8*)d_in, in_len, cap, c->k0ws);
    Pipe P0 = stream_pipe(c, d_out, out_cap);
    HIP_CHECK_RET(hipEventRecord(c->ev0, st));
    // the output is zeroed (k5_pack ORs into it) on a sub-batch stream NEXT TO the pre-pass instead of behind it (23 us per 10^8 bytes at the
    // head of every call); k5_begin and evReady come behind both
    HIP_CHECK_RET(hipStreamWaitEvent(c->sub[0], c->ev0, 0));
    HIP_CHECK_RET(hipMemsetAsync(P0.out, 0, P0.outCapBytes, c->sub[0]));
    HIP_CHECK_RET(hipEventRecord(c->evDone[0], c->sub[0]));
    rc = k0_prepass(K, cap, st);
    if (rc) { (void)hipStreamSynchronize(c->sub[0]); return rc; }     // (the zeroing of the caller's buffer is still in flight - ADVICE r4)
    HIP_CHECK_RET(hipStreamWaitEvent(st, c->evDone[0], 0));        // (k5_begin writes the stream header into the zeroed output)
    rc = k5_stream_begin(P0, level, st, false);
    if (rc) { (void)hipStreamSynchronize(c->sub[0]); return rc; }
    HIP_CHECK_RET(hipEventRecord(c->evReady, st));
    // (both small read-backs of the call go through the context's pinned memory - stream 0's, which no sub-batch is using at either time:
    // a pageable copy costs tens of microseconds more, with the GPU idle behind the first one)
    HIP_CHECK_RET(hipMemcpyAsync(c->pin[0], K.nBlocks, 4, hipMemcpyDeviceToHost, st));
    HIP_CHECK_RET(hipStreamSynchronize(st));
    const u32 nblocks = c->pin[0][0];
    rc = issue_blocks(c, K, cap, 0, nblocks, d_out, out_cap);
    if (rc) return rc;
    rc = k5_stream_end(P0, st);
    if (rc) return rc;
    HIP_CHECK_RET(hipEventRecord(c->ev1, st));
    const int64_t bits = stream_bits(c, st, c->pin[0]);
    if (bits < 0 && bits != CJS_E_NOSPACE) return bits;
    HIP_CHECK_RET(hipEventElapsedTime(&c->last_ms, c->ev0, c->ev1));
    c->last_blocks = nblocks;
    return bits < 0 ? bits : (bits + 7) >> 3;
}

int64_t cjs::stream_bits(cjs_ctx* c, hipStream_t st, u32* pin, u32* crc) {
    StreamState hs;
    HIP_CHECK_RET(hipMemcpyAsync(pin ? (void*)pin : (void*)&hs, c->d_ss, sizeof hs, hipMemcpyDeviceToHost, st));
    HIP_CHECK_RET(hipStreamSynchronize(st));
    if (pin) memcpy(&hs, pin, sizeof hs);
    if (hs.overflow) return CJS_E_NOSPACE;
    if (crc) *crc = hs.crc;
    return (int64_t)hs.bits;
}

uint64_t cjs::seg_bytes_for(const cjs_ctx* c, u32 cap, bool* from_env) {
    const char* ev = getenv("CJS_SEG_BYTES");                       // (read per call)
    const uint64_t v = ev ? strtoull(ev, nullptr, 10) : 0;
    if (from_env) *from_env = v != 0;
    return v ? v : (uint64_t)c->batch_blocks * cap;
}

extern "C" int64_t cjs_bz2_compress(cjs_ctx* c, const uint8_t* in, uint64_t in_len, int level, uint8_t* out,
                                    uint64_t out_cap) {
    if (!c || (!in && in_len) || !out) return CJS_E_ARG;
    if (level < 1 || level > 9) return CJS_E_LEVEL;
    HIP_CHECK_RET(hipSetDevice(c->device));
    const uint64_t need = (uint64_t)cjs_bz2_compress_bound(in_len);
    int rc = grow(&c->din, &c->din_bytes, in_len + 64);
    if (rc) return rc;
    rc = grow(&c->dout, &c->dout_bytes, need);
    if (rc) return rc;
    // one batch of blocks per segment; CJS_SEG_BYTES (tests) overrides.  Inputs of up to a batch and a half go in one
    // piece: half-size batches cost more (16.9 vs 14.2 ms per 10^8 bytes) than overlapping their copies would save.
    const u32 cap = block_cap(level);
    bool seg_env = false;
    const uint64_t seg_bytes = seg_bytes_for(c, cap, &seg_env);
    bool resident = false;
#ifndef CJS_CPU_DEBUG_BUILD
    {
        // the overlapped path: slices of CJS_SLICE_BLOCKS blocks - any input of at least two slices.  OFF by default (0): measured on the MI355X
        // (10^8 bytes of enwik, device-resident step 7.5 ms, one piece 9.92 ms host to host): 2 streams x slices of 28 / 40 / 56 blocks 10.9 /
        // 10.0 / 10.2 ms, 3 streams x 40 9.65, explicit 64+48 10.0, 4 streams 10.4 - a slice of 28 blocks takes 3.5-4.5 ms from its first
        // launch to its last however few blocks it has (a chain of ~160 launches, K1's read-back in the middle; tests/gpu_host_path_probe.py
        // with CJS_OV_TRACE=1 prints the timeline), so what the copies gain the shorter sub-batches lose.  Same bytes either way.
        static const u32 slice_blocks = []() -> u32 { const char* ev = getenv("CJS_SLICE_BLOCKS"); return ev ? (u32)strtoul(ev, nullptr, 10) : 0u; }();
        if (slice_blocks && !seg_env && in_len >= (uint64_t)slice_blocks * cap * 3 / 2) {
            const int64_t r = compress_overlapped(c, in, in_len, level, out, out_cap, slice_blocks);
            if (r != CJS_E_SPEC && r != CJS_OV_NOT_STARTED) return r;
            resident = r == CJS_E_SPEC;                     // a slice refused its plan (rare): the uploader has run to its end, the input is in HBM - one piece from here
        }
    }
#endif
    if (!resident && in_len > seg_bytes + seg_bytes / 2) return compress_segmented(c, in, in_len, level, out, out_cap, seg_bytes);
    if (!resident && in_len) HIP_CHECK_RET(hipMemcpyAsync(c->din, in, in_len, hipMemcpyHostToDevice, c->stream));
    const int64_t n = cjs_bz2_compress_device(c, c->din, in_len, level, c->dout, c->dout_bytes);
    if (n < 0) return n;
    if ((uint64_t)n > out_cap) return CJS_E_NOSPACE;
    HIP_CHECK_RET(hipMemcpy(out, c->dout, (size_t)n, hipMemcpyDeviceToHost));
    return n;
}

// Seam helper of the multi-GPU assembly (compressjs_amd/dist.py): d_out[0 .. nbytes] = the nbytes of
// d_in shifted right by `s` (0..7) bits.  Device pointers; d_out needs nbytes + 1 bytes.
extern "C" int32_t cjs_shift_bits(cjs_ctx* c, const uint8_t* d_in, uint64_t nbytes, uint32_t s, uint8_t* d_out) {
    if (!c || !d_in || !d_out || s > 7) return CJS_E_ARG;
    if (hipSetDevice(c->device) != hipSuccess) return CJS_E_NOGPU;
    const int rc = k5_shift_bits_run(d_in, nbytes, s, d_out, c->stream);
    if (rc) return rc;
    const hipError_t e = hipStreamSynchronize(c->stream);
    return e == hipSuccess ? CJS_OK : CJS_E_HIP - (int)e;
}

// ---------------------------------------------------------------------------------------------
// Workload generator of BASELINE.json configs[3] / SURVEY.md 8(c) on the device: bytes [first, first + n) of LCG(N, seed),
//   s <- s * 1664525 + 1013904223 (mod 2^32), byte = 32 + ((s >>> 16) mod 95),
// so that every rank of a multi-GPU run fills its own slice in HBM instead of receiving it from the host.  Jump-ahead:
// s_j = A^j s_0 + C (A^(j-1) + ... + 1); each thread squares its way to the state of its first byte (32 steps), then
// walks 16 bytes.  Same bytes as compressjs_amd.synth.lcg_ascii (tests).  Not a compression entry point.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_lcg_fill(u8* out, u64 n, u32 seed, u64 first) {
    const u64 t = (u64)blockIdx.x * 256u + threadIdx.x;
    const u64 i0 = t * 16u;
    if (i0 >= n) return;
    // state after j = first + i0 steps: affine map x -> a x + c composed j times by binary powering
    u64 j = first + i0;
    u32 ra = 1u, rc = 0u;                    // result map (identity)
    u32 ba = 1664525u, bc = 1013904223u;     // current power of the base map
    while (j) {
        if (j & 1u) { rc = ba * rc + bc; ra = ba * ra; }
        bc = ba * bc + bc; ba = ba * ba;
        j >>= 1;
    }
    u32 st = ra * seed + rc;
    const u64 m = n - i0 < 16u ? n - i0 : 16u;
    for (u64 k = 0; k < m; k++) {
        st = st * 1664525u + 1013904223u;
        out[i0 + k] = (u8)(32u + ((st >> 16) % 95u));
    }
}

extern "C" int32_t cjs_lcg_ascii_device(cjs_ctx* c, uint8_t* d_out, uint64_t n, uint32_t seed, uint64_t first) {
    if (!c || (!d_out && n)) return CJS_E_ARG;
    if (hipSetDevice(c->device) != hipSuccess) return CJS_E_NOGPU;
    if (n) hipLaunchKernelGGL(k_lcg_fill, dim3((unsigned)((n + 4095) / 4096)), dim3(256), 0, c->stream, d_out, n, seed, first);
    const hipError_t e = hipStreamSynchronize(c->stream);
    return e == hipSuccess ? CJS_OK : CJS_E_HIP - (int)e;
}

extern "C" float cjs_last_device_ms(const cjs_ctx* c) { return c ? c->last_ms : 0.f; }
extern "C" uint32_t cjs_last_block_count(const cjs_ctx* c) { return c ? c->last_blocks : 0; }
extern "C" void* cjs_stream(const cjs_ctx* c) { return c ? (void*)c->stream : nullptr; }

// Per-kernel timing of K1's main kernels with HIP events on the library's own streams, for bench.py's roofline leg
// (K1P_* classes of k1_bwt.h: 0 k1f_bsort, 1 k1r_round, 2 k1d_build, 3 k1d_round, 4 k1d_med, 5 k1d_large, 6 k1d_update,
// 7 k1f_task).  cjs_profile_enable(1) clears the records; the classes can be read in any order while they stand.
extern "C" int32_t cjs_profile_enable(cjs_ctx* c, int on) {
    if (!c) return CJS_E_ARG;
    return k1_prof_enable(c->prof, on);
}
extern "C" int32_t cjs_profile_read_class(cjs_ctx* c, uint32_t cls, float* total_ms, uint32_t* launches, uint64_t* elements) {
    if (!c || cls >= K1_PROF_CLASSES) return CJS_E_ARG;
    hipError_t e = hipSetDevice(c->device);
    if (e != hipSuccess) return CJS_E_HIP - (int)e;
    u64 el = 0;
    const int rc = k1_prof_read(c->prof, cls, total_ms, launches, &el);
    if (rc) return rc;
    if (cls == K1P_DROUND || cls == K1P_DUPDATE) {
        // list entries the doubling rounds walked: the counters of the LAST sub-batch of stream 0 (what a one-stream pass over
        // equal batches leaves), times the k1_dbl_run calls recorded
        const BatchGeom g = c->prof_g;
        if (!g.nb) { if (elements) *elements = 0; return CJS_OK; }
        Pipe P;
        pipe_carve(P, g, c->ws[0]);
        std::vector<u32> cn((size_t)(K1D_MAXR + 2) * P.k1.rstride);
        e = hipMemcpy(cn.data(), P.k1.dcnt, cn.size() * 4, hipMemcpyDeviceToHost);
        if (e != hipSuccess) return CJS_E_HIP - (int)e;
        u64 tot = 0;
        for (u32 v : cn) tot += v;
        el = tot * c->prof.dbl_runs;
    }
    if (elements) *elements = el;
    return CJS_OK;
}
extern "C" int32_t cjs_profile_read(cjs_ctx* c, float* total_ms, uint32_t* launches, uint64_t* elements) {
    return cjs_profile_read_class(c, K1P_BSORT, total_ms, launches, elements);
}

// ---------------------------------------------------------------------------------------------
// decoder: Bzip2.decompressFile / decompressBlock / table (lib/Bzip2.js:454-548)
// ---------------------------------------------------------------------------------------------
static u32 dec_slots(const cjs_ctx* c) { return c->batch_blocks < 16 ? 16u : c->batch_blocks; }

static int64_t dec_deliver(cjs_ctx* c, int64_t n, uint8_t* out, uint64_t out_cap, bool out_dev) {
    if (n < 0) return n;
    if ((uint64_t)n > out_cap) return CJS_E_NOSPACE;             // result stays fetchable (cjs_bz2_fetch)
    if (n == 0) return 0;
    if (!out) return CJS_E_ARG;
    u64 sz = 0;
    const u8* d = dec_output(c->dec, &sz);
    hipError_t e = hipMemcpyAsync(out, d, (size_t)n, out_dev ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, c->stream);
    dec_sync_note();
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    return e == hipSuccess ? n : (int64_t)(CJS_E_HIP - (int)e);
}

static int64_t dec_timed(cjs_ctx* c, const uint8_t* in, uint64_t in_len, bool in_dev, int multistream, bool check_crc) {
    if (!c || (!in && in_len)) return CJS_E_ARG;
    if (hipSetDevice(c->device) != hipSuccess) return CJS_E_NOGPU;
    (void)hipEventRecord(c->ev0, c->stream);
    const int64_t n = dec_stream(&c->dec, dec_slots(c), c->stream, in, in_len, in_dev, multistream, check_crc);
    (void)hipEventRecord(c->ev1, c->stream);
    (void)hipStreamSynchronize(c->stream);
    c->dec_ms = 0.f;
    (void)hipEventElapsedTime(&c->dec_ms, c->ev0, c->ev1);
    return n;
}

extern "C" int64_t cjs_bz2_decompress(cjs_ctx* c, const uint8_t* in, uint64_t in_len, uint8_t* out, uint64_t out_cap,
                                      int multistream) {
    return dec_deliver(c, dec_timed(c, in, in_len, false, multistream, true), out, out_cap, false);
}
extern "C" int64_t cjs_bz2_decompress_device(cjs_ctx* c, const uint8_t* d_in, uint64_t in_len, uint8_t* d_out,
                                             uint64_t out_cap, int multistream) {
    return dec_deliver(c, dec_timed(c, d_in, in_len, true, multistream, true), d_out, out_cap, true);
}
extern "C" int64_t cjs_bz2_decompress_block(cjs_ctx* c, const uint8_t* in, uint64_t in_len, uint64_t bitpos,
                                            uint8_t* out, uint64_t out_cap) {
    if (!c || (!in && in_len)) return CJS_E_ARG;
    if (hipSetDevice(c->device) != hipSuccess) return CJS_E_NOGPU;
    return dec_deliver(c, dec_block(&c->dec, dec_slots(c), c->stream, in, in_len, bitpos), out, out_cap, false);
}
// Bzip2.table: callback(position in bits, decoded bytes) per block -> two arrays; returns the block count
extern "C" int64_t cjs_bz2_table(cjs_ctx* c, const uint8_t* in, uint64_t in_len, int multistream, uint64_t* positions,
                                 uint64_t* sizes, uint32_t cap) {
    const int64_t n = dec_timed(c, in, in_len, false, multistream, false);     // the stream CRC is ignored (:536)
    if (n < 0) return n;
    const u64 *p = nullptr, *z = nullptr;
    const u32 nb = dec_table(c->dec, &p, &z);
    for (u32 i = 0; i < nb && i < cap; i++) { if (positions) positions[i] = p[i]; if (sizes) sizes[i] = z[i]; }
    return (int64_t)nb;
}
// size / bytes of the last successful decode (for callers that learn the size from the first call)
extern "C" int64_t cjs_bz2_last_size(cjs_ctx* c) {
    u64 sz = 0;
    if (!c || !c->dec) return 0;
    (void)dec_output(c->dec, &sz);
    return (int64_t)sz;
}
extern "C" int64_t cjs_bz2_fetch(cjs_ctx* c, uint8_t* out, uint64_t out_cap) {
    if (!c || !c->dec) return CJS_E_ARG;
    if (hipSetDevice(c->device) != hipSuccess) return CJS_E_NOGPU;
    return dec_deliver(c, cjs_bz2_last_size(c), out, out_cap, false);
}
// detail of the last decoder error: 1 'bad magic', 2 'level out of range', 3 'initial position out of
// bounds', 4 'Bad block CRC (got .. expected ..)', 5 'Bad stream CRC (got .. expected ..)'
extern "C" int32_t cjs_bz2_last_detail(cjs_ctx* c, uint32_t* crc_got, uint32_t* crc_expected) {
    int d = 0; u32 g = 0, w = 0;
    if (c && c->dec) dec_error_info(c->dec, &d, &g, &w);
    if (crc_got) *crc_got = g;
    if (crc_expected) *crc_expected = w;
    return d;
}
extern "C" float cjs_bz2_last_decode_ms(cjs_ctx* c) { return c ? c->dec_ms : 0.f; }
extern "C" int cjs_dbg_dec_syncs(void) { return dec_sync_count(); }

// Batched form (declared in include/compressjs_amd.h): document d decodes as Bzip2.decompressFile (lib/Bzip2.js:454-481) does on it
// alone; the document level is in decode.hip (dec_batch) and k7_docs.hip.
static int64_t dec_batch_call(cjs_ctx* c, const uint8_t* in, const uint64_t* off, uint32_t count, int multistream, uint8_t* out,
                              uint64_t out_cap, uint64_t* out_off, int32_t* status, uint32_t* detail, bool dev) {
    if (!c) return CJS_E_ARG;
    if (count == 0) return 0;
    if (!off || !out_off || !status) return CJS_E_ARG;
    if (hipSetDevice(c->device) != hipSuccess) return CJS_E_NOGPU;
    (void)hipEventRecord(c->ev0, c->stream);
    const int64_t n = dec_batch(&c->dec, dec_slots(c), c->stream, in, (const u64*)off, count, dev, multistream, (u64*)out_off, status, detail);
    (void)hipEventRecord(c->ev1, c->stream);
    dec_sync_note();
    (void)hipStreamSynchronize(c->stream);
    c->dec_ms = 0.f;
    (void)hipEventElapsedTime(&c->dec_ms, c->ev0, c->ev1);
    return dec_deliver(c, n, out, out_cap, dev);
}
extern "C" int64_t cjs_bz2_decompress_batch(cjs_ctx* c, const uint8_t* in, const uint64_t* off, uint32_t count, int multistream,
                                            uint8_t* out, uint64_t out_cap, uint64_t* out_off, int32_t* status, uint32_t* detail) {
    return dec_batch_call(c, in, off, count, multistream, out, out_cap, out_off, status, detail, false);
}
extern "C" int64_t cjs_bz2_decompress_batch_device(cjs_ctx* c, const uint8_t* d_in, const uint64_t* d_off, uint32_t count, int multistream,
                                                   uint8_t* d_out, uint64_t out_cap, uint64_t* d_out_off, int32_t* d_status,
                                                   uint32_t* d_detail) {
    return dec_batch_call(c, d_in, d_off, count, multistream, d_out, out_cap, d_out_off, d_status, d_detail, true);
}

// A list of blocks of one stream (declared in include/compressjs_amd.h): request k decodes as Bzip2.decompressBlock (lib/Bzip2.js:482-503)
// does at bitpos[k] alone; the request level is in decode.hip (dec_blocks) and k7_blocks.hip.
static int64_t dec_blocks_call(cjs_ctx* c, const uint8_t* in, uint64_t in_len, const uint64_t* bitpos, uint32_t count, uint8_t* out,
                               uint64_t out_cap, uint64_t* out_off, int32_t* status, uint32_t* detail, bool dev) {
    if (!c) return CJS_E_ARG;
    if (count == 0) return 0;
    if ((!in && in_len) || !bitpos || !out_off || !status) return CJS_E_ARG;
    if (hipSetDevice(c->device) != hipSuccess) return CJS_E_NOGPU;
    (void)hipEventRecord(c->ev0, c->stream);
    const int64_t n = dec_blocks(&c->dec, dec_slots(c), c->stream, in, in_len, (const u64*)bitpos, count, dev, (u64*)out_off, status, detail);
    (void)hipEventRecord(c->ev1, c->stream);
    dec_sync_note();
    (void)hipStreamSynchronize(c->stream);
    c->dec_ms = 0.f;
    (void)hipEventElapsedTime(&c->dec_ms, c->ev0, c->ev1);
    return dec_deliver(c, n, out, out_cap, dev);
}
extern "C" int64_t cjs_bz2_decompress_blocks(cjs_ctx* c, const uint8_t* in, uint64_t in_len, const uint64_t* bitpos, uint32_t count,
                                             uint8_t* out, uint64_t out_cap, uint64_t* out_off, int32_t* status, uint32_t* detail) {
    return dec_blocks_call(c, in, in_len, bitpos, count, out, out_cap, out_off, status, detail, false);
}
extern "C" int64_t cjs_bz2_decompress_blocks_device(cjs_ctx* c, const uint8_t* d_in, uint64_t in_len, const uint64_t* d_bitpos, uint32_t count,
                                                    uint8_t* d_out, uint64_t out_cap, uint64_t* d_out_off, int32_t* d_status,
                                                    uint32_t* d_detail) {
    return dec_blocks_call(c, d_in, in_len, d_bitpos, count, d_out, out_cap, d_out_off, d_status, d_detail, true);
}
