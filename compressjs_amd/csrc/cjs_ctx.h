// The context behind the C ABI and what the host translation units (cjs_abi.hip, cjs_host_paths.hip, cjs_multi.hip,
// cjs_bwtc.hip) share.  Private to the library: everything that is not extern "C" lives in namespace cjs.
#pragma once
#include "../../include/compressjs_amd.h"
#include "cjs_common.h"
#include "k1_bwt.h"
#include "pipeline.h"
#include "decode_host.h"
#include <vector>
#include <thread>
#include <functional>
#include <mutex>
#include <condition_variable>
#include <string.h>

#define CJS_PIN_WORDS 8192u  // pinned words per stream for K1's read-backs
#define CJS_NSTREAMS 4       // sub-batches in flight: latency-bound stages of one sub-batch
                             // (Huffman optimiser, scans, sparse sort rounds) overlap the
                             // bandwidth-bound stages of the others
#define CJS_SNAP_SLOTS 4096u

// BWTC: what the coder thread needs of one group of sub-batches (kept in the context: fresh 100 MB vectors per call would
// be page-faulted in by the D2H copies)
struct BwtcBlockJob { u32 len, pidx, nsym, ntri; u32 used[8]; size_t off; bool host; size_t soff; };   // host: K10 gave up (triples beyond its rows): model on the host
// triples of a group of blocks on the host: PINNED (hipHostMalloc, grow-only): the 350 MB of a 10^8-byte input took ~100 ms to
// arrive in pageable vectors, more than K1 + K2 together
struct PinnedU32 {
    u32* p = nullptr; size_t cap = 0;
    int reserve(size_t n) {
        if (n <= cap) return CJS_OK;
        if (p) (void)hipHostFree(p);
        p = nullptr; cap = 0;
        n += n / 8 + 1024;
        const hipError_t e = hipHostMalloc((void**)&p, n * sizeof(u32), hipHostMallocDefault);
        if (e != hipSuccess) { p = nullptr; return CJS_E_HIP - (int)e; }
        cap = n;
        return CJS_OK;
    }
    u32* data() { return p; }
    ~PinnedU32() { if (p) (void)hipHostFree(p); }
};
struct BwtcGroupJob { std::vector<BwtcBlockJob> blocks; PinnedU32 a, t; std::vector<u16> sym; bool busy = false; size_t nready = 0; };   // nready: leading blocks whose data has landed

// One persistent helper thread per extra stream: a sub-batch is issued from a host thread of its own (K1's read-backs block the thread that
// waits for them), and a thread made per call pays for its creation and its first HIP call (30-170 us before its first launch, seen on the
// kernel timeline) every time.  The thread starts with the first job posted; a helper that never gets one costs nothing.
struct CjsHelper {
    std::thread th;
    std::mutex mu;
    std::condition_variable cv;
    std::function<void()> job;
    bool has_job = false, busy = false, quit = false;
    void loop() {
        for (;;) {
            std::function<void()> j;
            {
                std::unique_lock<std::mutex> g(mu);
                cv.wait(g, [&]() { return has_job || quit; });
                if (!has_job) return;
                j = std::move(job);
                has_job = false;
            }
            j();
            {
                std::lock_guard<std::mutex> g(mu);
                busy = false;
            }
            cv.notify_all();
        }
    }
    void post(std::function<void()> j) {
        {
            std::lock_guard<std::mutex> g(mu);
            job = std::move(j);
            has_job = true;
            busy = true;
            if (!th.joinable()) th = std::thread([this]() { loop(); });
        }
        cv.notify_all();
    }
    void wait() {
        std::unique_lock<std::mutex> g(mu);
        cv.wait(g, [&]() { return !busy; });
    }
    void stop() {
        {
            std::lock_guard<std::mutex> g(mu);
            quit = true;
        }
        cv.notify_all();
        if (th.joinable()) th.join();
    }
};

struct cjs_ctx {
    int device = 0;
    hipStream_t stream = nullptr;      // stream 0: pre-pass, framing, timing events
    hipStream_t sub[CJS_NSTREAMS] = {};
    hipEvent_t evReady = nullptr;      // pre-pass + output zeroing done
    hipEvent_t evScan[CJS_NSTREAMS] = {};   // k5_blockscan of the last sub-batch issued on that stream
    hipEvent_t evDone[CJS_NSTREAMS] = {};   // everything issued on that stream
    u32* pin[CJS_NSTREAMS] = {};            // pinned host memory for K1's small read-backs of that stream's sub-batch (CJS_PIN_WORDS u32)
    CjsHelper helper[CJS_NSTREAMS];         // [i]: the host thread that issues stream i's sub-batches (i >= 1; stream 0's are issued by the caller)
    u32 nstreams = 0;          // streams in use (<= CJS_NSTREAMS; env CJS_STREAMS overrides)
    u32 batch_blocks = 0;      // blocks in flight over all streams
    u32 sub_blocks = 0;        // blocks per sub-batch, at most (what every stream's workspace is sized for)
    u32 share[CJS_NSTREAMS] = {};   // per mille of a batch that stream i's sub-batch takes (sums to 1000)
    void* ws[CJS_NSTREAMS] = {};    // block-pipeline workspaces (level-9 geometry)
    size_t ws_bytes = 0;
    StreamState* d_ss = nullptr;    // stream cursor + combined CRC, shared by all sub-batches
    void* k0ws = nullptr;           // K0 workspace (grows with the input length)
    size_t k0ws_bytes = 0;
    void* planws = nullptr;         // K0 workspace of cjs_bz2_plan: its own, so that a later compress call on this
    size_t planws_bytes = 0;        // context cannot re-carve or free what `plan` points into
    void* din = nullptr;  size_t din_bytes = 0;      // staging for the host-buffer entry point
    void* dout = nullptr; size_t dout_bytes = 0;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    float last_ms = 0.f;       // device time of the last compress call (HIP events on ctx->stream)
    u32 last_blocks = 0;
    // optional per-kernel timing of the dominant kernel (bench.py roofline leg)
    K1Prof prof = {};
    BatchGeom prof_g = {};     // geometry of the last sub-batch issued (where cjs_profile_read_class finds K1's counters)
    // state of cjs_bz2_plan
    K0Buf plan = {};
    int plan_level = 0;
    u32 plan_blocks = 0;
    float bwtc_times[5] = {};  // last cjs_bwtc_compress: K10 launch ms (first stream), ms until all triples were on the host, coder busy ms, total ms, encodeFreq calls
    hipEvent_t evK10[2] = {};
    hipEvent_t evB10[CJS_NSTREAMS] = {}, evB11[CJS_NSTREAMS] = {};   // cjs_bwtc_compress_batch: K10 of the last sub-batch on that workspace done; the K11 launch that read it done
    int bwtc_batch_syncs = 0;  // host<->device synchronisations the last cjs_bwtc_compress_batch* call made itself (K1's own read-backs not counted)
    int scan_level = 0;        // cjs_bz2_plan_scan ran for this level (0: no scan)
    uint64_t scan_total = 0;
    // decoder state (allocated by the first decompress call)
    DecState* dec = nullptr;
    float dec_ms = 0.f;
    std::vector<u8> bwtc_out;   // result of the last cjs_bwtc_decompress (or of a cjs_bwtc_decompress_batch* whose out_cap was too small)
    // cjs_bwtc_decompress_batch*: [0] the plan's documents and flags, [1] block rows, [2] the scratch (the blocks' last columns),
    // [3] rows of the batched inverse BWT, [4] its workspace - grow-only, kept across calls
    void* bd[5] = {}; size_t bd_bytes[5] = {};
    int bwtc_dec_batch_syncs = 0, bwtc_dec_batch_fallbacks = 0;   // of the last such call: its own host<->device waits; documents on the host path
    BwtcGroupJob bwtc_jobs[2];  // double buffer between the GPU stages and the coder thread of cjs_bwtc_compress
    // the overlapped host path (compress_overlapped): persistent helper threads, copy streams, per-slice events and cursors
    hipStream_t side = nullptr; // the block CRCs of every sub-batch (k0_crc) run here, next to K1
    hipEvent_t evPad[CJS_NSTREAMS] = {}, evCrc[CJS_NSTREAMS] = {};
    CjsHelper io[3];            // [0] uploader, [1] downloader, [2] issues the slices of stream 0 (the caller's thread plans)
    hipStream_t sIn = nullptr, sOut = nullptr;   // copy streams (non-blocking)
    std::vector<hipEvent_t> evPool;    // per slice: its k5_blockscan, everything of it
    u64* snapPin = nullptr;     // [CJS_SNAP_SLOTS] pinned: bit cursor behind every slice (written by k5_blockscan)
    void* k0sl = nullptr; size_t k0sl_bytes = 0;   // K0 workspaces of the slices of one call (one each: no reuse within a call)
    std::vector<std::pair<void*, size_t>> segpool;   // cjs_bz2_compress_multi: this device's segment buffers, one per wave of a call, grow-only and kept across calls
};

namespace cjs {
// bzip2's block capacity after RLE1 (lib/Bzip2.js:892-900), and the bytes of input behind a segment or slice that complete its last
// block: four blocks' worth of level * 100000
static inline u32 block_cap(int level) { return (u32)level * 100000u - 19u; }
static inline uint64_t plan_margin(u32 cap) { return (uint64_t)4 * (cap + 19u); }

// the Pipe of a stream-level call (k5_stream_begin / k5_stream_end): the context's cursor and the output buffer, nothing of a batch
static inline Pipe stream_pipe(const cjs_ctx* c, void* d_out, uint64_t out_cap) {
    Pipe P;
    memset(&P, 0, sizeof P);
    P.ss = c->d_ss;
    P.out = (u32*)d_out;
    P.outCapBytes = out_cap & ~(uint64_t)3;
    return P;
}
// a cjs_bz2_plan / _plan_scan result does not survive a call that re-carves or frees its workspace
static inline void invalidate_plan(cjs_ctx* c) { c->plan_level = 0; c->plan_blocks = 0; c->scan_level = 0; }

int grow(void** p, size_t* have, size_t need);
// BWTC decode of one stream (cjs_bwtc.hip): range decoder and models on the host, K6 per block
struct BwtcDecBufs { u8 *dT = nullptr, *dU = nullptr; void* ws = nullptr; };
int bwtc_dec_bufs_alloc(BwtcDecBufs& B);
void bwtc_dec_bufs_free(BwtcDecBufs& B);
int bwtc_decode_one(cjs_ctx* c, const BwtcDecBufs& B, const uint8_t* in, uint64_t in_len, int64_t* declared_size, std::vector<u8>& out);   // 0, -30, -31 or a call-level error; `out` empty unless 0
int issue_blocks(cjs_ctx* c, const K0Buf& K, u32 cap, u32 first, u32 count, void* d_out, uint64_t out_cap, const K5Docs* docs = nullptr);   // docs: a batch of documents (cjs_batch.hip)
int run_sub_batch(cjs_ctx* c, const K0Buf& K, const BatchGeom& g, u32 cap, u32 f, u32 nb, u32 si, void* d_out, uint64_t out_cap,
                  Pipe& P, u32 total_blocks);
// The stream cursor behind everything issued on `st`, waited for: the bits written so far, CJS_E_NOSPACE when the stream did not
// fit, or a HIP error.  pin (optional): pinned host memory the copy lands in; crc (optional): the combined CRC so far.
int64_t stream_bits(cjs_ctx* c, hipStream_t st, u32* pin = nullptr, u32* crc = nullptr);
// bytes of input per segment of the host paths: one batch of blocks; CJS_SEG_BYTES (tests) overrides; *from_env says that it did
uint64_t seg_bytes_for(const cjs_ctx* c, u32 cap, bool* from_env = nullptr);

int64_t compress_segmented(cjs_ctx* c, const uint8_t* in, uint64_t in_len, int level, uint8_t* out, uint64_t out_cap, uint64_t seg_bytes);
#ifndef CJS_CPU_DEBUG_BUILD
#define CJS_OV_NOT_STARTED (-1000)   // compress_overlapped: the input does not cut into slices - nothing was uploaded (internal: never returned by the ABI)
int64_t compress_overlapped(cjs_ctx* c, const uint8_t* in, uint64_t in_len, int level, uint8_t* out, uint64_t out_cap, u32 slice_blocks);
#endif
}
