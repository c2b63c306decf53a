/* compressjs_amd.h -- C ABI of libcompressjs_amd.so (MI355X-native bzip2 block pipeline).
 * (state: round 5; the full entry-point list with the reference binding of each is in INTEGRATION.md)
 */
#ifndef COMPRESSJS_AMD_H
#define COMPRESSJS_AMD_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* Opaque per-GPU context: one HIP stream + the HBM workspace for `batch_blocks` bzip2 blocks in
 * flight (about 31 B per block byte; 128 blocks of 900 kB = 3.6 GB).  Not thread safe; one
 * context per thread/GPU.  Returns NULL when no MI355X is visible (there is no CPU path). */
typedef struct cjs_ctx cjs_ctx;
cjs_ctx* cjs_create(int device, uint32_t batch_blocks);
void cjs_destroy(cjs_ctx* ctx);

/* Upper bound of the .bz2 size for in_len input bytes (any level). */
int64_t cjs_bz2_compress_bound(uint64_t in_len);

/* = Bzip2.compressFile(input, null, level)            (reference: lib/Bzip2.js:879-929)
 * Host buffers in, complete .bz2 stream out.  Returns the number of bytes written, or < 0:
 *   CJS_E_LEVEL (-20) 'Invalid block size multiplier' (lib/Bzip2.js:888-890),
 *   CJS_E_NOSPACE (-21) out_cap too small, CJS_E_ARG (-22), CJS_E_NOGPU (-23), -100-hipError_t. */
int64_t cjs_bz2_compress(cjs_ctx* ctx, const uint8_t* in, uint64_t in_len, int level, uint8_t* out,
                         uint64_t out_cap);
/* The same with input and output resident in HBM (device pointers, d_out 4-byte aligned). */
int64_t cjs_bz2_compress_device(cjs_ctx* ctx, const void* d_in, uint64_t in_len, int level, void* d_out,
                                uint64_t out_cap);
/* Batched form: `count` independent documents in, one complete .bz2 stream each out, in ONE trip through the kernels.
 * The reference has no batched entry; the contract is "equal to N single calls": stream d is bit-identical to what
 * Bzip2.compressFile (lib/Bzip2.js:879-929) gives for document d alone - its blocks are the ones readBlock (:636-667)
 * cuts from that document (a document start starts a fresh block and a fresh run), its stream header (:903-906),
 * combined CRC (:917) and trailer (:925-927) are its own.  Documents are packed back to back: document d is input bytes
 * [off[d], off[d+1]), off = count + 1 nondecreasing offsets; empty documents are allowed (a 14-byte stream); one level for
 * the call.  off[0] need not be 0: the bytes in front of it belong to no document (a run among them does not reach into
 * document 0).  Stream d is out[out_off[d] .. out_off[d+1]), out_off[0] = 0, byte-aligned and back to back without padding -
 * the whole output is also a valid multi-stream .bz2 file (cjs_bz2_decompress with multistream != 0 decodes it).
 * Both return the total number of bytes written (count == 0: 0), or CJS_E_LEVEL, CJS_E_ARG (null pointers, decreasing
 * offsets, d_out not 4-byte aligned, and - as in cjs_bz2_compress_device - a d_out of fewer than 64 bytes), CJS_E_NOSPACE
 * (out_cap too small for the streams; cjs_bz2_compress_batch_bound is enough),
 * CJS_E_NOGPU, -100-hipError_t.  The device form takes device pointers throughout (d_off and d_out_off included); the host
 * form uploads once and downloads once.  cjs_last_device_ms / cjs_last_block_count report the batch call. */
int64_t cjs_bz2_compress_batch_bound(uint64_t total_len, uint32_t count);
int64_t cjs_bz2_compress_batch_device(cjs_ctx* ctx, const void* d_in, const uint64_t* d_off, uint32_t count, int level,
                                      void* d_out, uint64_t out_cap, uint64_t* d_out_off);
int64_t cjs_bz2_compress_batch(cjs_ctx* ctx, const uint8_t* in, const uint64_t* off, uint32_t count, int level,
                               uint8_t* out, uint64_t out_cap, uint64_t* out_off);
/* = BWTC.compressFile(input, null, level) for level 6..9   (reference: lib/BWTC.js:12-139,
 * lib/Util.js:105-142).  GPU: BWT.bwtransform + MTF + RLE2 per 100000*level-byte block; host: the
 * adaptive Fenwick model + range coder (serial by construction: lib/RangeCoder.js, lib/FenwickModel.js).
 * declared_size = the size written into the header (input length, or -1 for streams of unknown
 * size, lib/Util.js:119-124).  Levels 1-5 use DefSumModel (lib/DefSumModel.js), 6-9 FenwickModel. */
int64_t cjs_bwtc_compress_bound(uint64_t in_len);
int64_t cjs_bwtc_compress(cjs_ctx* ctx, const uint8_t* in, uint64_t in_len, int level, uint8_t* out,
                          uint64_t out_cap, int64_t declared_size);
#define CJS_E_UNSUPPORTED (-24)
/* Phases of the last cjs_bwtc_compress (bench.py's BWTC line): out5[0] = ms of the first K10 launch (FenwickModel on the GPU),
 * [1] = ms until every (sy_f, lt_f, tot_f) triple was on the host, [2] = ms the serial range coder (lib/RangeCoder.js:79-89) was busy,
 * [3] = ms of the whole call, [4] = encodeFreq calls. */
int cjs_bwtc_last_times(cjs_ctx* ctx, float* out5);
/* Batched BWTC: `count` independent documents in, one complete BWTC stream each out, in one call.  The reference has no batched
 * entry; the contract is that of cjs_bz2_compress_batch, "equal to N single calls": stream d is bit-identical to
 * cjs_bwtc_compress(ctx, doc_d, len_d, level, ..., declared_size = len_d), i.e. to BWTC.compressFile(Buffer, null, level)
 * (lib/BWTC.js:12-139, lib/Util.js:105-142) on document d alone - its own magic, varint of len_d + 1 and coder start; its blocks
 * are the ceil(len_d / (level * 100000)) fixed-size pieces of that document (lib/BWTC.js:27), a document start starts a fresh block.
 * Documents are packed back to back: document d is input bytes [off[d], off[d+1]), off = count + 1 nondecreasing offsets (off[0]
 * need not be 0: the bytes in front of it belong to no document); empty documents are allowed and give the reference's stream for
 * empty input.  One level for the call; a level outside 1..9 means 9
 * (lib/BWTC.js:16-19).  Stream d is out[out_off[d] .. out_off[d+1]), out_off[0] = 0, back to back.
 * Both return the total number of bytes written (count == 0: 0), or CJS_E_ARG (null pointers, decreasing offsets), CJS_E_NOSPACE
 * (out_cap too small: out_off is written all the same; cjs_bwtc_compress_batch_bound = total_len + total_len / 4 + 4096 * count,
 * the sum of the single call's bounds, is always enough), CJS_E_NOGPU, -100-hipError_t, and CJS_E_UNSUPPORTED if a block's model
 * output did not fit the rows the block pipeline has for it (not seen; no bytes rather than wrong ones).  Every byte reported
 * has been written by the call.  The device form takes device pointers throughout; the host form uploads once and downloads once.
 * cjs_last_device_ms / cjs_last_block_count report the batch call.
 * Every level runs on the GPU: the model of every block (FenwickModel for levels 6-9: k10_bwtc_model.hip; DefSumModel, lib/BWTC.js:107,
 * for levels 1-5: k13_defsum_model.hip) and the range coder, one coder per document (k11_bwtc_coder.hip: lib/RangeCoder.js:27-140,
 * lib/BWTC.js:42-79,137-138, lib/NoModel.js, lib/LogDistanceModel.js).  The batch does not touch the host between upload and
 * download; the host waits for the device three times per call (the host form: four, with its download), whatever `count` and
 * `level` (cjs_dbg_bwtc_batch_syncs; the block sort's own small read-backs per sub-batch not counted). */
int64_t cjs_bwtc_compress_batch_bound(uint64_t total_len, uint32_t count);
int64_t cjs_bwtc_compress_batch_device(cjs_ctx* ctx, const void* d_in, const uint64_t* d_off, uint32_t count, int level,
                                       void* d_out, uint64_t out_cap, uint64_t* d_out_off);
int64_t cjs_bwtc_compress_batch(cjs_ctx* ctx, const uint8_t* in, const uint64_t* off, uint32_t count, int level,
                                uint8_t* out, uint64_t out_cap, uint64_t* out_off);
int cjs_dbg_bwtc_batch_syncs(cjs_ctx* ctx);      /* host<->device synchronisations the last batch call on ctx made itself */
/* (tests) floor(range / tot) as the device coder computes it (lib/RangeCoder.js:81): host pointers, n pairs, one tiny kernel */
int cjs_dbg_rc_div_device(const uint32_t* range, const uint32_t* tot, uint32_t n, uint32_t* out);
/* (tests) DefSumModel (lib/DefSumModel.js:39-111, BWTC levels 1-5) alone over nb rows of symbols: row b is sym[b * stride ..) with
 * nsym[b] <= stride symbols in [0, alpha[b]] (RUNA = 0, RUNB = 1, MTF index + 1; the model's size is alpha[b] + 1, alpha[b] <= 256).
 * Out, per row: ntri[b] triples, the arguments of the range coder's encodeFreq calls in order (encodeShift(sy, lt, 8) as
 * tot = 256): sylt[b * ostride + k] = sy_f | lt_f << 16, tot[b * ostride + k] = tot_f; ntri[b] = 0xFFFFFFFF if they did not fit
 * ostride (2 * nsym[b] always fit).  Host pointers.  on_host = 0: one launch of the device model (k13_defsum_model.hip);
 * on_host = 1: the host model the single call cjs_bwtc_compress uses, with a recorder in the coder's place. */
int32_t cjs_dbg_defsum_triples(const uint16_t* sym, const uint32_t* nsym, const uint32_t* alpha, uint32_t nb, uint32_t stride,
                               uint32_t* sylt, uint32_t* tot, uint32_t* ntri, uint32_t ostride, int on_host);

/* Sharded encoding for multi-GPU runs (blocks are independent once the RLE1 split is known):
 * cjs_bz2_plan   = the readBlock chain of lib/Bzip2.js:913-922 over the whole (device) input;
 *                  returns the number of blocks and keeps the split in the context, in a workspace of
 *                  its own: it stays valid across other calls on the context until the next
 *                  cjs_bz2_plan.  d_in must stay alive and unmodified until the last
 *                  cjs_bz2_encode_blocks that uses the plan (the plan points into it).
 * cjs_bz2_encode_blocks = compressBlock (lib/Bzip2.js:735-876) for blocks [first, first+count):
 *                  bare bit stream in d_seg starting at bit 0 (no "BZh" header, no trailer);
 *                  returns its length in BITS; *crc_fold = XOR_i rotl^(count-1-i)(blockCRC_i).
 *                  count is clamped to the blocks that exist (0xFFFFFFFF = "all remaining"). */
int64_t cjs_bz2_plan(cjs_ctx* ctx, const void* d_in, uint64_t in_len, int level);
/* first input byte, relative to the planned input, of block k of the current plan (k == block count: its length).  A
 * driver that holds only a slice of the stream plans from a block start, drops the last, incomplete block and tells the
 * next slice where that block started (compressjs_amd/dist.py, cjs_bz2_compress_multi). */
int64_t cjs_bz2_plan_block_start(cjs_ctx* ctx, uint32_t k);
/* Parallel plan of one slice of a longer stream (round 3; replaces the rank-to-rank chain of lib/Bzip2.js:913-922's serial
 * `do { readBlock } while` across GPUs).  With G(i) the RLE1 output length of stream bytes [0, i) under uncut runs, block k of
 * the stream starts where G reaches k * cap (cap = level * 100000 - 19, lib/Bzip2.js:636-667) unless that boundary falls
 * into a run of four or more equal bytes.  A rank that holds stream bytes [lo, lo + in_len) - its own slice [lo, lo + own_len)
 * and a margin of what follows - learns G(lo) from one all_gather of per-slice totals and boundary runs (compressjs_amd/dist.py):
 *   cjs_bz2_plan_scan   K0's scans over d_in; returns the input's own cost total;
 *   cjs_bz2_plan_cost   the input's own cost prefix at byte pos (pos = own_len: the slice's total);
 *   cjs_bz2_plan_phase  plans the blocks that START in [0, own_len), boundaries where the own prefix reaches phase + m * cap
 *                       (phase = (-(G(lo) + head-run correction)) mod cap; last != 0: no slice follows - d_in ends where the
 *                       stream ends, the final block may be short or absent, lib/Bzip2.js:916,922).  Returns their number - they are blocks 0 .. n-1
 *                       for cjs_bz2_encode_blocks - or CJS_E_SPEC when the slice cannot be planned on its own (a boundary in a
 *                       long run, a block longer than the margin): the caller falls back to cjs_bz2_plan on more of the stream.
 *   cjs_bz2_plan_chain  (round 6) the same plan as a link of a chain: t0 = the value the own prefix reaches at the slice's FIRST
 *                       block boundary (the slice before it hands it on; phase when nothing in front of the slice moved a
 *                       boundary).  A boundary inside a run of four or more equal bytes - ordinary text has them - restarts the
 *                       run in the new block (lib/Bzip2.js:636-667) and moves every later boundary by a few bytes: the slice goes
 *                       on serially from there instead of refusing, and *t_next = the target of the first boundary at or beyond
 *                       own_len carries the shift to the slices behind it (the next slice's t0 = *t_next + G(lo) - G(lo') under
 *                       its own origin, not below 0).  CJS_E_SPEC is left for what a slice cannot plan on its own (k0_phase_chain):
 *                       a block that starts in the slice and whose end the margin does not reach while last == 0; a run that
 *                       fills a whole block; a block start that cuts a run which reaches the end of d_in while last == 0 (where
 *                       the run ends is not known); more blocks than the plan has slots for (in_len / (cap / 2 + 1) + 2).
 *                       cjs_bz2_plan_phase returns it too when a boundary moved and last == 0 (it has no *t_next to carry
 *                       that). */
#define CJS_E_SPEC (-25)
int64_t cjs_bz2_plan_scan(cjs_ctx* ctx, const void* d_in, uint64_t in_len, int level);
int64_t cjs_bz2_plan_cost(cjs_ctx* ctx, uint64_t pos);
int64_t cjs_bz2_plan_phase(cjs_ctx* ctx, uint64_t own_len, uint64_t phase, int last);
int64_t cjs_bz2_plan_chain(cjs_ctx* ctx, uint64_t own_len, uint64_t t0, int last, uint64_t* t_next);
int64_t cjs_bz2_encode_blocks(cjs_ctx* ctx, uint32_t first, uint32_t count, void* d_seg,
                              uint64_t seg_cap, uint32_t* crc_fold, uint32_t* n_done);
/* Device time (HIP events on the context's stream) and block count of the last compress call. */
float cjs_last_device_ms(const cjs_ctx* ctx);
uint32_t cjs_last_block_count(const cjs_ctx* ctx);
void* cjs_stream(const cjs_ctx* ctx);   /* the hipStream_t the library launches on */
/* HIP-event timing of every launch of the suffix sort's main kernels (event pairs on the library's own streams), for
 * bench.py's roofline leg - which names the kernel with the largest total for the workload at hand.  Classes: 0 k1f_bsort
 * (in-LDS bucket sort of the sample-sort front end), 1 k1r_round (text refinement rounds), 2 k1d_build, 3 k1d_round,
 * 4 k1d_med, 5 k1d_large, 6 k1d_update (prefix-doubling stage), 7 k1f_task.  `elements`: rotations (classes 0, 2), list
 * entries walked (3, 6: read back from the last sub-batch's counters - exact for a one-stream pass over equal batches).
 * cjs_profile_enable(ctx, 1) clears the records; cjs_profile_read = class 0.  Test / bench instrumentation: no reference
 * counterpart. */
int32_t cjs_profile_enable(cjs_ctx* ctx, int on);
int32_t cjs_profile_read_class(cjs_ctx* ctx, uint32_t cls, float* total_ms, uint32_t* launches, uint64_t* elements);
int32_t cjs_profile_read(cjs_ctx* ctx, float* total_ms, uint32_t* launches, uint64_t* elements);

#define CJS_E_LEVEL (-20)
#define CJS_E_NOSPACE (-21)
#define CJS_E_ARG (-22)
#define CJS_E_NOGPU (-23)

/* The four BWT.* entry points below handle ONE block per call with n <= 2^22 - 1 = 4 194 303 bytes (CJS_E_ARG
 * above that: ranks are packed into 22 bits by the refinement kernels; bzip2 blocks are <= 900 000 and the
 * reference's own tests go up to test/sample5.ref = 2 130 640).  The reference has no such limit; js/index.js
 * hands larger n to the reference package when it is installed. */
/* = BWT.bwtransform2(T, U, n, 256) -> pidx            (reference: lib/BWT.js:372-417) */
int32_t cjs_bwt_cyclic(const uint8_t* T, uint8_t* U, uint32_t n, uint32_t* pidx);
/* = BWT.bwtransform(T, U, A, n, 256) -> pidx           (reference: lib/BWT.js:328-350, :153-192) */
int32_t cjs_bwt_linear(const uint8_t* T, uint8_t* U, uint32_t n, uint32_t* pidx);
/* = BWT.suffixsort(T, SA, n, 256)                      (reference: lib/BWT.js:305-321) */
int32_t cjs_suffixsort(const uint8_t* T, int32_t* SA, uint32_t n);
/* = BWT.unbwtransform(T, U, LF, n, pidx)                (reference: lib/BWT.js:352-363); list ranking */
int32_t cjs_unbwt_linear(const uint8_t* T, uint8_t* U, uint32_t n, uint32_t pidx);
/* The same for `count` blocks in one call (host pointers): block k = T[off[k] .. off[k+1]) with primary index pidx[k], its text
 * to U[off[k] .. off[k+1]) (off[0] need not be 0; nothing in front of U[off[0]] is written); every block is what cjs_unbwt_linear
 * gives for it alone.  One sequence of launches per group of
 * blocks (the list-ranking workspace of a group, ~20 bytes per byte, stays inside 512 MiB), no host wait in between; a (T, pidx)
 * pair that is no BWT gets the reference's literal walk.  CJS_E_ARG: pidx[k] > its block's length, decreasing offsets. */
int32_t cjs_unbwt_linear_batch(const uint8_t* T, const uint64_t* off, const uint32_t* pidx, uint32_t count, uint8_t* U);

/* = require('compressjs/lib/HuffmanAllocator').allocateHuffmanCodeLengths(array, maxLength)
 *   (reference: lib/HuffmanAllocator.js:199-222, exercised by test/huffman.js): in place, ascending
 *   weights in, code lengths out.  64-bit cells carry any integer weight a JS caller can pass.
 *   The batch form runs `count` independent arrays, array k = arr[off[k] .. off[k+1]). */
int32_t cjs_huff_lengths(int64_t* arr, uint32_t n, uint32_t max_len);
int32_t cjs_huff_lengths_batch(int64_t* arr, const uint32_t* off, uint32_t count, uint32_t max_len);
/* cjs_bwt_cyclic for nb independent blocks laid out at a fixed pitch `cap` (host pointers) */
int32_t cjs_bwt_cyclic_batch(const uint8_t* T, const uint32_t* nlen, uint32_t nb, uint32_t cap,
                             uint8_t* U, uint32_t* pidx);

/* ---- debug/test entry points (not part of the drop-in surface) ------------------------------ */
typedef struct cjs_dbg_stage_out {   /* every pointer may be NULL; pitches in elements */
    uint8_t* U;          /* [nb][cap]        BWT output                           */
    uint32_t* pidx;      /* [nb]                                                   */
    uint16_t* A;         /* [nb][cap+1]      MTF/RLE2 symbols incl. EOB            */
    uint32_t* pos;       /* [nb]                                                   */
    uint32_t* alpha;     /* [nb]             alphabetSize                          */
    uint32_t* freq;      /* [nb][258]                                              */
    uint32_t* used;      /* [nb][8]          256-bit used-symbol set               */
    uint8_t* sel;        /* [nb][(cap+1)/50+2]                                     */
    uint8_t* lens;       /* [nb][6][258]                                           */
    uint32_t* ngroups;   /* [nb]                                                   */
    uint32_t* nsel;      /* [nb]                                                   */
    uint64_t* bitlen;    /* [nb]                                                   */
    const uint32_t* crc_in; /* [nb] block CRCs to put in the headers (K0 is bypassed here) */
    int32_t level;       /* level digit for the stream header                      */
    uint8_t* stream;     /* whole .bz2 stream of the batch (header, blocks, trailer) */
    uint64_t stream_cap;
    uint64_t stream_bytes; /* out */
} cjs_dbg_stage_out;
int32_t cjs_dbg_bwt_batch_time(const uint8_t* T, const uint32_t* nlen, uint32_t nb, uint32_t cap,
                               uint8_t* U, uint32_t* pidx, int reps, float* ms);
int cjs_dbg_k1_sparse_rounds(void);   /* rounds of the last K1 run that used the sparse phase */
int cjs_dbg_k1_rounds(void);
uint32_t cjs_dbg_rc_div(uint32_t range, uint32_t tot);   /* bwtc_host.hip: the range coder's range / tot by reciprocal (boundary test in tests/test_host_api.py) */
int cjs_dbg_multi_replans(void);      /* segments of cjs_bz2_compress_multi planned a second time: the chain carried a boundary shift to them (round 6: such calls used to take the replicated plan) */
int cjs_dbg_multi_fallbacks(void);    /* calls of cjs_bz2_compress_multi that took the REPLICATED plan (a segment that cannot be planned on its own: every device plans the whole input, encodes its share) */
int cjs_dbg_multi_mallocs(void);      /* hipMalloc calls cjs_bz2_compress_multi has made for its per-device segment buffers (grow-only pools: none after warm-up) */
int cjs_dbg_k1_periodic_blocks(void); /* k1_period.hip, last K1 run (counted under CJS_K1_TRACE only): blocks with a period <= 64 (closed form) | blocks sorted through a reduced block << 16 */
int32_t cjs_dbg_block_stages(const uint8_t* T, const uint32_t* nlen, uint32_t nb, uint32_t cap,
                             int upto, cjs_dbg_stage_out* out);

/* ---- decoder --------------------------------------------------------
 * = Bzip2.decompressFile(input, output, multistream) = Bunzip.decode   (reference: lib/Bzip2.js:454-481,
 *   _start_bunzip :137-152, _get_next_block :153-398, _read_bunzip :405-448).
 * Returns the decoded size or a negative code: the reference's own Err values -2 NOT_BZIP_DATA,
 * -5 DATA_ERROR, -7 OBSOLETE_INPUT (lib/Bzip2.js:62-72; which one, and when, follows the reference's
 * sequential order), or -21 when `out_cap` is too small (the result stays in HBM: cjs_bz2_last_size /
 * cjs_bz2_fetch), -22/-23/-100-e as above.  cjs_bz2_last_detail gives the optDetail of the error. */
int64_t cjs_bz2_decompress(cjs_ctx* ctx, const uint8_t* in, uint64_t in_len, uint8_t* out, uint64_t out_cap,
                           int multistream);
/* the same with the stream and the output resident in HBM */
int64_t cjs_bz2_decompress_device(cjs_ctx* ctx, const uint8_t* d_in, uint64_t in_len, uint8_t* d_out,
                                  uint64_t out_cap, int multistream);
/* = Bzip2.decompressBlock(input, bitPos, output) = Bunzip.decodeBlock   (reference: lib/Bzip2.js:482-503) */
int64_t cjs_bz2_decompress_block(cjs_ctx* ctx, const uint8_t* in, uint64_t in_len, uint64_t bitpos, uint8_t* out,
                                 uint64_t out_cap);
/* = Bzip2.table(input, callback, multistream)   (reference: lib/Bzip2.js:508-548): positions[i] (bits)
 *   and sizes[i] (decoded bytes) of block i, at most `cap` of them; returns the number of blocks */
int64_t cjs_bz2_table(cjs_ctx* ctx, const uint8_t* in, uint64_t in_len, int multistream, uint64_t* positions,
                      uint64_t* sizes, uint32_t cap);
int64_t cjs_bz2_last_size(cjs_ctx* ctx);
int64_t cjs_bz2_fetch(cjs_ctx* ctx, uint8_t* out, uint64_t out_cap);
int32_t cjs_bz2_last_detail(cjs_ctx* ctx, uint32_t* crc_got, uint32_t* crc_expected);
float cjs_bz2_last_decode_ms(cjs_ctx* ctx);

/* Batched form: `count` independent .bz2 documents in, the decoded bytes of each out, in ONE trip through the kernels.  The
 * reference has no batched entry; the contract is "equal to N single calls": result d is what Bzip2.decompressFile(document d, null,
 * multistream) (lib/Bzip2.js:454-481) gives for that document ALONE - bits behind its end read as zeros (lib/BitStream.js:84), never
 * as its neighbour's bytes - either the decoded bytes or the reference's Err code in status[d] (0, or -2 / -5 / -7 as above; which
 * one, and when, follows the reference's sequential order inside the document: a bad block CRC in block 1 wins over a structural
 * error behind block 2).  detail[3d .. 3d+2] = optDetail number, CRC got, CRC expected, as cjs_bz2_last_detail reports them
 * (`detail` may be NULL).  Document d is in[off[d] .. off[d+1]), off = count + 1 nondecreasing offsets, any byte alignment (off[0]
 * need not be 0), empty documents allowed (status -2, detail 1).  Results lie back to back: result d is
 * out[out_off[d] .. out_off[d+1]), out_off[0] = 0;
 * a failed document contributes no bytes and changes nothing for any other document.
 * Both return the total number of decoded bytes (>= 0 even when documents failed; count == 0: 0).  Negative returns are call-level
 * only: CJS_E_ARG (null ctx / off / out_off / status, decreasing offsets, null `in` with a non-empty batch), CJS_E_NOGPU,
 * -100-hipError_t, CJS_E_UNSUPPORTED (candidate cap), and CJS_E_NOSPACE when out_cap is too small - out_off / status / detail have
 * been written then and the result stays in HBM (cjs_bz2_last_size / cjs_bz2_fetch).  The device form takes device pointers
 * throughout.  cjs_bz2_last_decode_ms reports the batch call; cjs_bz2_last_detail is the single call's and reads 0 after a batch. */
int64_t cjs_bz2_decompress_batch(cjs_ctx* ctx, const uint8_t* in, const uint64_t* off, uint32_t count, int multistream,
                                 uint8_t* out, uint64_t out_cap, uint64_t* out_off, int32_t* status, uint32_t* detail);
int64_t cjs_bz2_decompress_batch_device(cjs_ctx* ctx, const uint8_t* d_in, const uint64_t* d_off, uint32_t count, int multistream,
                                        uint8_t* d_out, uint64_t out_cap, uint64_t* d_out_off, int32_t* d_status, uint32_t* d_detail);
/* Batched block fetch: `count` chosen blocks of ONE stream in one call - index a .bz2 once with cjs_bz2_table, then fetch many blocks
 * at random.  The reference has no batched entry; the contract is "equal to N single calls": result k is what
 * Bzip2.decompressBlock(stream, bitpos[k]) = Bunzip.decodeBlock (lib/Bzip2.js:482-503) gives for that position ALONE.  The 4-byte
 * stream header is checked first, as `new Bunzip` does (_start_bunzip, :137-152): a bad or missing one gives EVERY request status -2
 * with detail 1 ('bad magic') or 2 ('level out of range') - not a call-level error.  Otherwise status[k] is 0 with the block's bytes
 * where the 48 bits at bitpos[k] are the block magic, 0 with no bytes at the end-of-stream magic (_get_next_block, :157-159), -2 with
 * detail 0 anywhere else (:160-161), the reference's block errors in its order (-7; -5 detail 3 'initial position out of bounds'
 * :177-178; -5 detail 0), or -5 detail 4 on a block-CRC mismatch (:437-445) with CRC got / expected in detail[3k+1] / detail[3k+2]
 * (`detail` may be NULL).  Positions are bit positions, in any order, duplicates allowed, any 64-bit value: bits behind the stream's end
 * read as zeros (lib/BitStream.js:84), so a position at or behind 8 * in_len is -2.  Results lie back to back in request order: result
 * k is out[out_off[k] .. out_off[k+1]), out_off has count + 1 entries, out_off[0] = 0; a failed request contributes no bytes and changes
 * nothing for any other request.
 * Both return the total number of decoded bytes (count == 0: 0).  Negative returns are call-level only: CJS_E_ARG (null ctx / bitpos /
 * out_off / status, null `in` with in_len > 0), CJS_E_NOGPU, -100-hipError_t, CJS_E_UNSUPPORTED (more than 2^27 requests), and
 * CJS_E_NOSPACE when out_cap is too small - out_off / status / detail have been written then and the bytes stay in HBM
 * (cjs_bz2_last_size / cjs_bz2_fetch).  The device form takes device pointers throughout (d_bitpos included).  The stream is uploaded
 * once and the requests are classified on the GPU; the number of host<->device waits does not depend on count while the block requests
 * fit one slot batch.  cjs_bz2_last_decode_ms reports the call; cjs_bz2_last_detail reads 0 after it. */
int64_t cjs_bz2_decompress_blocks(cjs_ctx* ctx, const uint8_t* in, uint64_t in_len, const uint64_t* bitpos, uint32_t count,
                                  uint8_t* out, uint64_t out_cap, uint64_t* out_off, int32_t* status, uint32_t* detail);
int64_t cjs_bz2_decompress_blocks_device(cjs_ctx* ctx, const uint8_t* d_in, uint64_t in_len, const uint64_t* d_bitpos, uint32_t count,
                                         uint8_t* d_out, uint64_t out_cap, uint64_t* d_out_off, int32_t* d_status, uint32_t* d_detail);
int cjs_dbg_dec_syncs(void);          /* host<->device synchronisations (stream syncs, synchronous copies) of the last decode call of the process */

/* = BWTC.decompressFile(input, output)   (reference: lib/BWTC.js:141-233 via Util.decompressFileHelper
 *   lib/Util.js:143-166; decoder sides of lib/RangeCoder.js:146-226, lib/FenwickModel.js:88-136,
 *   lib/LogDistanceModel.js:37-44, lib/NoModel.js:22-29).  Range decoder on the host (serial by
 *   construction), BWT.unbwtransform of every block on the GPU.  Returns the decoded size, -30 'Bad
 *   magic', -31 corrupt/truncated stream (undefined behaviour in the reference),
 *   -21 when out_cap is too small (then cjs_bwtc_last_size / cjs_bwtc_fetch).  *declared_size gets the
 *   size recorded in the header (-1: unknown). */
int64_t cjs_bwtc_decompress(cjs_ctx* ctx, const uint8_t* in, uint64_t in_len, uint8_t* out, uint64_t out_cap,
                            int64_t* declared_size);
int64_t cjs_bwtc_last_size(cjs_ctx* ctx);
int64_t cjs_bwtc_fetch(cjs_ctx* ctx, uint8_t* out, uint64_t out_cap);
/* Batched BWTC decode: `count` independent BWTC streams in, the decoded documents back to back out, in one call.  The reference has
 * no batched entry; the contract is that of cjs_bz2_decompress_batch and cjs_bwtc_compress_batch, "equal to N single calls":
 * result d is what cjs_bwtc_decompress(ctx, stream_d, len_d, ...) gives for document d alone, with bwtc_decode's order of checks -
 * either the decoded bytes (status[d] = 0), or status[d] = -30 (bad magic) / -31 (corrupt or truncated) and no bytes.  A damaged
 * stream that the single call decodes without error into other bytes comes out as those same bytes.  declared[d] (may be NULL)
 * is the size recorded in the header where the single call reports it, else -1 (unknown; also: bad magic, a size cut short).
 * Document d is in[off[d] .. off[d+1]), off = count + 1 nondecreasing offsets, at any byte alignment (off[0] need not be 0); empty
 * documents are allowed (-30).  A read behind a document's end is end-of-input for that document, never its neighbour's bytes.
 * Result d is
 * out[out_off[d] .. out_off[d+1]), out_off[0] = 0, back to back; a failed document contributes nothing and changes nothing for
 * any other.  Both forms return the total of decoded bytes (>= 0 also when documents failed; count == 0: 0).  Negative returns
 * are call-level only: CJS_E_ARG (null ctx / off / out_off / status, decreasing offsets, null `in` with bytes to read),
 * CJS_E_NOGPU, -100-hipError_t, and CJS_E_NOSPACE when out_cap is too small (a null `out` counts as out_cap = 0) - then out_off,
 * status and declared are complete all the same and the result is retained for cjs_bwtc_last_size / cjs_bwtc_fetch, which
 * otherwise keep serving the single call as before.  The device form takes device pointers throughout.
 * The fast path - FenwickModel streams (levels 6-9) with their size declared, as the encoder makes them: a plan kernel reads the
 * headers, one range decoder per document runs on the GPU, one wave each (k12_bwtc_decoder.hip: lib/RangeCoder.js:146-226,
 * lib/FenwickModel.js:88-172, lib/BWTC.js:172-223), the inverse BWT of all blocks runs batched (k6_unbwt_batch) and writes every
 * block to its final place.  The host waits for the device three times per call, whatever `count` (cjs_dbg_bwtc_dec_batch_syncs):
 * for the plan's totals, for the documents' statuses and block rows (out_off is their scan, made on the host), and at the end.
 * The host path - DefSumModel streams (levels 1-5), no size declared, a document that holds more bytes or blocks than its header
 * declares, a declared size beyond what is left of the call's scratch budget (512 MiB; the memory a call takes is bounded by it,
 * never by what a header claims): decoded by the single call's machinery, document after document, same result, no speed claim
 * (cjs_dbg_bwtc_dec_batch_fallbacks counts them; they add their own waits).  The device form stages these through the host.
 * The _ex forms take a `flags` word; flags = 0 is the call above, bit for bit, and an unknown bit is CJS_E_ARG.  With
 * CJS_BWTC_DEC_DEFSUM_DEVICE a DefSumModel stream (levels 1-5) that declares its size takes the fast path too: its range decoder
 * runs on the GPU, one wave per document (k14_defsum_decoder.hip: lib/DefSumModel.js:11-131 on K12's decoder), between the same
 * three waits.  Every other reason for the host path stays, the contract is the same: result d is cjs_bwtc_decompress's for stream
 * d alone, and the two counters report the _ex calls the same way. */
#define CJS_BWTC_DEC_DEFSUM_DEVICE 1u   /* DefSumModel streams (levels 1-5) with a declared size: decoded on the GPU */
int64_t cjs_bwtc_decompress_batch_ex(cjs_ctx* ctx, const uint8_t* in, const uint64_t* off, uint32_t count, uint8_t* out,
                                     uint64_t out_cap, uint64_t* out_off, int32_t* status, int64_t* declared, uint32_t flags);
int64_t cjs_bwtc_decompress_batch_device_ex(cjs_ctx* ctx, const void* d_in, const uint64_t* d_off, uint32_t count, void* d_out,
                                            uint64_t out_cap, uint64_t* d_out_off, int32_t* d_status, int64_t* d_declared, uint32_t flags);
int64_t cjs_bwtc_decompress_batch(cjs_ctx* ctx, const uint8_t* in, const uint64_t* off, uint32_t count, uint8_t* out,
                                  uint64_t out_cap, uint64_t* out_off, int32_t* status, int64_t* declared);
int64_t cjs_bwtc_decompress_batch_device(cjs_ctx* ctx, const void* d_in, const uint64_t* d_off, uint32_t count, void* d_out,
                                         uint64_t out_cap, uint64_t* d_out_off, int32_t* d_status, int64_t* d_declared);
int cjs_dbg_bwtc_dec_batch_syncs(cjs_ctx* ctx);      /* host<->device waits the last such call on ctx made itself */
int cjs_dbg_bwtc_dec_batch_fallbacks(cjs_ctx* ctx);  /* documents of the last such call that took the host path */
int cjs_dbg_k6_groups(void);          /* groups of blocks the last batched inverse BWT of the process ran (cjs_unbwt_linear_batch, cjs_bwtc_decompress_batch*): a new group after 65 535 blocks or 512 MiB of list-ranking workspace */

/* Workload helper (not a compression entry point): bytes [first, first + n) of LCG(N, seed) - SURVEY.md 8(c), BASELINE.json
 * configs[3] "random printable ASCII" - written straight into HBM, so that every GPU of a multi-GPU run fills its own slice. */
int32_t cjs_lcg_ascii_device(cjs_ctx* ctx, uint8_t* d_out, uint64_t n, uint32_t seed, uint64_t first);
/* HIP devices visible to the process (0: none; the product has no CPU path). */
int32_t cjs_device_count(void);
/* = Bzip2.compressFile over SEVERAL GPUs of one node from one process (the N-API addon's path to N
 * devices, the reference's single entry point lib/Bzip2.js:879 staying the only call): ctxs[i] = contexts created
 * on different devices (the same device twice is allowed: tests).  The input is cut into segments of about one batch of
 * blocks, segment k is uploaded to, planned and encoded on device k mod n, the segments' bit streams are shifted to
 * their offsets on the devices and copied side by side into `out` (parallel D2H); same bytes as cjs_bz2_compress. */
int64_t cjs_bz2_compress_multi(cjs_ctx** ctxs, uint32_t n, const uint8_t* in, uint64_t in_len, int level,
                               uint8_t* out, uint64_t out_cap);

/* multi-GPU seam helper: d_out[0 .. nbytes] = d_in[0 .. nbytes) shifted right by s (0..7) bits (MSB first).
 * Used when a rank's bit-0-aligned segment (cjs_bz2_encode_blocks) is placed at its offset in the stream. */
int32_t cjs_shift_bits(cjs_ctx* ctx, const uint8_t* d_in, uint64_t nbytes, uint32_t s, uint8_t* d_out);

#ifdef __cplusplus
}
#endif
#endif
