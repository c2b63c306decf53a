// Device-side view of one batch of bzip2 blocks moving through K0..K5.
#pragma once
#include "cjs_common.h"
#include "devutil.h"
#include "k1_bwt.h"

#define K2_SEG 1024          // run heads per MTF segment (one wave)
#define K2_FREQ_PITCH 260    // u32 per block in freq[]
#define CJS_MAX_SYMS 258     // lib/Bzip2.js:41
#define CJS_MAX_GROUPS 6     // lib/Bzip2.js:45
#define CJS_GROUP 50         // lib/Bzip2.js:46
#define CJS_MAX_BITS 20      // lib/Bzip2.js:40
#define CJS_LEN_PITCH 264    // bytes per table in lens[], u32 per table in codes[]

#define K5_NONE (-0x40000000)
#define K5_TGROUPS 80u       // groups of 50 symbols per K5 tile: a tile's code bits are a sum of the optimiser's group costs
#define K5_TILE (K5_TGROUPS * CJS_GROUP)
#define K5_TILES(g) ((g).stride / K5_TILE + 2u)              // >= ceil((symbols of a block + EOB) / K5_TILE)
#define K5_HDR_WORDS 6144     // >= worst-case header: 18001 selectors x 6 bits + 6 tables x 10067 bits

struct StreamState {
    u64 bits;          // bits written so far (next block starts here)
    u32 crc;           // combined CRC so far (lib/Bzip2.js:917)
    u32 overflow;      // set when the stream would not fit outCapBytes
};

struct Pipe {
    BatchGeom g;
    u32 segs;          // stride / K2_SEG
    // ---- block text (K0 output / K1 input)
    u8* T;             // [nb][tstride]  T_ext
    u32* nlen;         // [nb]
    u32* crc;          // [nb]           block CRCs
    // ---- K1
    K1Buf k1;
    u8* U;             // [nb][stride]
    u32* pidx;         // [nb]
    // ---- K2
    u32* used;         // [nb][8]        256-bit used-symbol set
    u32* alpha;        // [nb]           alphabetSize
    u32* nruns;        // [nb]
    u32* tileCnt;      // [nb][rtiles]
    u32* symCnt;       // [nb][rtiles]
    u8* RHsym;         // [nb][stride]
    u32* RHpos;        // [nb][stride+1]
    int* Ltab;         // [nb][segs][256]
    u8* J;             // [nb][stride]
    u16* A;            // [nb][stride]   MTF/RLE2 symbols incl. EOB
    u32* pos;          // [nb]           number of symbols in A
    u32* freq;         // [nb][K2_FREQ_PITCH]
    // ---- K3/K4
    u8* sel;           // [nb][selPitch] selectors
    u32 selPitch;
    u8* lens;          // [nb][6][CJS_LEN_PITCH]
    u32* codes;        // [nb][6][CJS_LEN_PITCH]
    u32* ngroups;      // [nb]
    u32* nsel;         // [nb]
    u16* selCost;      // [nb][selPitch] best cost of every 50-symbol group (optimiser scratch)
    u32* fr2;          // [nb][2][6][CJS_LEN_PITCH] frequency rows of the optimiser's tables, two sets used alternately
    // ---- K5
    u32* hdr;          // [nb][K5_HDR_WORDS] block header bits (magic .. code-length tables)
    u32* hbits;        // [nb]           header length in bits
    u32* tileBits;     // [nb][K5_TILES] code bits per tile of K5_TILE symbols -> exclusive offsets
    u64* bitlen;       // [nb]           bits of the encoded block
    u64* bitoff;       // [nb]           absolute bit offset of the block in the stream
    StreamState* ss;   // running stream state (bit cursor, combined CRC), device resident
    u32* out;          // the .bz2 stream being assembled (byte order = memory order)
    u64 outCapBytes;
    u64* snap;         // optional (pinned host memory): k5_blockscan leaves the bit cursor behind this batch's blocks here - everything before it is final once the batch is packed
};

// K0 (whole-input pre-pass) ----------------------------------------------------------------------
struct K0Buf {
    const u8* in;      // input bytes (device)
    u64 in_len;
    u64 ntiles;        // 4096-byte tiles
    u64 nchunks;       // scan chunks of 1024 tiles
    u32 maxBlocks;
    u64* tileA;        // [ntiles+2] last run boundary (+1) before the tile   (exclusive max-scan)
    u64* tileB;        // [ntiles+2] last run boundary (+1) inside the tile
    u64* tileC;        // [ntiles+2] C(4096 t): RLE1 output bytes before the tile with uncut runs; [ntiles] = total
    u64* chunk;        // [nchunks+1] scan scratch
    u64* blkStart;     // [maxBlocks] first input byte of block k
    u64* blkEnd;       // [maxBlocks] one past its last input byte
    u64* blkAdj;       // [maxBlocks] output position of input byte i >= blkRe is C(i) - blkAdj
    u64* blkRe;        // [maxBlocks] end of the run the block start cuts (== blkStart if none)
    u32* blkN;         // [maxBlocks] block length after RLE1
    u32* nBlocks;      // [1]
    u64* specEnd;      // [maxBlocks+2] speculative chain: boundary j = min{ i : C(i) >= j*cap }
    u64* specC;        // [maxBlocks+2] C at that boundary
    u64* specBad;      // [1] first boundary where the speculation does not hold (UINT64_MAX: none)
};
size_t k0_bytes(u64 in_len, u32 cap);
void k0_carve(K0Buf& K, const u8* d_in, u64 in_len, u32 cap, void* ws);
int k0_prepass(K0Buf K, u32 cap, hipStream_t stream);
// multi-GPU parallel plan (see k0_rle1.hip): scans only; C at a position (-> K.specC[0]); the blocks that start in [0, own_len)
#define K0_PHASE_FAIL 0xFFFFFFFFu
int k0_scans(K0Buf K, hipStream_t stream);
int k0_eval(K0Buf K, u64 pos, hipStream_t stream);
int k0_phase_plan(K0Buf K, u32 cap, u64 t0, u64 own_len, u32 last, u64 total, hipStream_t stream);   // t0: target of the slice's first boundary (round 6: carried from slice to slice; *K.nBlocks, ((u64*)K.nBlocks)[1] = blocks, the next slice's target)

int k6_unbwt_linear(const u8* dT, u8* dU, u32 n, u32 pidx, void* ws, hipStream_t stream);
// the same over many blocks in one sequence of launches (no host wait); block k = one K6Blk row
struct K6Blk {
    u64 tAt, uAt;      // the block's BWT string at T + tAt, its text at U + uAt (the final place)
    u64 wsAt;          // its slice of the workspace, in u32 (k6_ws_words(n) of them)
    u32 n, pidx;       // n >= 1, pidx <= n
};
#define K6_GROUP_MAX 65535u   // blocks per call (the grid's y extent)
size_t k6_ws_words(u32 n);
int k6_unbwt_batch(const K6Blk* d_B, u32 nblk, u32 max_n, const u8* dT, u8* dU, void* ws, hipStream_t stream);
int k2_run(Pipe P, u32 max_n, hipStream_t stream);
// BWTC levels 6..9: FenwickModel of every block on the GPU -> (sy_f | lt_f << 16, tot_f) per encodeFreq call, [nb][stride] each
int k10_model_run(Pipe P, u32* sylt, u32* tot, u32* ntri, u32 ostride, u32 ocap, hipStream_t stream);
// BWTC levels 1..5: DefSumModel of every block on the GPU (k13_defsum_model.hip), K10's inputs and K10's output layout; a symbol
// gives one or two triples, so rows of 2 x stride always hold a block
int k13_defsum_run(Pipe P, u32* sylt, u32* tot, u32* ntri, u32 ostride, u32 ocap, hipStream_t stream);
// Batched BWTC (cjs_bwtc_compress_batch*, k11_bwtc_coder.hip): document d of the batch is input bytes [off[d], off[d+1]) and becomes a
// BWTC stream of its own, coded by a range coder of its own on the device.
struct K11State {      // RangeCoder (lib/RangeCoder.js:27-34) of one document between two launches, and its write cursor
    u32 low, range, buffer, help, bytecount;
    u32 acc;           // the bytes of the stream's last, incomplete dword
    u64 n;             // bytes of the stream so far (beyond the document's bound: counted, not stored)
};
#define K11_F_NBLOCKS 0      // flags[]: blocks of the batch
#define K11_F_MAXLEN 1       //          the longest block
#define K11_F_BAD 2          //          the plan needs more blocks than it has slots for
#define K11_F_K10 3          //          K10 gave up on a block (its triples did not fit the rows)
#define K11_F_SCRATCH 4      //          a stream outgrew its document's bound
#define K11_F_NOSPACE 5      //          the streams do not fit out_cap
#define K11_F_WORDS 8
struct K11Plan {
    const u8* in;      // the documents, back to back (device)
    const u64* off;    // [count+1] (device)
    u32 count;
    u32 bs;            // level * 100000: bytes per block (lib/BWTC.js:27)
    u32 level;
    u32 maxBlocks;
    u32* docFirst;     // [count+1] first block of document d; [count] = blocks of the batch
    u64* docScr;       // [count+1] byte offset of document d's stream in scr: exclusive scan of its bound (rounded up to a dword)
    u32* blkDoc;       // [maxBlocks] document of block k
    K11State* st;      // [count]
    u32* scr;          // the streams before they are moved to their places
    u32* flags;        // [K11_F_WORDS]
};
struct K11Sub {        // what a sub-batch's K1 / K2 / K10 left for its blocks [first, first + nb) of the batch
    u32 first, nb;
    const u32 *nlen, *pidx, *used, *ntri, *sylt, *tot;
    u32 ostride;       // u32 per row of sylt / tot (= K10's capacity: the batch path gives it its full rows)
};
__host__ __device__ static inline u64 k11_bound(u64 len) { return len + len / 4 + 4096; }                 // = bwtc_bound
size_t k11_plan_bytes(u64 in_len, u32 count, u32 bs);
void k11_plan_carve(K11Plan& Q, const u8* d_in, const u64* d_off, u64 in_len, u32 count, int level, void* ws);
int k11_plan_run(K11Plan Q, hipStream_t stream);                                      // docFirst, docScr, blkDoc, flags; the streams of the empty documents
int k11_gather_run(K11Plan Q, Pipe P, u32 first, hipStream_t stream);                 // rows of P.T and P.nlen for blocks [first, first + P.g.nb)
int k11_code_run(K11Plan Q, K11Sub S, hipStream_t stream);
int k11_finish_run(K11Plan Q, u8* d_out, u64 out_cap, u64* d_out_off, u32 split, hipStream_t stream);   // out_off, then the streams to their places
// Batched BWTC decode (cjs_bwtc_decompress_batch*, k12_bwtc_decoder.hip, k14_defsum_decoder.hip): document d is a BWTC stream of its own, decoded by a
// range decoder of its own on the device, ONE WAVE per document.
#define K12_HOST 1           // K12Doc.status: not the fast path - the host decodes this document (cjs_bwtc_decompress's machinery)
#define K12_F_SCR 0          // flags[] (u64): bytes of scratch the admitted documents need
#define K12_F_BLK 1          //                their block rows
#define K12_F_BAD 2          //                the offsets decrease somewhere, or `in` is null with bytes to read
#define K12_F_TOTAL 3        //                off[count]
#define K12_F_NFEN 4         //                admitted documents of levels 6-9 (FenwickModel: k12_decode)
#define K12_F_NDEF 5         //                admitted documents of levels 1-5 (DefSumModel: k14_decode)
#define K12_F_WORDS 6
#define K12_OPT_DEFSUM 1u    // K12Plan.opt (= CJS_BWTC_DEC_DEFSUM_DEVICE): DefSumModel streams with a declared size are admitted
struct K12Doc {
    u64 scrAt;         // the document's bytes in the scratch (dword aligned)
    long long declared;   // the size its header records (-1: none, or the header was not read that far)
    u32 scrLen;        // = declared: the scratch it gets
    u32 blk0, blkMax;  // its rows; at most ceil(declared / (level * 100000)) blocks
    int status;        // 0, -30, -31 or K12_HOST
    u32 nblk, size;    // (K12) blocks decoded, bytes decoded
    u32 level, pad;
};
struct K12Row { u32 len, pidx, place, pad; };   // one block: its MTF-decoded last column lies at scrAt + place
struct K12Plan {
    const u8* in; const u64* off; u32 count;
    u32 opt;           // K12_OPT_*
    u64 budget;        // bytes of scratch a call may take
    K12Doc* doc;       // [count]
    K12Row* row;       // [flags[K12_F_BLK]]
    u8* scr;
    u64* flags;        // [K12_F_WORDS]
};
int k12_plan_run(K12Plan Q, hipStream_t stream);
int k12_decode_run(K12Plan Q, hipStream_t stream);     // levels 6-9; the documents of the other model are left alone
int k14_decode_run(K12Plan Q, hipStream_t stream);     // levels 1-5 (k14_defsum_decoder.hip)
int k34_run(Pipe P, hipStream_t stream);
int k3_alloc_lengths_run(long long* d_arr, const u32* d_off, u32 count, int maxlen, hipStream_t stream);
// Batched compression (cjs_bz2_compress_batch*): document d of the batch is input bytes [off[d], off[d+1]) and becomes a .bz2 stream of
// its own.  K0Docs (k0_docs.hip) is the plan's view of the documents, K5Docs (k5_docs.hip) the stream cursor's.
struct K0Docs {
    const u64* off;    // [count+1] document offsets (device), nondecreasing
    u32 count;
    u32* docFirst;     // [count+1] first block of document d (an empty document has none); [count] = blocks of the batch
    u32* blkDoc;       // [maxBlocks] document of block k
    u32* bad;          // [1] set when the plan needs more blocks than it has slots for
};
struct K5Docs {
    const u32* docFirst;
    const u32* blkDoc;
    u64* outOff;       // [count+1] byte offset of stream d in the output (device); [count] = bytes written
    u32 count;
    u32 level;
};
size_t k0_docs_bytes(u64 in_len, u32 count, u32 cap);
void k0_docs_carve(K0Buf& K, K0Docs& D, const u8* d_in, const u64* d_off, u64 in_len, u32 count, u32 cap, void* ws);
int k0_docs_check(const u64* d_off, u32 count, u64* d_res, hipStream_t stream);   // d_res[0] = off[count], d_res[1] != 0: the offsets decrease somewhere
int k0_docs_prepass(K0Buf K, K0Docs D, u32 cap, hipStream_t stream);             // tile scans + per-document block chains: *K.nBlocks, blk*, D.docFirst, D.blkDoc
int k5_docs_begin(Pipe P, K5Docs D, hipStream_t stream);                          // resets the cursor; the streams of the empty documents in front of the first block
int k5_docscan_run(Pipe P, K5Docs D, u32 first_block, hipStream_t stream);        // k5_blockscan's sibling: bit offsets, stream headers and trailers of a sub-batch

int k5_run(Pipe P, u32 max_n, hipStream_t stream, hipEvent_t after = nullptr, hipEvent_t done = nullptr, hipEvent_t crc_ready = nullptr,
           const K5Docs* docs = nullptr, u32 first_block = 0);   // crc_ready: the block CRCs were computed on another stream (k0_batch); docs: the batch path's cursor kernel instead of k5_blockscan
int k5_stream_begin(Pipe P, int level, hipStream_t stream, bool zero = true);   // zero = false: the caller has zeroed P.out (on another stream, next to the pre-pass)
int k5_stream_end(Pipe P, hipStream_t stream);
int k5_shift_bits_run(const u8* d_in, u64 nbytes, u32 s, u8* d_out, hipStream_t stream);
int k0_batch(K0Buf K, Pipe P, u32 first_block, u32 cap, hipStream_t stream, u32 crc_parts, hipStream_t side = nullptr, hipEvent_t ev_pad = nullptr, hipEvent_t ev_crc = nullptr);   // crc_parts: workgroups per block of k0_crc (1 .. 16)
size_t pipe_bytes(const BatchGeom& g);
void pipe_carve(Pipe& P, const BatchGeom& g, void* base);
int pipe_run_block_stages(Pipe& P, u32 max_n, hipStream_t stream, int upto, hipEvent_t after = nullptr,
                          hipEvent_t done = nullptr);
