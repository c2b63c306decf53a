// K11: the range coder of BWTC levels 6..9 on the GPU, ONE CODER PER DOCUMENT of a batch (cjs_bwtc_compress_batch*).
//
// The coder's state crosses the blocks of a stream, so one stream's entropy tail is serial (bwtc_host.hip); across
// the documents of a batch there are as many independent coders as documents.  K1 (linear), K2 and K10 leave, per block, the
// (sy_f, lt_f, tot_f) triples of FenwickModel; what is left of lib/BWTC.js:12-139 is restated here on the device:
//   Util.compressFileHelper      lib/Util.js:105-142         magic, varint(size + 1), last byte withheld        k11_begin
//   RangeCoder (encoder)         lib/RangeCoder.js:27-140    start / normalize / encodeFreq / encodeShift / finish   K11Enc
//   NoModel.encode               lib/NoModel.js:15-21        bits through encodeShift(1, b, 1)                   nomodel
//   LogDistanceModel.encode      lib/LogDistanceModel.js:24-36                                                   logdist
//   block header                 lib/BWTC.js:42-79           short-block flag, length, primary index, use tree   k11_block_header
//   "no more blocks" + finish    lib/BWTC.js:137-138                                                             k11_end
// (the host's RangeEnc, bwtc_begin, bwtc_block_header, bwtc_block_triples and bwtc_end of bwtc_host.hip, which stay what the single
// call runs: one lane is slower than one CPU core).
//
// k11_code: one launch per sub-batch, one lane per block slot.  The lane of a document's FIRST block in the sub-batch codes all of
// that document's blocks in it, in order; the other lanes of the document leave.  With one block per document - the batch of small
// records this is for - consecutive documents fill a wave, which runs as long as its longest document.  A document whose first
// block is in the launch begins with the stream header, one whose last block is in it ends the stream; in between the coder state
// (K11State: low, range, buffer, help, bytecount, the write cursor and the bytes of its last incomplete dword) waits in HBM.
// Documents without a block (empty ones) are begun and ended by k11_plan's own pass, exactly once.
//
// No per-lane arrays (they would live in scratch memory): the use tree's node i is the population count of an aligned range of the
// 256-bit used set, taken from its eight words, which are picked by selects.  floor(range / tot) is the compiler's 32-bit
// division, exact by construction (cjs_dbg_rc_div_device runs it alone for the tests).  The output is append-only - the held-back
// `buffer` byte and the `help` count do the carry - so a lane collects four bytes in a register and stores aligned dwords.
//
// The plan (k11_plan), the rows of a sub-batch (k11_gather), the offsets of the finished streams (k11_offsets) and their move from
// the scratch to their places (k11_copy) are here too: the batch never needs the offsets on the host.
#include "pipeline.h"
#include <string.h>

#define K11_TOP 0x80000000u            // Top_value    lib/RangeCoder.js:15
#define K11_BOTTOM (K11_TOP >> 8)      // Bottom_value :18
#define K11_SHIFT 23                   // SHIFT_BITS   :16

__device__ __forceinline__ u32 k11_div(u32 range, u32 tot) { return range / tot; }
__device__ __forceinline__ u32 k11_fls(u32 v) { return v ? 32u - (u32)__clz((int)v) : 0u; }     // lib/Util.js:301

struct K11Enc {                        // lib/RangeCoder.js:27-140 with the output of one document
    u32 low, range, buffer, help, bytecount, acc;
    u64 n, cap;                        // bytes so far; the document's bound: nothing is stored at or beyond it
    u32* w;                            // the document's stream in the scratch (dword aligned)
    __device__ __forceinline__ void put(u32 b) {
        if (n < cap) {
            const u32 k = (u32)n & 3u;
            acc |= (b & 0xFFu) << (8u * k);
            if (k == 3u) { w[n >> 2] = acc; acc = 0u; }
        }
        n++;
    }
    __device__ __forceinline__ void flush() { if (((u32)n & 3u) && (n & ~(u64)3) < cap) w[n >> 2] = acc; }   // (the last dword holds a stored byte; the scratch is cut in whole dwords)
    __device__ __forceinline__ void start(u32 c, u32 initlength) { low = 0u; range = K11_TOP; buffer = c; help = 0u; bytecount = initlength; }
    __device__ __forceinline__ void normalize() {                                                 // :38-60
        while (range <= K11_BOTTOM) {
            if (low < (0xFFu << K11_SHIFT)) {
                put(buffer);
                for (; help; help--) put(0xFFu);
                buffer = (low >> K11_SHIFT) & 0xFFu;
            } else if (low & K11_TOP) {
                put(buffer + 1u);
                for (; help; help--) put(0x00u);
                buffer = (low >> K11_SHIFT) & 0xFFu;
            } else {
                help++;
            }
            range <<= 8;
            low = (low << 8) & (K11_TOP - 1u);
            bytecount++;
        }
    }
    __device__ __forceinline__ void encodeFreq(u32 sy_f, u32 lt_f, u32 tot_f) {                    // :79-89
        normalize();
        const u32 r = k11_div(range, tot_f);
        const u32 tmp = r * lt_f;
        low += tmp;
        if (lt_f + sy_f < tot_f) range = r * sy_f; else range -= tmp;
    }
    __device__ __forceinline__ void encodeShift(u32 sy_f, u32 lt_f, u32 shift) {                   // :90-100
        normalize();
        const u32 r = range >> shift;
        const u32 tmp = r * lt_f;
        low += tmp;
        if ((lt_f + sy_f) >> shift) range -= tmp; else range = r * sy_f;
    }
    __device__ __forceinline__ void encodeBit(u32 b) { encodeShift(1u, b ? 1u : 0u, 1u); }         // :102-104
    __device__ __forceinline__ void finish() {                                                    // :116-140
        normalize();
        bytecount += 5u;
        u32 tmp = low >> K11_SHIFT;
        if ((low & (K11_BOTTOM - 1u)) >= ((bytecount & 0xFFFFFFu) >> 1)) tmp++;
        if (tmp > 0xFFu) { put(buffer + 1u); for (; help; help--) put(0x00u); }
        else { put(buffer); for (; help; help--) put(0xFFu); }
        put(tmp & 0xFFu);
        put((bytecount >> 16) & 0xFFu);
        put((bytecount >> 8) & 0xFFu);
        put(bytecount & 0xFFu);
    }
    __device__ __forceinline__ void nomodel(u32 bits, u32 sym) {                                   // lib/NoModel.js:15-21
        for (u32 i = bits; i > 0u; i--) encodeBit((sym >> (i - 1u)) & 1u);
    }
    __device__ __forceinline__ void logdist(u32 lgbits, u32 d) {                                   // lib/LogDistanceModel.js:24-36
        if (d < 2u) { nomodel(lgbits, d); return; }
        const u32 lg = k11_fls(d);
        nomodel(lgbits, lg);
        nomodel(lg - 1u, d & ((1u << (lg - 1u)) - 1u));        // distanceModel[lg] = NoModel(1 << (lg - 1)): lg - 1 bits
    }
    __device__ __forceinline__ void load(const K11State& s) { low = s.low; range = s.range; buffer = s.buffer; help = s.help; bytecount = s.bytecount; acc = s.acc; n = s.n; }
    __device__ __forceinline__ void save(K11State& s) const { s.low = low; s.range = range; s.buffer = buffer; s.help = help; s.bytecount = bytecount; s.acc = acc; s.n = n; }
};

// LogDistanceModel(blockSize, 0, NoModel, NoModel) (lib/BWTC.js:37-39): its length model is NoModel(1 + fls(size - 1))
__device__ __forceinline__ u32 k11_lgbits(u32 bs) { return k11_fls(k11_fls(bs - 1u)); }

// the stream header: Util.compressFileHelper (lib/Util.js:105-142) and lib/BWTC.js:13-20
__device__ __forceinline__ void k11_begin(K11Enc& E, u64 size, u32 level) {
    E.acc = 0u; E.n = 0u;
    E.put('b'); E.put('w'); E.put('t'); E.put('c');
    const u64 v = size + 1u;                                   // writeUnsignedNumber :194-206, 7 bits a byte, the last one withheld
    u32 nv = 1u;
    while (nv < 10u && (v >> (7u * nv))) nv++;
    for (u32 i = nv - 1u; i >= 1u; i--) E.put((u32)(v >> (7u * i)) & 0x7Fu);
    E.start(((u32)v & 0x7Fu) | 0x80u, 1u);
    E.encodeShift(1u, level, 8u);                              // encodeByte(level)  lib/BWTC.js:20
}
__device__ __forceinline__ void k11_end(K11Enc& E) {
    E.encodeFreq(1u, 2u, 3u);                                  // "no more blocks"  lib/BWTC.js:137
    E.finish();                                                // :138
    E.flush();
}

struct K11Used { u32 a, b, c, d, e, f, g, h; };                // the 256-bit used-symbol set
__device__ __forceinline__ u32 k11_pick(const K11Used& u, u32 k) {
    const u32 x01 = (k & 1u) ? u.b : u.a, x23 = (k & 1u) ? u.d : u.c, x45 = (k & 1u) ? u.f : u.e, x67 = (k & 1u) ? u.h : u.g;
    const u32 y0 = (k & 2u) ? x23 : x01, y1 = (k & 2u) ? x67 : x45;
    return (k & 4u) ? y1 : y0;
}
// useTree[i] of lib/BWTC.js:57-65, i = 1 .. 511: the used symbols among the 256 >> level that node i covers
__device__ __forceinline__ u32 k11_node(const K11Used& u, u32 i) {
    const u32 lv = k11_fls(i) - 1u, wd = 256u >> lv, s = (i - (1u << lv)) * wd;
    if (wd >= 32u) {
        u32 c = 0u;
        for (u32 k = 0; k < (wd >> 5); k++) c += (u32)__popc(k11_pick(u, (s >> 5) + k));
        return c;
    }
    return (u32)__popc((k11_pick(u, s >> 5) >> (s & 31u)) & ((1u << wd) - 1u));
}
// block header: short-block flag + length, primary index, used-symbol tree (lib/BWTC.js:42-79)
__device__ __forceinline__ void k11_block_header(K11Enc& E, u32 bs, u32 lgbits, u32 length, u32 pidx, const K11Used& u) {
    if (length == bs) E.encodeFreq(1u, 0u, 3u);                // :47-49
    else { E.encodeFreq(1u, 1u, 3u); E.logdist(lgbits, length); }   // :51-53
    E.logdist(lgbits, pidx);                                   // :56
    for (u32 i = 1u; i < 512u; i++) {                          // :66-79
        const u32 full = 1u << (9u - k11_fls(i));
        const u32 pv = i == 1u ? 1u : k11_node(u, i >> 1);     // (useTree[0] = 1)
        if (pv == 0u || pv == full * 2u) continue;
        const u32 v = k11_node(u, i);
        if (i >= 256u) E.encodeBit(v);
        else E.encodeFreq(1u, v == 0u ? 0u : (v == full ? 2u : 1u), 3u);
    }
}

__global__ __launch_bounds__(64) void k11_code(K11Plan Q, K11Sub S) {
    const u32 b0 = blockIdx.x * 64u + threadIdx.x;
    if (b0 >= S.nb) return;
    const u32 k0 = S.first + b0;
    const u32 d = Q.blkDoc[k0];
    if (b0 > 0u && Q.blkDoc[k0 - 1u] == d) return;             // an earlier lane codes this document
    const u32 kfirst = Q.docFirst[d], kend = Q.docFirst[d + 1u];
    const u32 kstop = kend < S.first + S.nb ? kend : S.first + S.nb;
    const u64 len = Q.off[d + 1u] - Q.off[d];
    K11Enc E;
    E.cap = k11_bound(len);
    E.w = Q.scr + (Q.docScr[d] >> 2);
    if (k0 == kfirst) k11_begin(E, len, Q.level);
    else E.load(Q.st[d]);
    const u32 lgbits = k11_lgbits(Q.bs);
    bool bad = false;
    for (u32 k = k0; k < kstop; k++) {
        const u32 b = k - S.first;
        const u32 ntri = S.ntri[b];
        if (ntri > S.ostride) { bad = true; break; }           // K10_OVERFLOW: no triples to code
        const u32* up = S.used + (size_t)b * 8u;
        const K11Used u = {up[0], up[1], up[2], up[3], up[4], up[5], up[6], up[7]};
        k11_block_header(E, Q.bs, lgbits, S.nlen[b], S.pidx[b], u);
        // RangeCoder.encodeFreq over the block's triples, four to a load, the next four requested before these are coded
        const uint4* a4 = (const uint4*)(S.sylt + (size_t)b * S.ostride);
        const uint4* t4 = (const uint4*)(S.tot + (size_t)b * S.ostride);
        const u32 n4 = (ntri + 3u) >> 2;                       // (ostride is a multiple of 4: the last load stays in the row)
        uint4 a = make_uint4(0u, 0u, 0u, 0u), t = a;
        if (n4) { a = a4[0]; t = t4[0]; }
        for (u32 j = 0; j < n4; j++) {
            uint4 an = a, tn = t;
            if (j + 1u < n4) { an = a4[j + 1u]; tn = t4[j + 1u]; }
            const u32 m = ntri - 4u * j;
            E.encodeFreq(a.x & 0xFFFFu, a.x >> 16, t.x);
            if (m > 1u) E.encodeFreq(a.y & 0xFFFFu, a.y >> 16, t.y);
            if (m > 2u) E.encodeFreq(a.z & 0xFFFFu, a.z >> 16, t.z);
            if (m > 3u) E.encodeFreq(a.w & 0xFFFFu, a.w >> 16, t.w);
            a = an; t = tn;
        }
    }
    if (bad) Q.flags[K11_F_K10] = 1u;
    if (!bad && kstop == kend) k11_end(E);
    if (E.n > E.cap) Q.flags[K11_F_SCRATCH] = 1u;
    E.save(Q.st[d]);
}

// ---- the plan ------------------------------------------------------------------------------------------
// One workgroup: thread t owns a run of consecutive documents.  Per document its blocks - the ceil(len / bs) fixed-size pieces of
// that document alone - and the bound of its stream; their exclusive scans are docFirst and docScr.  Then blkDoc, and the
// streams of the documents that have no block.
__global__ __launch_bounds__(1024) void k11_plan(K11Plan Q) {
    __shared__ u64 shB[1024], shS[1024];
    __shared__ u32 shM[1024];
    const u32 tid = threadIdx.x;
    const u32 per = (Q.count + 1023u) / 1024u;
    const u64 lo64 = (u64)tid * per;
    const u32 lo = lo64 < Q.count ? (u32)lo64 : Q.count, hi = lo64 + per < Q.count ? (u32)(lo64 + per) : Q.count;
    u64 nb = 0, scr = 0;
    u32 mx = 0;
    for (u32 d = lo; d < hi; d++) {
        const u64 len = Q.off[d + 1u] - Q.off[d];
        nb += (len + Q.bs - 1u) / Q.bs;
        scr += (k11_bound(len) + 3u) & ~(u64)3;
        const u32 l = len < Q.bs ? (u32)len : Q.bs;
        mx = l > mx ? l : mx;
    }
    shB[tid] = nb; shS[tid] = scr; shM[tid] = mx;
    __syncthreads();
    if (tid == 0) {
        u64 b = 0, s = 0;
        u32 m = 0;
        for (u32 i = 0; i < 1024u; i++) {
            const u64 vb = shB[i], vs = shS[i];
            shB[i] = b; shS[i] = s;
            b += vb; s += vs;
            m = shM[i] > m ? shM[i] : m;
        }
        const bool bad = b > Q.maxBlocks;
        Q.docFirst[Q.count] = bad ? 0u : (u32)b;
        Q.docScr[Q.count] = s;
        Q.flags[K11_F_NBLOCKS] = bad ? 0u : (u32)b;
        Q.flags[K11_F_MAXLEN] = m;
        Q.flags[K11_F_BAD] = bad ? 1u : 0u;
        shM[0] = bad ? 1u : 0u;
    }
    __syncthreads();
    if (shM[0]) return;
    u64 kb = shB[tid];
    scr = shS[tid];
    for (u32 d = lo; d < hi; d++) {
        const u64 len = Q.off[d + 1u] - Q.off[d];
        const u32 n = (u32)((len + Q.bs - 1u) / Q.bs);
        Q.docFirst[d] = (u32)kb;
        Q.docScr[d] = scr;
        for (u32 j = 0; j < n; j++) Q.blkDoc[kb + j] = d;
        if (n == 0u) {                                          // an empty document: header, "no more blocks", finish
            K11Enc E;
            E.cap = k11_bound(0u);
            E.w = Q.scr + (scr >> 2);
            k11_begin(E, 0u, Q.level);
            k11_end(E);
            E.save(Q.st[d]);
        }
        kb += n;
        scr += (k11_bound(len) + 3u) & ~(u64)3;
    }
}

// T_ext rows of a sub-batch: block k of the batch is bytes [j * bs, ..) of its document; the row ends in zeros (linear mode pads
// with the smallest symbol).  The single call copies rows with hipMemcpy2D; here they come from many documents.
__global__ __launch_bounds__(256) void k11_gather(K11Plan Q, u8* T, u32 tstride, u32* nlen, u32 first) {
    const u32 b = blockIdx.y, k = first + b;
    const u32 d = Q.blkDoc[k];
    const u64 d0 = Q.off[d], dend = Q.off[d + 1u];
    const u64 src = d0 + (u64)(k - Q.docFirst[d]) * Q.bs;
    const u32 len = dend - src < Q.bs ? (u32)(dend - src) : Q.bs;
    if (blockIdx.x == 0 && threadIdx.x == 0) nlen[b] = len;
    u32* row = (u32*)(T + (size_t)b * tstride);                // (tstride is a multiple of 64)
    const u8* s = Q.in + src;
    for (u32 wi = blockIdx.x * 256u + threadIdx.x; wi < tstride / 4u; wi += gridDim.x * 256u) {
        const u32 at = wi * 4u;
        u32 v = 0u;
        if (at + 4u <= len) v = (u32)s[at] | ((u32)s[at + 1u] << 8) | ((u32)s[at + 2u] << 16) | ((u32)s[at + 3u] << 24);
        else for (u32 q = 0; q < 4u; q++) if (at + q < len) v |= (u32)s[at + q] << (8u * q);
        row[wi] = v;
    }
}

// out_off: exclusive scan of the streams' sizes; [count] = the bytes of the batch; do they fit?
__global__ __launch_bounds__(1024) void k11_offsets(K11Plan Q, u64* out_off, u64 out_cap) {
    __shared__ u64 sh[1024];
    const u32 tid = threadIdx.x;
    const u32 per = (Q.count + 1023u) / 1024u;
    const u64 lo64 = (u64)tid * per;
    const u32 lo = lo64 < Q.count ? (u32)lo64 : Q.count, hi = lo64 + per < Q.count ? (u32)(lo64 + per) : Q.count;
    u64 s = 0;
    for (u32 d = lo; d < hi; d++) s += Q.st[d].n;
    sh[tid] = s;
    __syncthreads();
    if (tid == 0) {
        u64 a = 0;
        for (u32 i = 0; i < 1024u; i++) { const u64 v = sh[i]; sh[i] = a; a += v; }
        out_off[Q.count] = a;
        if (a > out_cap) Q.flags[K11_F_NOSPACE] = 1u;
    }
    __syncthreads();
    s = sh[tid];
    for (u32 d = lo; d < hi; d++) { out_off[d] = s; s += Q.st[d].n; }
}

// Stream d from the scratch to out[out_off[d] ..): workgroup (d, y) moves the y-th of gridDim.y pieces of it.  The scratch side
// is dword aligned, the output side is not: whole output dwords are built from two scratch dwords, the ends go byte by byte.
__global__ __launch_bounds__(256) void k11_copy(K11Plan Q, u8* out, const u64* out_off, u64 out_cap) {
    if (out_off[Q.count] > out_cap || Q.flags[K11_F_K10] || Q.flags[K11_F_SCRATCH]) return;   // nothing is delivered
    for (u32 d = blockIdx.x; d < Q.count; d += gridDim.x) {
        const u64 n = out_off[d + 1u] - out_off[d];
        const u32* sw = Q.scr + (Q.docScr[d] >> 2);
        const u8* sb = (const u8*)sw;
        u8* dst = out + out_off[d];
        u64 piece = (n + gridDim.y - 1u) / gridDim.y;
        piece = (piece + 255u) & ~(u64)255;
        const u64 p0 = (u64)blockIdx.y * piece < n ? (u64)blockIdx.y * piece : n;
        const u64 p1 = p0 + piece < n ? p0 + piece : n;       // this workgroup: stream bytes [p0, p1)
        if (p0 >= p1) continue;
        const u64 head = (4u - (u32)((uintptr_t)(dst + p0) & 3u)) & 3u;     // bytes in front of the first aligned output dword
        const u64 h1 = p0 + head < p1 ? p0 + head : p1;
        const u64 nw = (p1 - h1) >> 2;                         // whole output dwords
        for (u64 i = p0 + threadIdx.x; i < h1; i += 256u) dst[i] = sb[i];
        u32* dw = (u32*)(dst + h1);
        const u32 sh = (u32)(h1 & 3u) * 8u;
        for (u64 i = threadIdx.x; i < nw; i += 256u) {
            const u64 si = (h1 >> 2) + i;                      // scratch dword that holds stream byte h1 + 4 i
            u32 v = sw[si];
            if (sh) v = (v >> sh) | (sw[si + 1u] << (32u - sh));   // (si + 1 holds stream byte h1 + 4 i + 3 < n: inside the document's scratch)
            dw[i] = v;
        }
        for (u64 i = h1 + nw * 4u + threadIdx.x; i < p1; i += 256u) dst[i] = sb[i];
    }
}

__global__ __launch_bounds__(256) void k11_div_test(const u32* range, const u32* tot, u32 n, u32* out) {
    const u32 i = blockIdx.x * 256u + threadIdx.x;
    if (i < n) out[i] = k11_div(range[i], tot[i]);
}

// ---- host side ---------------------------------------------------------------------------------------
static inline size_t k11_al(size_t x) { return (x + 255) & ~(size_t)255; }
static inline u64 k11_max_blocks(u64 in_len, u32 count, u32 bs) { return in_len / bs + (u64)count + 1; }

size_t k11_plan_bytes(u64 in_len, u32 count, u32 bs) {
    const u64 mb = k11_max_blocks(in_len, count, bs);
    return k11_al(((size_t)count + 1) * 4) + k11_al(((size_t)count + 1) * 8) + k11_al((size_t)mb * 4) + k11_al((size_t)count * sizeof(K11State)) +
           k11_al(K11_F_WORDS * 4) + k11_al((size_t)(in_len + in_len / 4 + (u64)count * 4100u) + 64);
}

void k11_plan_carve(K11Plan& Q, const u8* d_in, const u64* d_off, u64 in_len, u32 count, int level, void* ws) {
    memset(&Q, 0, sizeof Q);
    Q.in = d_in; Q.off = d_off; Q.count = count;
    Q.level = (u32)level; Q.bs = (u32)level * 100000u;
    Q.maxBlocks = (u32)k11_max_blocks(in_len, count, Q.bs);
    char* p = (char*)ws;
    Q.docFirst = (u32*)p; p += k11_al(((size_t)count + 1) * 4);
    Q.docScr = (u64*)p; p += k11_al(((size_t)count + 1) * 8);
    Q.blkDoc = (u32*)p; p += k11_al((size_t)Q.maxBlocks * 4);
    Q.st = (K11State*)p; p += k11_al((size_t)count * sizeof(K11State));
    Q.flags = (u32*)p; p += k11_al(K11_F_WORDS * 4);
    Q.scr = (u32*)p;
}

int k11_plan_run(K11Plan Q, hipStream_t stream) {
    HIP_CHECK_RET(hipMemsetAsync(Q.flags, 0, K11_F_WORDS * 4, stream));
    hipLaunchKernelGGL(k11_plan, dim3(1), dim3(1024), 0, stream, Q);
    HIP_CHECK_RET(hipGetLastError());
    return CJS_OK;
}

int k11_gather_run(K11Plan Q, Pipe P, u32 first, hipStream_t stream) {
    const u32 words = P.g.tstride / 4u;
    const u32 gx = (words + 256u * 8u - 1u) / (256u * 8u);     // eight dwords a thread
    hipLaunchKernelGGL(k11_gather, dim3(gx, P.g.nb), dim3(256), 0, stream, Q, P.T, P.g.tstride, P.nlen, first);
    HIP_CHECK_RET(hipGetLastError());
    return CJS_OK;
}

int k11_code_run(K11Plan Q, K11Sub S, hipStream_t stream) {
    hipLaunchKernelGGL(k11_code, dim3((S.nb + 63u) / 64u), dim3(64), 0, stream, Q, S);
    HIP_CHECK_RET(hipGetLastError());
    return CJS_OK;
}

int k11_finish_run(K11Plan Q, u8* d_out, u64 out_cap, u64* d_out_off, u32 split, hipStream_t stream) {
    hipLaunchKernelGGL(k11_offsets, dim3(1), dim3(1024), 0, stream, Q, d_out_off, out_cap);
    const u32 gx = Q.count < (1u << 20) ? Q.count : (1u << 20);
    hipLaunchKernelGGL(k11_copy, dim3(gx, split ? split : 1u), dim3(256), 0, stream, Q, d_out, (const u64*)d_out_off, out_cap);
    HIP_CHECK_RET(hipGetLastError());
    return CJS_OK;
}

// (tests) floor(range / tot) as k11_code computes it: host pointers in and out, one tiny kernel
extern "C" int cjs_dbg_rc_div_device(const uint32_t* range, const uint32_t* tot, uint32_t n, uint32_t* out) {
    if (!n) return CJS_OK;
    if (!range || !tot || !out) return CJS_E_ARG;
    u32* d = nullptr;
    HIP_CHECK_RET(hipMalloc((void**)&d, (size_t)n * 12));
    hipError_t e = hipMemcpy(d, range, (size_t)n * 4, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(d + n, tot, (size_t)n * 4, hipMemcpyHostToDevice);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(k11_div_test, dim3((n + 255u) / 256u), dim3(256), 0, (hipStream_t) nullptr, (const u32*)d, (const u32*)(d + n), n, d + 2 * (size_t)n);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpy(out, d + 2 * (size_t)n, (size_t)n * 4, hipMemcpyDeviceToHost);
    (void)hipFree(d);
    return e == hipSuccess ? CJS_OK : CJS_E_HIP - (int)e;
}
