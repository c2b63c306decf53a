// K12: the decoder of BWTC levels 6..9 on the GPU, ONE WAVE PER DOCUMENT of a batch (cjs_bwtc_decompress_batch*).
//
// One stream's entropy tail is serial, and on the decoder side the model cannot be split from the coder as K10 / K11 split them:
// the symbol that updates the model is not known until the range decoder has produced it.  Across the documents of a batch there
// are as many independent decoders as documents.  What bwtc_host.hip's bwtc_decode does on one host thread is restated here:
//   Util.decompressFileHelper    lib/Util.js:143-166,211-220   magic, varint(size + 1)                         k12_header
//   RangeCoder (decoder)         lib/RangeCoder.js:146-226     decodeStart(true) / normalize / culFreq / culShift / update   K12Dec
//   NoModel.decode               lib/NoModel.js:22-29                                                           nomodel
//   LogDistanceModel.decode      lib/LogDistanceModel.js:37-44                                                  logdist
//   the use tree                 lib/BWTC.js:172-195                                                            k12_decode
//   FenwickModel._decode/decode  lib/FenwickModel.js:88-172    with rescale and the last-escape zeroing         k12_fen1
//   RUNA / RUNB and the MTF      lib/BWTC.js:200-223                                                            k12_decode
// (the host's RangeDec, fenwick_decode1 and bwtc_decode stay what the single call and this batch's host path run).
//
// k12_plan: a lane per document reads the header (magic, size, level) and decides: -30, -31, the host path (levels 1-5, no size
// declared, a size beyond what is left of the call's scratch budget), or the fast path with `declared` bytes of scratch and
// ceil(declared / (level * 100000)) block rows - exclusive scans over both, as k11_plan's.
//
// k12_decode: workgroup d = one wave = document d.  Everything the decoder decides is wave-uniform (all lanes hold the same
// coder state and walk the same tree: the descent is a dependent chain, one lane's worth of work).  The wave's width is used for
//   the path update (lane l holds node leaf >> l, as K10's walk), the rescale and the rebuild (k10_sum_tree),
//   the MTF shift (64 entries a step), filling a zero run, and fetching the input ahead of the decoder (two registers of 64
//   dwords: the one in use and the next; a byte is a v_readlane away).
// The packed Fenwick tree (2 * 258 words), the use tree and the MTF array live in LDS; no per-lane arrays.  range / tot and
// low / help are the compiler's 32-bit divisions.  Out: the MTF-decoded last column of every block, back to back in the document's
// scratch, a row (length, pidx, place) per block, the document's status.  A document that holds more bytes or blocks than its header
// declares is handed to the host path (K12_HOST) rather than given more room.
// Termination: every byte read moves `pos` towards the stream's end, beyond it the decoder is at end-of-input and the symbol loop
// leaves; the symbol loop is bounded by the block's length, the block loop by the document's rows, the use tree by 511.
#include "pipeline.h"
#include "k10_tree.h"

#define K12_TOP 0x80000000u            // Top_value    lib/RangeCoder.js:15
#define K12_BOTTOM (K12_TOP >> 8)      // Bottom_value :18
#define K12_NVAL_MAX (1ull << 50)      // a declared size beyond this is left to the host path (which computes it as the reference does, in a double)
#define K12_E_MAGIC (-30)
#define K12_E_CORRUPT (-31)

__device__ __forceinline__ u32 k12_fls(u32 v) { return v ? 32u - (u32)__clz((int)v) : 0u; }     // lib/Util.js:301

// the stream's bytes, one lane on its own (k12_plan)
struct K12Direct {
    const u8* p; u64 n, pos; bool eof;
    __device__ __forceinline__ void open(const u8* p_, u64 n_) { p = p_; n = n_; pos = 0; eof = false; }
    __device__ __forceinline__ u32 readByte() { if (pos < n) return p[pos++]; eof = true; return 0xFFFFFFFFu; }
};
// the stream's bytes for a whole wave in uniform control flow: the aligned dwords around byte `pos`, 64 in r0 and the next 64 in r1
struct K12Window {
    const u8* p; u64 n, pos; bool eof;
    u32 mis, lane, r0, r1;             // mis: p's misalignment - window byte k is stream byte k - mis
    u64 wb;                            // first window byte of r0 (a multiple of 256)
    // the dword of window bytes [at, at + 4): only the document's own bytes are ever loaded
    __device__ __forceinline__ u32 fetch(u64 at) const {
        const long long rel = (long long)at - (long long)mis;
        if (rel >= 0 && (u64)rel + 4u <= n) return *(const u32*)(p + rel);
        u32 v = 0u;
        for (int q = 0; q < 4; q++) { const long long r = rel + q; if (r >= 0 && (u64)r < n) v |= (u32)p[r] << (8 * q); }
        return v;
    }
    __device__ __forceinline__ void open(const u8* p_, u64 n_) {
        p = p_; n = n_; pos = 0; eof = false;
        mis = (u32)((uintptr_t)p_ & 3u); lane = threadIdx.x & 63u; wb = 0;
        r0 = fetch((u64)lane * 4u); r1 = fetch(256u + (u64)lane * 4u);
    }
    __device__ __forceinline__ u32 readByte() {
        if (pos >= n) { eof = true; return 0xFFFFFFFFu; }
        u64 k = pos + mis - wb;        // <= 256: pos moves a byte at a time
        if (k >= 256u) { wb += 256u; r0 = r1; r1 = fetch(wb + 256u + (u64)lane * 4u); k -= 256u; }
        const u32 dw = (u32)__builtin_amdgcn_readlane((int)r0, (int)(k >> 2));
        pos++;
        return (dw >> (8u * ((u32)k & 3u))) & 0xFFu;
    }
};

template <class R> struct K12Dec {     // lib/RangeCoder.js:146-226 (EXTRA_BITS = 7); `buffer` = -1 at end-of-input, as readByte gives it
    R in;
    u32 low, range, help, buffer;
    __device__ __forceinline__ void start() { buffer = in.readByte(); low = buffer >> 1; range = 1u << 7; help = 0u; }   // decodeStart(true)
    __device__ __forceinline__ void normalize() {                                                 // :157-166
        while (range <= K12_BOTTOM) {
            if (range == 0u) { in.eof = true; return; }        // (no stream gets here: shifting 0 would never end)
            low = (low << 8) | ((buffer << 7) & 0xFFu);
            buffer = in.readByte();
            low |= buffer >> 1;
            range <<= 8;
        }
    }
    __device__ __forceinline__ u32 culFreq(u32 tot) {                                             // :173-178
        normalize();
        help = range / tot;
        if (help == 0u) { in.eof = true; return 0u; }
        const u32 tmp = low / help;
        return tmp >= tot ? tot - 1u : tmp;
    }
    __device__ __forceinline__ u32 culShift(u32 shift) {                                          // :179-185
        normalize();
        help = range >> shift;
        if (help == 0u) { in.eof = true; return 0u; }
        const u32 tmp = low / help;
        return (tmp >> shift) ? (1u << shift) - 1u : tmp;
    }
    __device__ __forceinline__ void update(u32 sy_f, u32 lt_f, u32 tot_f) {                       // :192-200
        const u32 tmp = help * lt_f;
        low -= tmp;
        if (lt_f + sy_f < tot_f) range = help * sy_f; else range -= tmp;
    }
    __device__ __forceinline__ u32 freq3() { const u32 v = culFreq(3u); update(1u, v, 3u); return v; }
    __device__ __forceinline__ u32 bit() { const u32 t = culShift(1u); update(1u, t, 2u); return t; }        // :203-207
    __device__ __forceinline__ u32 byte() { const u32 t = culShift(8u); update(1u, t, 256u); return t; }     // :209-213
    __device__ __forceinline__ u32 nomodel(u32 bits) {                                            // lib/NoModel.js:22-29
        u32 r = 0u;
        for (u32 i = 0; i < bits; i++) r = (r << 1) | bit();
        return r;
    }
    __device__ __forceinline__ u32 logdist(u32 lgbits) {                                          // lib/LogDistanceModel.js:37-44
        const u32 lg = nomodel(lgbits);
        if (lg < 2u) return lg;
        if (lg > 32u) { in.eof = true; return 0u; }
        return (1u << (lg - 1u)) + nomodel(lg - 1u);
    }
};

// Util.decompressFileHelper (lib/Util.js:143-166) and lib/BWTC.js:142-146, in bwtc_decode's order of checks: 0 (a FenwickModel stream
// with its size declared: the coder stands behind the level byte), -30, -31 or K12_HOST.  *declared as the single call reports it.
template <class R> __device__ __forceinline__ int k12_header(K12Dec<R>& D, long long* declared, u32* level) {
    *declared = -1; *level = 0u;
    for (u32 i = 0; i < 4u; i++) {
        const u32 b = D.in.readByte();
        if (D.in.eof || b != ((0x63747762u >> (8u * i)) & 0xFFu)) return K12_E_MAGIC;              // "bwtc"
    }
    u64 nval = 0;                                              // readUnsignedNumber :211-220
    for (;;) {
        const u32 c = D.in.readByte();
        if (D.in.eof) return K12_E_CORRUPT;
        if (c & 0x80u) { nval += c & 0x7Fu; break; }
        nval = (nval + c) * 128u;
        if (nval > K12_NVAL_MAX) return K12_HOST;
    }
    *declared = (long long)nval - 1;
    D.start();                                                 // lib/BWTC.js:142-143
    const u32 lv = D.byte();                                   // :144
    if (D.in.eof || lv < 1u || lv > 9u) return K12_E_CORRUPT;
    *level = lv;
    if (lv <= 5u || nval == 0u) return K12_HOST;               // DefSumModel (:146); no size declared
    return 0;
}

// ---- the plan ------------------------------------------------------------------------------------------
// One workgroup: thread t owns a run of consecutive documents, as in k11_plan.  A document is ADMITTED to the fast path while the
// scratch of the candidates up to and including it stays inside the budget (a prefix of the candidates: once the budget is spent
// every later one takes the host path), so what a call allocates is bounded by the budget, never by what a header claims.
__global__ __launch_bounds__(1024) void k12_plan(K12Plan Q) {
    __shared__ u64 shS[1024], shB[1024];
    __shared__ u32 shBad[1];
    const u32 tid = threadIdx.x;
    if (tid == 0) shBad[0] = 0u;
    __syncthreads();
    const u32 per = (Q.count + 1023u) / 1024u;
    const u64 lo64 = (u64)tid * per;
    const u32 lo = lo64 < Q.count ? (u32)lo64 : Q.count, hi = lo64 + per < Q.count ? (u32)(lo64 + per) : Q.count;
    u64 scr = 0, nb = 0;
    // the offsets first: no byte of the input is read unless all of them are in order (then every document lies inside in[0, off[count]))
    for (u32 d = lo; d < hi; d++) {
        const u64 o0 = Q.off[d], o1 = Q.off[d + 1u];
        if (o1 < o0 || (o1 > o0 && !Q.in)) shBad[0] = 1u;
    }
    __syncthreads();
    if (shBad[0]) {
        if (tid == 0) Q.flags[K12_F_BAD] = 1u;
        return;
    }
    for (u32 d = lo; d < hi; d++) {
        const u64 o0 = Q.off[d], o1 = Q.off[d + 1u];
        K12Doc r;
        r.scrAt = 0; r.declared = -1; r.scrLen = 0u; r.blk0 = 0u; r.blkMax = 0u; r.status = K12_E_MAGIC; r.nblk = 0u; r.size = 0u; r.level = 0u; r.pad = 0u;
        {
            K12Dec<K12Direct> D;
            D.in.open(Q.in + o0, o1 - o0);
            r.status = k12_header(D, &r.declared, &r.level);
            if (r.status == 0) {
                if ((u64)r.declared > Q.budget) r.status = K12_HOST;
                else {
                    const u32 bs = r.level * 100000u;
                    r.scrLen = (u32)r.declared;
                    r.blkMax = (r.scrLen + bs - 1u) / bs;
                    scr += ((u64)r.scrLen + 3u) & ~(u64)3;
                    nb += r.blkMax;
                }
            }
        }
        Q.doc[d] = r;
    }
    shS[tid] = scr; shB[tid] = nb;
    __syncthreads();
    if (tid == 0) {
        u64 s = 0, b = 0;
        for (u32 i = 0; i < 1024u; i++) {
            const u64 vs = shS[i], vb = shB[i];
            shS[i] = s; shB[i] = b;
            s += vs; b += vb;
        }
        Q.flags[K12_F_TOTAL] = Q.off[Q.count];
    }
    __syncthreads();
    scr = shS[tid]; nb = shB[tid];
    u64 useS = 0, useB = 0;
    for (u32 d = lo; d < hi; d++) {
        if (Q.doc[d].status != 0) continue;
        const u32 len = Q.doc[d].scrLen, bm = Q.doc[d].blkMax;
        if (scr + len > Q.budget) { Q.doc[d].status = K12_HOST; Q.doc[d].scrLen = 0u; Q.doc[d].blkMax = 0u; }
        else {
            Q.doc[d].scrAt = scr; Q.doc[d].blk0 = (u32)nb;
            useS = scr + (((u64)len + 3u) & ~(u64)3); useB = nb + bm;
        }
        scr += ((u64)len + 3u) & ~(u64)3;
        nb += bm;
    }
    if (useS) atomicMax(&Q.flags[K12_F_SCR], useS);
    if (useB) atomicMax(&Q.flags[K12_F_BLK], useB);
}

// ---- the decoder ---------------------------------------------------------------------------------------
struct K12Model { u32* tree; u32 numSyms, lane; };

// FenwickModel._rescale  lib/FenwickModel.js:137-166 (wave-uniform call), as k10_model's
__device__ __forceinline__ void k12_rescale(const K12Model& m) {
    u32* tree = m.tree;
    const u32 numSyms = m.numSyms, lane = m.lane;
    bool noEscape = true;
    for (u32 j = lane; j < numSyms - 1u; j += 64u) {
        u32 p = tree[numSyms + j];
        if (p & 0xFFFFu) { noEscape = false; continue; }
        p = (p & 0xFFFEFFFEu) >> 1;
        if (p == 0u) { p = 1u; noEscape = false; }
        tree[numSyms + j] = p;
    }
    const bool allNo = __ballot(!noEscape) == 0ull;
    if (lane == 0) {
        u32 p = tree[2u * numSyms - 1u];
        p = (p & 0xFFFEFFFEu) >> 1;
        if (allNo) p = 0u; else if (p == 0u) p = 1u << 16;
        tree[2u * numSyms - 1u] = p;
    }
    __builtin_amdgcn_wave_barrier();
    k10_sum_tree(tree, numSyms, lane);
}

// FenwickModel._decode  lib/FenwickModel.js:88-128: the descent reads the tree only (a node's own increment does not reach its
// children), then the nodes of the leaf's path take the update together, lane l the node leaf >> l
__device__ __forceinline__ u32 k12_fen1(const K12Model& m, K12Dec<K12Window>& D, bool isEscape) {
    u32* tree = m.tree;
    const u32 numSyms = m.numSyms, lane = m.lane;
    const u32 mask = isEscape ? 0x0000FFFFu : 0xFFFF0000u, shift = isEscape ? 0u : 16u;
    const u32 update = isEscape ? (0x0100u << 16) - 1u : (0x0100u << 16);
    const u32 tot_f = (tree[1] & mask) >> shift;
    if (tot_f == 0u) { D.in.eof = true; return 0u; }
    const u32 prob = D.culFreq(tot_f);
    if (D.in.eof) return 0u;
    u32 i = 1u, lt_f = 0u;
    while (i < numSyms) {
        const u32 leftProb = (tree[2u * i] & mask) >> shift;
        i *= 2u;
        if (prob - lt_f >= leftProb) { lt_f += leftProb; i++; }
    }
    const u32 symbol = i - numSyms;
    const u32 leafv = tree[i];
    const u32 sy_f = (leafv & mask) >> shift;
    const u32 L = 32u - (u32)__clz((int)i);                    // nodes on the path incl. the root
    const u32 node = i >> lane;
    const bool on = lane < L;
    __builtin_amdgcn_wave_barrier();
    if (on) tree[node] += update;
    __builtin_amdgcn_wave_barrier();
    D.update(sy_f, lt_f, tot_f);
    if (symbol == numSyms - 1u && (tree[1] & 0xFFFFu) == 1u) {                                     // the last escape: zero it out
        const u32 zero = 0u - (leafv + update);
        __builtin_amdgcn_wave_barrier();
        if (on) tree[node] += zero;
        __builtin_amdgcn_wave_barrier();
    }
    if ((tree[1] >> 16) >= 0xFF00u) k12_rescale(m);
    return symbol;
}
__device__ __forceinline__ u32 k12_fen(const K12Model& m, K12Dec<K12Window>& D) {                // :129-136
    u32 s = k12_fen1(m, D, false);
    if (!D.in.eof && s == m.numSyms - 1u) s = k12_fen1(m, D, true);
    return s;
}

__global__ __launch_bounds__(64) void k12_decode(K12Plan Q) {
    __shared__ u32 tree[2 * K10_MAXSYM + 8];
    __shared__ u16 useTree[512];
    __shared__ u8 M[256];
    const u32 d = blockIdx.x, lane = threadIdx.x;
    const K12Doc doc = Q.doc[d];
    if (doc.status != 0) return;                               // decided by the plan
    K12Dec<K12Window> D;
    D.in.open(Q.in + Q.off[d], Q.off[d + 1u] - Q.off[d]);
    long long declared;
    u32 level;
    int status = k12_header(D, &declared, &level);            // (the plan's answer again: 0; the coder now stands behind the level byte)
    const u32 blockSize = level * 100000u;
    const u32 lgbits = k12_fls(k12_fls(blockSize - 1u));       // LogDistanceModel(blockSize, 0, NoModel, NoModel): NoModel(1 + fls(size - 1))
    u8* scr = Q.scr + doc.scrAt;
    K12Row* rows = Q.row + doc.blk0;
    u32 nblk = 0u, place = 0u;
    while (status == 0) {
        const u32 ind = D.freq3();                             // lib/BWTC.js:158-159
        if (D.in.eof) { status = K12_E_CORRUPT; break; }
        if (ind == 2u) break;                                  // no more blocks :166-167
        const u32 length = ind == 0u ? blockSize : D.logdist(lgbits);
        const u32 pidx = D.logdist(lgbits);                    // :170
        if (D.in.eof || length > blockSize || pidx > length) { status = K12_E_CORRUPT; break; }
        // the use tree :172-186 (node i needs its parent: serial, uniform)
        if (lane == 0) useTree[0] = 1;
        __builtin_amdgcn_wave_barrier();
        for (u32 i = 1u; i < 512u; i++) {
            const u32 pv = useTree[i >> 1];
            const u32 full = 1u << (9u - k12_fls(i));
            u32 v;
            if (pv == 0u || pv == full * 2u) v = pv >> 1;
            else if (i >= 256u) v = D.bit();
            else { const u32 t = D.freq3(); v = t == 2u ? full : t; }
            __builtin_amdgcn_wave_barrier();
            if (lane == 0) useTree[i] = (u16)v;
            __builtin_amdgcn_wave_barrier();
        }
        if (D.in.eof) { status = K12_E_CORRUPT; break; }
        u32 alphabetSize = 0u;                                 // :188-193
        for (u32 r = 0; r < 4u; r++) {
            const bool used = useTree[256u + r * 64u + lane] != 0;
            const u64 bal = __ballot(used);
            if (used) M[alphabetSize + (u32)__popcll(bal & lanemask_lt())] = (u8)(r * 64u + lane);
            alphabetSize += (u32)__popcll(bal);
        }
        // a document with more blocks or bytes than its header declares: the host path decodes it (nothing here is kept)
        if (nblk >= doc.blkMax || length > doc.scrLen - place) { status = K12_HOST; break; }
        if (length && alphabetSize == 0u) { status = K12_E_CORRUPT; break; }   // (bwtc_decode: the first MTF index is >= alphabetSize)
        // FenwickModel(coder, alphabetSize + 1, 0xFF00, 0x0100) :196-197, init lib/FenwickModel.js:13-32
        K12Model m;
        m.tree = tree; m.lane = lane; m.numSyms = alphabetSize + 2u;
        for (u32 i = lane; i < 2u * m.numSyms; i += 64u) tree[i] = i >= m.numSyms ? (i == 2u * m.numSyms - 1u ? 0x0100u << 16 : 1u) : 0u;
        __builtin_amdgcn_wave_barrier();
        k10_sum_tree(tree, m.numSyms, lane);
        u8* out = scr + place;
        u32 val = 1u, i = 0u;
        while (i < length) {                                   // :200-223, the MTF decode applied as the symbols come
            const u32 c = k12_fen(m, D);
            if (D.in.eof) { status = K12_E_CORRUPT; break; }
            if (c <= 1u) {                                     // RUNA / RUNB: val * (c + 1) times the front of the MTF list
                const u32 cnt = val * (c + 1u);
                if (cnt > length - i) { status = K12_E_CORRUPT; break; }       // the reference would write past the block
                const u8 z = M[0];
                for (u32 k = lane; k < cnt; k += 64u) out[i + k] = z;
                i += cnt;
                val *= 2u;                                     // (cnt <= length: no overflow)
            } else {
                val = 1u;
                const u32 j = c - 1u;
                if (j >= alphabetSize) { status = K12_E_CORRUPT; break; }
                const u8 ch = M[j];
                for (int r = (int)((j - 1u) >> 6); r >= 0; r--) {              // M[k] = M[k - 1] for k = j .. 1, the highest 64 first
                    const u32 k = (u32)r * 64u + lane + 1u;
                    const bool mv = k <= j;
                    const u8 v = mv ? M[k - 1u] : (u8)0;
                    __builtin_amdgcn_wave_barrier();
                    if (mv) M[k] = v;
                    __builtin_amdgcn_wave_barrier();
                }
                if (lane == 0) { M[0] = ch; out[i] = ch; }
                __builtin_amdgcn_wave_barrier();
                i++;
            }
        }
        if (status != 0) break;
        if (lane == 0) { K12Row rw; rw.len = length; rw.pidx = pidx; rw.place = place; rw.pad = 0u; rows[nblk] = rw; }
        nblk++;
        place += length;
    }
    if (lane == 0) {
        Q.doc[d].status = status;
        Q.doc[d].nblk = status == 0 ? nblk : 0u;
        Q.doc[d].size = status == 0 ? place : 0u;
    }
}

int k12_plan_run(K12Plan Q, hipStream_t stream) {
    HIP_CHECK_RET(hipMemsetAsync(Q.flags, 0, K12_F_WORDS * 8, stream));
    hipLaunchKernelGGL(k12_plan, dim3(1), dim3(1024), 0, stream, Q);
    HIP_CHECK_RET(hipGetLastError());
    return CJS_OK;
}

int k12_decode_run(K12Plan Q, hipStream_t stream) {
    hipLaunchKernelGGL(k12_decode, dim3(Q.count), dim3(64), 0, stream, Q);
    HIP_CHECK_RET(hipGetLastError());
    return CJS_OK;
}
