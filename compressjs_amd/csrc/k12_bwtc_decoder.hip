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
// k12_plan: a lane per document reads the header (magic, size, level) and decides: -30, -31, the host path (levels 1-5 unless the
// call puts them on the device, no size declared, a size beyond what is left of the call's scratch budget), or the fast path with
// `declared` bytes of scratch and ceil(declared / (level * 100000)) block rows - exclusive scans over both, as k11_plan's.
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
// K12Window, K12Dec, k12_header and the decoder's body (k12_decode_body) live in k12_dec.h: k14_defsum_decoder.hip runs the same body
// over DefSumModel for levels 1-5, where the call asks for it (CJS_BWTC_DEC_DEFSUM_DEVICE); k12_plan counts the admitted documents
// of either model, and the host launches the kernels that have any.
// Termination: every byte read moves `pos` towards the stream's end, beyond it the decoder is at end-of-input and the symbol loop
// leaves; the symbol loop is bounded by the block's length, the block loop by the document's rows, the use tree by 511.
#include "k12_dec.h"
#include "k10_tree.h"

// the stream's bytes, one lane on its own (k12_plan)
struct K12Direct {
    const u8* p; u64 n, pos; bool eof;
    __device__ __forceinline__ void open(const u8* p_, u64 n_) { p = p_; n = n_; pos = 0; eof = false; }
    __device__ __forceinline__ u32 readByte() { if (pos < n) return p[pos++]; eof = true; return 0xFFFFFFFFu; }
};

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
            r.status = k12_header(D, &r.declared, &r.level, Q.opt);
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
    u64 useS = 0, useB = 0, nFen = 0, nDef = 0;
    for (u32 d = lo; d < hi; d++) {
        if (Q.doc[d].status != 0) continue;
        const u32 len = Q.doc[d].scrLen, bm = Q.doc[d].blkMax;
        if (scr + len > Q.budget) { Q.doc[d].status = K12_HOST; Q.doc[d].scrLen = 0u; Q.doc[d].blkMax = 0u; }
        else {
            Q.doc[d].scrAt = scr; Q.doc[d].blk0 = (u32)nb;
            useS = scr + (((u64)len + 3u) & ~(u64)3); useB = nb + bm;
            if (Q.doc[d].level > 5u) nFen++; else nDef++;
        }
        scr += ((u64)len + 3u) & ~(u64)3;
        nb += bm;
    }
    if (useS) atomicMax(&Q.flags[K12_F_SCR], useS);
    if (useB) atomicMax(&Q.flags[K12_F_BLK], useB);
    if (nFen) atomicAdd(&Q.flags[K12_F_NFEN], nFen);          // which decode kernels the host launches
    if (nDef) atomicAdd(&Q.flags[K12_F_NDEF], nDef);
}

// ---- the decoder ---------------------------------------------------------------------------------------
struct K12Fenwick {
    static constexpr u32 WORDS = 2 * K10_MAXSYM + 8;
    u32* tree; u32 numSyms, lane;
    __device__ static __forceinline__ bool mine(u32 level) { return level > 5u; }
    __device__ __forceinline__ void init(u32* mem, u32 alphabetSize, u32 lane_);
    __device__ __forceinline__ u32 decode(K12Dec<K12Window>& D);
};

// FenwickModel._rescale  lib/FenwickModel.js:137-166 (wave-uniform call), as k10_model's
__device__ __forceinline__ void k12_rescale(const K12Fenwick& m) {
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
__device__ __forceinline__ u32 k12_fen1(const K12Fenwick& m, K12Dec<K12Window>& D, bool isEscape) {
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
__device__ __forceinline__ u32 k12_fen(const K12Fenwick& m, K12Dec<K12Window>& D) {                // :129-136
    u32 s = k12_fen1(m, D, false);
    if (!D.in.eof && s == m.numSyms - 1u) s = k12_fen1(m, D, true);
    return s;
}
// FenwickModel(coder, alphabetSize + 1, 0xFF00, 0x0100) lib/BWTC.js:196-197, init lib/FenwickModel.js:13-32
__device__ __forceinline__ void K12Fenwick::init(u32* mem, u32 alphabetSize, u32 lane_) {
    tree = mem; lane = lane_; numSyms = alphabetSize + 2u;
    for (u32 i = lane; i < 2u * numSyms; i += 64u) tree[i] = i >= numSyms ? (i == 2u * numSyms - 1u ? 0x0100u << 16 : 1u) : 0u;
    __builtin_amdgcn_wave_barrier();
    k10_sum_tree(tree, numSyms, lane);
}
__device__ __forceinline__ u32 K12Fenwick::decode(K12Dec<K12Window>& D) { return k12_fen(*this, D); }

__global__ __launch_bounds__(64) void k12_decode(K12Plan Q) { k12_decode_body<K12Fenwick>(Q); }


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
