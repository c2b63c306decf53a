// The range decoder of the batched BWTC decode (cjs_bwtc_decompress_batch*), ONE WAVE PER DOCUMENT: everything but the adaptive
// model.  k12_bwtc_decoder.hip (FenwickModel, levels 6-9: k12_decode) and k14_defsum_decoder.hip (DefSumModel, levels 1-5:
// k14_decode) are k12_decode_body over their model; k12_plan reads the headers with k12_header.  What is restated from the
// reference, the wave's use of its width and the termination argument stand in k12_bwtc_decoder.hip's header.
//
// A model is a struct with
//   WORDS                  u32 of LDS it needs
//   mine(level)            whether a stream of that level is this model's (a workgroup of the other kernel leaves at once)
//   init(mem, alphabetSize, lane)   the model of a block, as lib/BWTC.js:196-198 builds it over alphabetSize + 1 symbols
//   decode(D)              the next symbol (wave-uniform); end-of-input and damage are reported through D.in.eof
#pragma once
#include "pipeline.h"

#define K12_TOP 0x80000000u            // Top_value    lib/RangeCoder.js:15
#define K12_BOTTOM (K12_TOP >> 8)      // Bottom_value :18
#define K12_NVAL_MAX (1ull << 50)      // a declared size beyond this is left to the host path (which computes it as the reference does, in a double)
#define K12_E_MAGIC (-30)
#define K12_E_CORRUPT (-31)

__device__ __forceinline__ u32 k12_fls(u32 v) { return v ? 32u - (u32)__clz((int)v) : 0u; }     // lib/Util.js:301

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

// Util.decompressFileHelper (lib/Util.js:143-166) and lib/BWTC.js:142-146, in bwtc_decode's order of checks: 0 (a stream with
// its size declared, of levels 6-9, or of levels 1-5 where `opt` has K12_OPT_DEFSUM: the coder stands behind the level byte), -30,
// -31 or K12_HOST.  *declared as the single call reports it.
template <class R> __device__ __forceinline__ int k12_header(K12Dec<R>& D, long long* declared, u32* level, u32 opt) {
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
    if (nval == 0u) return K12_HOST;                           // no size declared
    if (lv <= 5u && !(opt & K12_OPT_DEFSUM)) return K12_HOST;  // DefSumModel (:146), unless the call asks for it on the device
    return 0;
}

template <class Model> __device__ __forceinline__ void k12_decode_body(const K12Plan& Q) {
    __shared__ u32 mem[Model::WORDS];
    __shared__ u16 useTree[512];
    __shared__ u8 M[256];
    const u32 d = blockIdx.x, lane = threadIdx.x;
    const K12Doc doc = Q.doc[d];
    if (doc.status != 0 || !Model::mine(doc.level)) return;    // decided by the plan; the other kernel's document
    K12Dec<K12Window> D;
    D.in.open(Q.in + Q.off[d], Q.off[d + 1u] - Q.off[d]);
    long long declared;
    u32 level;
    int status = k12_header(D, &declared, &level, Q.opt);     // (the plan's answer again: 0; the coder now stands behind the level byte)
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
        Model m;                                               // :196-198
        m.init(mem, alphabetSize, lane);
        u8* out = scr + place;
        u32 val = 1u, i = 0u;
        while (i < length) {                                   // :200-223, the MTF decode applied as the symbols come
            const u32 c = m.decode(D);
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
