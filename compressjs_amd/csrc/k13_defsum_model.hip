// K13: the adaptive model of BWTC levels 1..5 on the GPU - DefSumModel (lib/DefSumModel.js:11-111; the host's restatement is
// DefSum in bwtc_host.hip), ONE WAVE per block, for the batched entries (cjs_bwtc_compress_batch*).
//
// K13 is to levels 1-5 what K10 is to levels 6-9: it reads what K2 left (P.A, P.pos, P.alpha) and writes, per block, the
// (sy_f, lt_f, tot_f) triples that k11_code feeds to RangeCoder.encodeFreq.  DefSumModel codes a live symbol with
// encodeShift(sy_f, lt_f, 8) (:99), which is encodeFreq(sy_f, lt_f, 256): range >> 8 = floor(range / 256), and
// (lt_f + sy_f) >> 8 != 0 is lt_f + sy_f >= 256 (lib/RangeCoder.js:79-100).  So a live symbol is one triple
// (prob[x+1] - prob[x], prob[x], 256), and a symbol whose probability is 0 is two: the escape symbol's, then
// (escape[x+1] - escape[x], escape[x], escape[numSyms]) (:104-109).  sy_f can be 256 (the escape symbol before the first rebuild).
//
// The model is DEFERRED: prob[] and escape[] change only when updateCount reaches updateThresh (_update :51-80), every 88-176
// symbols; in between - an EPOCH - a triple is a table lookup.  So the wave takes CHUNKS of up to 64 consecutive symbols, a
// lane each, that end where the epoch ends:
//   e_i   symbol i escapes under the tables of the chunk's start; E_i = escapes among lanes 0..i (a ballot);
//   the escape symbol's own update (:40-47) is ignored once update[ESC] has reached 40, so lanes 0..i were granted
//   g_i = min(E_i, 40 - update[ESC] at the chunk's start) of them, and updateCount after symbol i is t_i = uc + (i + 1) + g_i -
//   as long as the other rule, updateCount >= updateThresh - 1 (:46), has refused nothing.  It can refuse only the escape that
//   meets updateCount == updateThresh - 1; the escaped symbol's own update then makes it updateThresh and ends the epoch,
//   where t_i says updateThresh + 1.  t_i grows by 1 or 2 a lane, so in both cases the epoch ends at the FIRST lane with
//   t_i >= updateThresh (ballot, find-first), t_i > updateThresh there means one granted update too many, and an escape never
//   triggers the rebuild: both triples of an escaped symbol come from the same tables.
// Lane i writes its one or two triples at nout + i + E_(i-1); the update counts are LDS atomics (a symbol can repeat in a
// chunk).  The rebuild (:54-80) runs wave-wide over the numSyms + 1 <= 258 entries, 64 at a time: newProb = (p >> 1) + update,
// the cumulative probability from a DPP scan, the cumulative escape index and the odd count from ballots (k13_rebuild.h, which the
// decoder K14 calls too).
//
// Row capacity: a symbol gives at most two triples, so a block gives at most 2 * nsym, and nsym = pos - 1 <= stride.  The batch
// hands K13 the rows it hands K10, ostride = ocap = 2 * stride u32, which therefore always suffice; the check in front of every
// chunk (nout + 2 * symbols of the chunk <= ocap, exact: nout <= 2 * posn) can only fire for a caller with shorter rows, and
// then reports K10_OVERFLOW in ntri[b] instead of writing past the row.
//
// No per-lane arrays (no scratch memory); prob, escape and update sit in LDS (3 x 264 u32).
#include "pipeline.h"
#include "bwtc_host.h"
#include "k13_rebuild.h"
#include <string.h>
#include <vector>

#define K10_OVERFLOW 0xFFFFFFFFu

__global__ __launch_bounds__(64) void k13_defsum(const u16* A, u32 stride, const u32* pos, const u32* alpha, u32* sylt, u32* tot,
                                                 u32* ntri, u32 ostride, u32 ocap) {
    __shared__ u32 prob[K13_TAB], esc[K13_TAB], upd[K13_TAB];
    const u32 b = blockIdx.x, lane = threadIdx.x;
    const u32 nsym = pos[b] ? pos[b] - 1u : 0u;               // K2 appended bzip2's end-of-block symbol; BWTC has none
    const u32 size = (alpha[b] < 256u ? alpha[b] : 256u) + 1u;   // DefSumModel(coder, alphabetSize + 1)  lib/BWTC.js:107; ESCAPE = size
    const u16* sym = A + (size_t)b * stride;
    u32* osl = sylt + (size_t)b * ostride;
    u32* oto = tot + (size_t)b * ostride;
    // init :16-24
    for (u32 i = lane; i < K13_TAB; i += 64u) { prob[i] = i > size ? 256u : 0u; esc[i] = i; upd[i] = 0u; }
    __builtin_amdgcn_wave_barrier();
    u32 uc = 0u, th = 128u;                                   // updateCount, updateThresh
    u32 uesc = 0u;                                            // update[ESCAPE] (kept here, not in upd[])
    u32 nout = 0u, posn = 0u;                                 // triples emitted, symbols consumed (all uniform)
    const u64 lt_lanes = lanemask_lt();
    // the symbols of rows wbase / wbase + 64 in two registers, as in K10: a chunk starts anywhere in the first
    u32 wbase = 0;
    u32 r0 = lane < nsym ? sym[lane] : 0u, r1 = 64u + lane < nsym ? sym[64u + lane] : 0u;
    auto window = [&]() -> u32 {
        while (posn - wbase >= 64u) { wbase += 64u; r0 = r1; r1 = wbase + 64u + lane < nsym ? sym[wbase + 64u + lane] : 0u; }
        const u32 off = posn - wbase + lane;                  // 0 .. 126
        const u32 a0 = (u32)__shfl((int)r0, (int)(off & 63u)), a1 = (u32)__shfl((int)r1, (int)(off & 63u));
        return off < 64u ? a0 : a1;
    };
    u32 nxt = window();
    while (posn < nsym) {
        const u32 avail = nsym - posn < 64u ? nsym - posn : 64u;
        if (nout + 2u * avail > ocap) {                       // (wave-uniform)
            if (lane == 0) ntri[b] = K10_OVERFLOW;
            return;
        }
        const u32 x = nxt < size ? nxt : size - 1u;           // symbols lie in [0, alphabetSize]: the tables are never left
        const bool in = lane < avail;
        // encode :95-109 under the tables of the chunk's start
        const u32 p0 = prob[x], sy = prob[x + 1u] - p0;
        const u32 e0 = esc[x], e1 = esc[x + 1u] - e0, et = esc[size];
        const u32 pe = prob[size], se = prob[size + 1u] - pe;
        const bool e = in && sy == 0u;
        const u64 em = __ballot(e);
        const u32 Eprev = (u32)__popcll(em & lt_lanes);
        const u32 Einc = Eprev + (e ? 1u : 0u), room = K13_MAX_ESC - uesc;
        const u32 g = Einc < room ? Einc : room;              // escape updates granted up to this lane  :42
        const u32 t = uc + lane + 1u + g;                     // updateCount behind this lane's symbol
        const u64 endm = __ballot(in && t >= th);
        const u32 m = endm ? (u32)__ffsll((long long)endm) : avail;   // symbols of this chunk: up to the one that ends the epoch
        const u32 tl = (u32)__builtin_amdgcn_readlane((int)t, (int)(m - 1u));
        const u32 gl = (u32)__builtin_amdgcn_readlane((int)g, (int)(m - 1u));
        if (lane < m) {
            const u32 at = nout + lane + Eprev;
            if (e) {
                osl[at] = se | (pe << 16);          oto[at] = 256u;
                osl[at + 1u] = e1 | (e0 << 16);     oto[at + 1u] = et;
            } else {
                osl[at] = sy | (p0 << 16);          oto[at] = 256u;
            }
            atomicAdd(&upd[x], 1u);                           // :48
        }
        nout += m + (u32)__popcll(em & (m < 64u ? (1ull << m) - 1ull : ~0ull));
        posn += m;
        nxt = window();
        if (tl < th) { uc = tl; uesc += gl; continue; }       // :51 defer
        // the rebuild :54-80; the escape that met updateCount == updateThresh - 1 was refused  :46
        uesc += gl - (tl > th ? 1u : 0u);
        th = k13_rebuild(prob, esc, upd, size, uesc, lane, lt_lanes);
        uesc = 1u; uc = 1u;                                   // :79-80
    }
    if (lane == 0) ntri[b] = nout;
}

int k13_defsum_run(Pipe P, u32* sylt, u32* tot, u32* ntri, u32 ostride, u32 ocap, hipStream_t stream) {
    hipLaunchKernelGGL(k13_defsum, dim3(P.g.nb), dim3(64), 0, stream, (const u16*)P.A, P.g.stride, (const u32*)P.pos, (const u32*)P.alpha, sylt, tot, ntri, ostride, ocap);
    HIP_CHECK_RET(hipGetLastError());
    return CJS_OK;
}

// (tests) the model alone over nb rows of symbols: host pointers in and out.  on_host = 0: one K13 launch; on_host = 1: the same
// rows through DefSum::encode of bwtc_host.hip with a recorder in the range coder's place.
extern "C" int32_t cjs_dbg_defsum_triples(const uint16_t* sym, const uint32_t* nsym, const uint32_t* alpha, uint32_t nb, uint32_t stride,
                                          uint32_t* sylt, uint32_t* tot, uint32_t* ntri, uint32_t ostride, int on_host) {
    if (!nb) return CJS_OK;
    if (!sym || !nsym || !alpha || !sylt || !tot || !ntri || !stride) return CJS_E_ARG;
    for (u32 b = 0; b < nb; b++) {
        if (nsym[b] > stride || alpha[b] > 256u) return CJS_E_ARG;
        for (u32 i = 0; i < nsym[b]; i++) if (sym[(size_t)b * stride + i] > alpha[b]) return CJS_E_ARG;
    }
    if (on_host) {
        for (u32 b = 0; b < nb; b++)
            ntri[b] = bwtc_defsum_triples(sym + (size_t)b * stride, nsym[b], alpha[b], sylt + (size_t)b * ostride, tot + (size_t)b * ostride, ostride);
        return CJS_OK;
    }
    const size_t symB = ((size_t)nb * stride * 2 + 255) & ~(size_t)255, rowB = (size_t)nb * ostride * 4, nbB = ((size_t)nb * 4 + 255) & ~(size_t)255;
    char* d = nullptr;
    HIP_CHECK_RET(hipMalloc((void**)&d, symB + 3 * nbB + 2 * rowB + 256));
    Pipe P;
    memset(&P, 0, sizeof P);
    P.g.nb = nb; P.g.stride = stride;
    P.A = (u16*)d; P.pos = (u32*)(d + symB); P.alpha = (u32*)(d + symB + nbB);
    u32* d_ntri = (u32*)(d + symB + 2 * nbB);
    u32* d_sylt = (u32*)(d + symB + 3 * nbB);
    u32* d_tot = (u32*)(d + symB + 3 * nbB + rowB);
    std::vector<u32> hpos(nb);
    for (u32 b = 0; b < nb; b++) hpos[b] = nsym[b] + 1u;      // (K2 counts its end-of-block symbol)
    hipError_t e = hipMemcpy(P.A, sym, (size_t)nb * stride * 2, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(P.pos, hpos.data(), (size_t)nb * 4, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(P.alpha, alpha, (size_t)nb * 4, hipMemcpyHostToDevice);
    int rc = CJS_OK;
    if (e == hipSuccess) rc = k13_defsum_run(P, d_sylt, d_tot, d_ntri, ostride, ostride, (hipStream_t) nullptr);
    if (e == hipSuccess && !rc) e = hipMemcpy(ntri, d_ntri, (size_t)nb * 4, hipMemcpyDeviceToHost);
    if (e == hipSuccess && !rc && rowB) e = hipMemcpy(sylt, d_sylt, rowB, hipMemcpyDeviceToHost);
    if (e == hipSuccess && !rc && rowB) e = hipMemcpy(tot, d_tot, rowB, hipMemcpyDeviceToHost);
    (void)hipFree(d);
    return rc ? rc : (e == hipSuccess ? CJS_OK : CJS_E_HIP - (int)e);
}
