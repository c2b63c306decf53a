// K14: the decoder of BWTC levels 1..5 on the GPU, ONE WAVE PER DOCUMENT of a batch (cjs_bwtc_decompress_batch_ex* with
// CJS_BWTC_DEC_DEFSUM_DEVICE).  It is K12 with DefSumModel in FenwickModel's place: the byte window, the range decoder, the
// header, the block loop, the use tree, the alphabet ballot, the RUNA / RUNB fill, the MTF shift and the row and status writes are
// k12_decode_body of k12_dec.h, and this file is the model alone - the decode side of lib/DefSumModel.js:11-131, built per block as
// DefSumModel(decoder, alphabetSize + 1, true) (lib/BWTC.js:198-200).  The host's restatement, which the single call and the batch's
// host path run, is DefSum / defsum_decode of bwtc_host.hip.
//
// State: prob[], escape[] and update[] (numSyms + 2 <= 259 entries, K13_TAB u32 each) in LDS; updateCount, updateThresh and
// update[ESCAPE] are wave-uniform scalars, as in K13.  ESCAPE = numSyms = alphabetSize + 1.
//
// decode (:116-137): p = culShift(8), the symbol s whose interval holds p, update(prob[s+1] - prob[s], prob[s], 256), _update(s);
// if s is ESCAPE: tot_f = escape[numSyms], k = culFreq(tot_f), the dead symbol whose escape interval holds k, update, _update.
//
// Finding the symbol - NO TABLE.  The reference keeps probToSym[256] / escProbToSym[] and rewrites them after every rebuild.
// probToSym[j] is the largest i with prob[i] <= j, escProbToSym[k] the largest i <= numSyms with escape[i] <= k (escape[numSyms] =
// tot_f > k, so the result is a symbol below ESCAPE); before the first rebuild the tables are all ESCAPE and k -> k, the same
// functions of the initial arrays (prob = 0 up to ESCAPE, escape[i] = i).  Both arrays are nondecreasing, so "the largest i with
// a[i] <= x" is (the number of entries <= x) - 1.  Each lane holds entries lane, 64 + lane, ... of prob[] and of escape[] in five
// registers each (entries beyond numSyms read as 0xFFFF, never counted), reloaded after a rebuild (10 LDS reads every 88-176
// symbols), and a lookup is five compares with a ballot and a population count each.  The lookup itself makes no LDS round trip:
// the one left on the symbol's dependency chain is the read of prob[s] and prob[s + 1] (a table would add a second, dependent one
// in front of it); there is no table to rewrite wave-wide after every rebuild (256 + up to 258 entries), and the two u16 tables'
// ~1 kB of LDS is not needed.  prob[s] and prob[s + 1] are two adjacent LDS reads at a uniform address.  The table variant was
// not built; no A/B was run.
//
// _update (:40-52) is serial here - the decoder learns one symbol at a time, K13's chunks of 64 do not apply - and keeps both
// escape rules: update[ESCAPE] stops at 40, and the escape that meets updateCount >= updateThresh - 1 is refused.  The rebuild
// (:54-80) is K13's wave-wide loop, k13_rebuild.
//
// Guards (the single call is the arbiter for damaged streams; D.in.eof is what the host's rc.eof is): tot_f == 0 on an escape is
// end-of-input and never reaches culFreq's division; help == 0 in culShift / culFreq (K12Dec); c - 1 >= alphabetSize, a run longer
// than what is left of the block, length && alphabetSize == 0 (k12_decode_body).  The host's index clamps (p & 255, min(k, 303)) are
// no-ops for what culShift(8) and culFreq(tot_f <= 258) return; here p <= 255 and k < tot_f index nothing: they are compared.
// The counts cannot leave the arrays: prob[0] = escape[0] = 0 always counts (s >= 0), entries beyond numSyms never do, so
// s <= numSyms and s + 1 <= 258 < K13_TAB.
//
// Termination: every byte read moves `pos` towards the stream's end, beyond it every decode reports end-of-input and the symbol
// loop leaves; the symbol loop is bounded by the block's length, the block loop by the document's rows, the use tree by 511,
// the rebuild by size + 1 <= 258 entries (five rounds), a lookup by its five rounds; the run and MTF loops as in K12.
// All control flow is wave-uniform; no per-lane arrays indexed at run time (no scratch memory).
#include "k12_dec.h"
#include "k13_rebuild.h"

struct K14DefSum {
    static constexpr u32 WORDS = 3u * K13_TAB;
    u32 *prob, *esc, *upd;
    u32 size, lane;                    // ESCAPE = numSyms = size
    u32 uc, th, uesc;                  // updateCount, updateThresh, update[ESCAPE]
    u32 pr[5], er[5];                  // prob[r * 64 + lane], escape[r * 64 + lane] (constant indices only: registers)
    u64 lt_lanes;
    __device__ static __forceinline__ bool mine(u32 level) { return level <= 5u; }
    __device__ __forceinline__ void load() {
#pragma unroll
        for (u32 r = 0; r < 5u; r++) {
            const u32 i = r * 64u + lane;
            const bool v = i <= size;
            pr[r] = v ? prob[i] : 0xFFFFu;
            er[r] = v ? esc[i] : 0xFFFFu;
        }
    }
    __device__ __forceinline__ void init(u32* mem, u32 alphabetSize, u32 lane_) {                 // :11-37
        prob = mem; esc = mem + K13_TAB; upd = mem + 2u * K13_TAB;
        size = alphabetSize + 1u; lane = lane_;
        lt_lanes = lanemask_lt();
        __builtin_amdgcn_wave_barrier();
        for (u32 i = lane; i < K13_TAB; i += 64u) { prob[i] = i > size ? 256u : 0u; esc[i] = i; upd[i] = 0u; }
        __builtin_amdgcn_wave_barrier();
        uc = 0u; th = 128u; uesc = 0u;
        load();
    }
    // the largest i with a[i] <= x, a[] as the five registers hold it
    __device__ __forceinline__ u32 find(const u32 (&a)[5], u32 x) const {
        u32 n = 0u;
#pragma unroll
        for (u32 r = 0; r < 5u; r++) n += (u32)__popcll(__ballot(a[r] <= x));
        return n - 1u;
    }
    __device__ __forceinline__ void update(u32 s) {                                               // _update :40-80
        if (s == size) {
            if (uesc >= K13_MAX_ESC || uc >= th - 1u) return;
            uesc++;
        } else if (lane == 0) upd[s]++;
        uc++;
        if (uc < th) return;
        th = k13_rebuild(prob, esc, upd, size, uesc, lane, lt_lanes);
        uesc = 1u; uc = 1u;
        load();
    }
    __device__ __forceinline__ u32 decode(K12Dec<K12Window>& D) {                                 // :116-137
        const u32 p = D.culShift(8u);
        if (D.in.eof) return 0u;
        u32 s = find(pr, p);
        u32 lt_f = prob[s], sy_f = prob[s + 1u] - lt_f;
        D.update(sy_f, lt_f, 256u);
        update(s);
        if (s != size) return s;
        const u32 tot_f = esc[size];
        if (tot_f == 0u) { D.in.eof = true; return 0u; }       // no dead symbol is left: the escape cannot be followed
        const u32 k = D.culFreq(tot_f);
        if (D.in.eof) return 0u;
        s = find(er, k);
        lt_f = esc[s]; sy_f = esc[s + 1u] - lt_f;
        D.update(sy_f, lt_f, tot_f);
        update(s);
        return s;
    }
};

__global__ __launch_bounds__(64) void k14_decode(K12Plan Q) { k12_decode_body<K14DefSum>(Q); }

int k14_decode_run(K12Plan Q, hipStream_t stream) {
    hipLaunchKernelGGL(k14_decode, dim3(Q.count), dim3(64), 0, stream, Q);
    HIP_CHECK_RET(hipGetLastError());
    return CJS_OK;
}
