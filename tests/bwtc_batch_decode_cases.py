"""Document sets and checkers of the batched BWTC decode tests (tests/test_emu_bwtc_batch_decode.py on the CPU logic build,
tests/test_gpu_bwtc_batch_decode.py on the GPU).  No stored streams: a test compresses with the existing batch or single call
(their output is pinned to the reference by the digests of golden_bwtc.json / golden.json), then decodes.  The arbiter for a
decoded document is the input itself; for a damaged stream it is cjs_bwtc_decompress on that document alone, same build.
Everything here takes the ctypes library and a context handle, so both builds share it; `mem` makes the buffers of the device
form ("host": numpy, for the CPU build where host memory serves as device memory; "torch": CUDA tensors)."""
import ctypes as C

import numpy as np

import bwtc_cases


def _u8(d):
    return np.ascontiguousarray(np.frombuffer(d, dtype=np.uint8) if isinstance(d, (bytes, bytearray)) else d, dtype=np.uint8).reshape(-1)


def pack(streams):
    """-> (flat uint8, off uint64[count + 1])"""
    arrs = [_u8(s) for s in streams]
    off = np.zeros(len(arrs) + 1, np.uint64)
    if arrs:
        off[1:] = np.cumsum([a.size for a in arrs], dtype=np.uint64)
    flat = np.concatenate(arrs) if int(off[-1]) else np.zeros(0, np.uint8)
    return np.ascontiguousarray(flat), off


# ---- making streams (existing entries) -----------------------------------------------------------------
def compress_many(L, h, docs, level):
    flat, off = pack(docs)
    cap = int(L.cjs_bwtc_compress_batch_bound(int(off[-1]), len(docs)))
    out = np.zeros(cap, np.uint8)
    oo = np.zeros(len(docs) + 1, np.uint64)
    n = L.cjs_bwtc_compress_batch(h, flat.ctypes.data if flat.size else None, off.ctypes.data, len(docs), level, out.ctypes.data, cap, oo.ctypes.data)
    assert n > 0, n
    return [out[int(oo[k]):int(oo[k + 1])].tobytes() for k in range(len(docs))]


def compress_one(L, h, doc, level, declared=None):
    d = _u8(doc)
    cap = int(L.cjs_bwtc_compress_bound(d.size))
    out = np.zeros(cap, np.uint8)
    n = L.cjs_bwtc_compress(h, d.ctypes.data, d.size, level, out.ctypes.data, cap, d.size if declared is None else declared)
    assert n > 0, n
    return out[:n].tobytes()


def single(L, h, stream):
    """cjs_bwtc_decompress on one document -> (status, bytes, declared)"""
    s = _u8(stream)
    declared = C.c_int64(-1)
    n = L.cjs_bwtc_decompress(h, s.ctypes.data if s.size else None, s.size, None, 0, C.byref(declared))
    if n == -21:
        n = int(L.cjs_bwtc_last_size(h))
        out = np.zeros(n, np.uint8)
        assert L.cjs_bwtc_fetch(h, out.ctypes.data, n) == n
        return 0, out.tobytes(), int(declared.value)
    assert n in (0, -30, -31), n
    return int(n), b"", int(declared.value)


# ---- one batch call --------------------------------------------------------------------------------------
class Result:
    def __init__(self, ret, out_off, status, declared, docs):
        self.ret, self.out_off, self.status, self.declared, self.docs = ret, out_off, status, declared, docs


def run_batch(L, h, streams, device=False, cap=None, mem="host", with_declared=True):
    """One call; every buffer is pre-filled with stale values.  cap None: the output gets exactly the room it needs - a first
    call with no room (-21), then the bytes through cjs_bwtc_last_size / cjs_bwtc_fetch, then the call again with the exact cap,
    which must give the same."""
    flat, off = pack(streams)
    n = len(streams)

    def call(room):
        out_off = np.full(n + 1, 0xEEEE, np.uint64)
        status = np.full(n, 77, np.int32)
        declared = np.full(n, -777, np.int64)
        out = np.full(room + 8, 0xAA, np.uint8)
        if device and mem == "torch":
            import torch
            t_in = torch.from_numpy(flat if flat.size else np.zeros(1, np.uint8)).cuda()
            t_off = torch.from_numpy(off.astype(np.int64)).cuda()
            t_out = torch.from_numpy(out).cuda()
            t_oo = torch.from_numpy(out_off.astype(np.int64)).cuda()
            t_st = torch.from_numpy(status).cuda()
            t_de = torch.from_numpy(declared).cuda()
            ret = L.cjs_bwtc_decompress_batch_device(h, t_in.data_ptr() if flat.size else None, t_off.data_ptr(), n, t_out.data_ptr(), room,
                                                     t_oo.data_ptr(), t_st.data_ptr(), t_de.data_ptr() if with_declared else None)
            torch.cuda.synchronize()
            out, out_off, status, declared = t_out.cpu().numpy(), t_oo.cpu().numpy().astype(np.uint64), t_st.cpu().numpy(), t_de.cpu().numpy()
        else:
            fn = L.cjs_bwtc_decompress_batch_device if device else L.cjs_bwtc_decompress_batch
            ret = fn(h, flat.ctypes.data if flat.size else None, off.ctypes.data, n, out.ctypes.data, room, out_off.ctypes.data,
                     status.ctypes.data, declared.ctypes.data if with_declared else None)
        assert (out[room:] == 0xAA).all(), "bytes written beyond out_cap"
        return ret, out, out_off, status, declared

    if cap is None:
        ret, _out, out_off, status, declared = call(0)
        total = int(out_off[-1])
        if total == 0:
            assert ret == 0, ret
            return Result(0, out_off, status, declared, [b""] * n)
        assert ret == -21 and int(L.cjs_bwtc_last_size(h)) == total, (ret, total)
        kept = np.full(total, 0xAA, np.uint8)
        assert L.cjs_bwtc_fetch(h, kept.ctypes.data, total) == total
        ret2, out, oo2, st2, de2 = call(total)
        assert ret2 == total and oo2.tolist() == out_off.tolist() and st2.tolist() == status.tolist(), (ret2, total)
        if with_declared:
            assert de2.tolist() == declared.tolist()
        assert out[:total].tobytes() == kept.tobytes(), "the retained result differs from the delivered one"
        ret = total
    else:
        ret, out, out_off, status, declared = call(cap)
        if ret < 0:
            return Result(ret, out_off, status, declared, None)
    assert int(out_off[0]) == 0 and int(out_off[-1]) == ret
    assert all(int(out_off[k]) <= int(out_off[k + 1]) for k in range(n))
    return Result(ret, out_off, status, declared, [out[int(out_off[k]):int(out_off[k + 1])].tobytes() for k in range(n)])


def check_inputs(r, docs, tag=""):
    """every document decoded to its input"""
    assert r.ret >= 0 and len(r.docs) == len(docs), (tag, r.ret)
    for k, d in enumerate(docs):
        assert int(r.status[k]) == 0 and r.docs[k] == _u8(d).tobytes(), (tag, k, int(r.status[k]), len(r.docs[k]), _u8(d).size)


def check_vs_single(L, h, r, streams, tag=""):
    """every document: the single call's outcome on that document alone - status, bytes and declared size.  -> [(status, bytes)]"""
    assert r.ret >= 0 and len(r.docs) == len(streams), (tag, r.ret)
    want = []
    for k, s in enumerate(streams):
        st, data, decl = single(L, h, s)
        assert int(r.status[k]) == st and r.docs[k] == data, (tag, k, int(r.status[k]), st, len(r.docs[k]), len(data))
        assert int(r.declared[k]) == decl, (tag, k, int(r.declared[k]), decl)
        want.append((st, data))
    return want


def fallbacks(L, h):
    return int(L.cjs_dbg_bwtc_dec_batch_fallbacks(h))


def syncs(L, h):
    return int(L.cjs_dbg_bwtc_dec_batch_syncs(h))


# ---- the sets --------------------------------------------------------------------------------------------
def fuzz_of_level(level, max_size=None):
    """-> ([case numbers], [documents]) of bwtc_cases.case(i) with that level"""
    ids, docs = [], []
    for i in range(bwtc_cases.N_SMALL):
        d, lv = bwtc_cases.case(i)
        if lv == level and (max_size is None or d.size <= max_size):
            ids.append(i)
            docs.append(d)
    return ids, docs


TREE_SHAPES = (1, 2, 3, 4, 127, 128, 129, 254, 255, 256)


def tree_shape_docs():
    """alphabets of k symbols, 700 shuffled bytes each: numSyms = k + 2 is mostly no power of two, so the walk's leaf order wraps"""
    rng = np.random.RandomState(4242)
    return [rng.permutation(np.resize(np.arange(k), 700)).astype(np.uint8) for k in TREE_SHAPES]


def runs_and_ends_docs():
    """empty documents in first, middle and last place; 1 byte; a x 1000; 30 000 zeros (the run doubles up to the block's end); a
    document that ends inside a run"""
    rng = np.random.RandomState(77)
    e = np.zeros(0, np.uint8)
    tail_run = np.concatenate([rng.randint(0, 256, size=500), np.full(777, 122)]).astype(np.uint8)
    return [e, np.array([120], np.uint8), np.full(1000, 97, np.uint8), e, np.zeros(30000, np.uint8), tail_run, e]


def alignment_streams(valid):
    """the same valid stream behind fillers of 0..7 bytes of garbage: [garbage_0, valid, garbage_1, valid, ...]"""
    rng = np.random.RandomState(8)
    out = []
    for f in range(8):
        out.append(rng.randint(0, 256, size=f).astype(np.uint8).tobytes())
        out.append(valid)
    return out


def flip(s, bit):
    b = bytearray(s)
    b[bit >> 3] ^= 0x80 >> (bit & 7)
    return bytes(b)


def isolation_streams(streams):
    """12 streams in, three of them damaged: a truncation by 13 bytes, a flipped bit in the magic, a flipped bit mid-stream"""
    s = list(streams[:12])
    assert len(s) == 12 and all(len(x) > 40 for x in (s[2], s[5], s[9]))
    s[2] = s[2][:len(s[2]) - 13]
    s[5] = flip(s[5], 13)
    s[9] = flip(s[9], (len(s[9]) // 2) * 8 + 3)
    return s


def sweep_streams(streams, seed=5):
    """per stream six single-bit flips at seeded places (the first inside the magic or the size) and cuts of 1, 2, 3, 5, 9 and
    len / 2 bytes -> [(kind, damaged stream, original index)]"""
    rng = np.random.RandomState(seed)
    out = []
    for k, s in enumerate(streams):
        for j in range(6):
            bit = int(rng.randint(0, 48)) if j == 0 else int(rng.randint(0, len(s) * 8))
            out.append(("flip", flip(s, bit), k))
        for cut in (1, 2, 3, 5, 9, len(s) // 2):
            out.append(("cut", s[:len(s) - cut], k))
    return out


def outcome_classes(want, originals, sweep):
    """-> set of the outcomes in the sweep: -30, -31, 'same' (decodes to the input), 'other' (decodes without error to other bytes)"""
    seen = set()
    for (st, data), (_kind, _s, k) in zip(want, sweep):
        seen.add(st if st else ("same" if data == originals[k] else "other"))
    return seen


# ---- cjs_unbwt_linear_batch ------------------------------------------------------------------------------
def unbwt_batch(L, blocks, pidxs):
    """-> (return value, [text of every block]); the output is pre-filled with stale bytes"""
    flat, off = pack(blocks)
    pidx = np.ascontiguousarray(np.asarray(pidxs, dtype=np.uint32))
    out = np.full(flat.size + 8, 0xAA, np.uint8)
    rc = L.cjs_unbwt_linear_batch(flat.ctypes.data if flat.size else None, off.ctypes.data, pidx.ctypes.data, len(blocks), out.ctypes.data)
    assert (out[flat.size:] == 0xAA).all()
    return rc, [out[int(off[k]):int(off[k + 1])].tobytes() for k in range(len(blocks))]


UNBWT_SIZES = (0, 1, 2, 63, 64, 65, 4095, 4096, 4097, 100000)


def check_unbwt_batch(L, golden):
    """the three sets of the issue, each in ONE call: real BWTs of the boundary sizes; the (T, pidx) pairs of cases.UNBWT_CASES
    that are no BWT at all, against the oracle and the reference-made digests; random pairs over two symbols; pidx = 0, n, > n"""
    import hashlib

    import cases
    import oracle
    from compressjs_amd import synth
    texts = [synth.text_like(n, 3 + n % 7) if n else np.zeros(0, np.uint8) for n in UNBWT_SIZES]
    pairs = [oracle.bwt_linear(t) if t.size else (np.zeros(0, np.uint8), 0) for t in texts]
    rc, got = unbwt_batch(L, [np.ascontiguousarray(u) for u, _p in pairs], [p for _u, p in pairs])
    assert rc == 0
    for t, g in zip(texts, got):
        assert g == t.tobytes(), t.size
    blocks, pidxs, keys = [], [], []
    for cid, ps in cases.UNBWT_CASES.items():
        for p in ps:
            blocks.append(np.ascontiguousarray(cases.case_input(cid), dtype=np.uint8))
            pidxs.append(p)
            keys.append("%s:unbwt:%d" % (cid, p))
    rc, got = unbwt_batch(L, blocks, pidxs)
    assert rc == 0
    for b, p, k, g in zip(blocks, pidxs, keys, got):
        assert g == oracle.unbwt_linear(b, p).tobytes(), k
        assert hashlib.sha256(g).hexdigest() == golden[k]["u_sha256"], k
    rng = np.random.RandomState(300)
    blocks = [rng.randint(0, 2, size=300).astype(np.uint8) for _ in range(24)]
    pidxs = [int(rng.randint(0, 301)) for _ in range(22)] + [0, 300]
    rc, got = unbwt_batch(L, blocks, pidxs)
    assert rc == 0
    for b, p, g in zip(blocks, pidxs, got):
        assert g == oracle.unbwt_linear(b, p).tobytes(), p
    assert unbwt_batch(L, blocks[:3], [5, 301, 7])[0] == -22                     # pidx > n
    assert unbwt_batch(L, [], [])[0] == 0
