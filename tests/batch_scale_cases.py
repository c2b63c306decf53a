"""Document sets, runners and checkers of the batch entries' scale tests (tests/test_gpu_batch_scale.py on the GPU,
tests/test_emu_batch_scale.py on the CPU logic build): the code that exists only for more than 1 024 documents, more than 64 block
slots in a sub-batch, more than one group of the batched inverse BWT, and offsets that do not start at 0.  The arbiters are the
oracle, the reference-made digests of tests/golden/ and the input bytes - never another call of the library.  pack / run_batch /
check_* of batch_cases, batch_decode_cases and bwtc_batch_decode_cases are used where they fit; the runners here add what those
lack: a prefix in front of off[0], and the device forms on CUDA tensors (`mem` = "torch") as well as on host memory ("host": the
CPU build, where host memory serves as device memory)."""
import hashlib
import json
import os

import numpy as np

import batch_decode_cases as bdc
import bwtc_batch_decode_cases as dc
import oracle

COUNT = 2500                     # ceil(2500 / 1024) = 3 documents per thread, the last run partial (2500 = 833 * 3 + 1), 190 threads idle
K6_COUNT = 66000                 # K6_GROUP_MAX = 65 535 blocks per group: 65 535 + 465


# ---- buffers of one call -----------------------------------------------------------------------------------
def _put(a, on_device):
    """-> (pointer, function that gives the array back after the call)"""
    if not on_device:
        return a.ctypes.data, lambda: a
    import torch
    same = {np.dtype(np.uint64): np.int64, np.dtype(np.uint32): np.int32}.get(a.dtype)
    t = torch.from_numpy(a.view(same) if same else a).cuda()
    return t.data_ptr(), lambda: t.cpu().numpy().view(a.dtype)


def _finish(on_device):
    if on_device:
        import torch
        torch.cuda.synchronize()


def with_prefix(items, prefix=b""):
    """-> (flat uint8 = prefix + the items back to back, off uint64[count + 1] with off[0] = len(prefix))"""
    flat, off = dc.pack(items)
    pre = np.frombuffer(bytes(prefix), dtype=np.uint8)
    flat = np.concatenate([pre, flat])
    if flat.size == 0:
        flat = np.zeros(1, np.uint8)
    return np.ascontiguousarray(flat), off + np.uint64(pre.size)


def prefix_for(first, n):
    """n bytes to put in front of a batch whose first document is `first`: they end in a run of the document's first byte (260 of
    them for n = 261), so a run that starts outside any document must not reach into it"""
    if n == 0:
        return b""
    c, other = int(first[0]), 2 if n < 200 else 1
    return bytes([c ^ 1] * other + [c] * (n - other))


# ---- the compress entries ----------------------------------------------------------------------------------
def compress(L, h, which, docs, level, device=False, mem="host", prefix=b""):
    """cjs_<which>_compress_batch (which = "bz2" / "bwtc") or its device form, ONE call, every buffer pre-filled with stale values
    -> (out_off uint64[count + 1], [streams])"""
    flat, off = with_prefix(docs, prefix)
    n = len(docs)
    cap = int(getattr(L, "cjs_%s_compress_batch_bound" % which)(int(off[-1]), n))
    on = device and mem == "torch"
    p_in, _keep_in = _put(flat, on)                                 # (the getters keep the tensors alive through the call)
    p_off, _keep_off = _put(off, on)
    p_out, get_out = _put(np.full(cap, 0xAA, np.uint8), on)
    p_oo, get_oo = _put(np.full(n + 1, 0xEEEE, np.uint64), on)
    fn = getattr(L, "cjs_%s_compress_batch%s" % (which, "_device" if device else ""))
    ret = fn(h, p_in, p_off, n, level, p_out, cap, p_oo)
    _finish(on)
    assert ret >= 0, (which, ret)
    out, oo = get_out(), get_oo()
    assert int(oo[0]) == 0 and int(oo[-1]) == ret and (oo[1:] >= oo[:-1]).all(), (which, ret, int(oo[0]), int(oo[-1]))
    return oo, [out[int(oo[k]):int(oo[k + 1])].tobytes() for k in range(n)]


def check_streams_exact(oo, got, want, tag=""):
    """every stream equals `want` (the oracle's), and out_off is their scan"""
    assert len(got) == len(want), tag
    for k, (g, w) in enumerate(zip(got, want)):
        assert g == w, (tag, k, len(g), len(w))
    assert oo.tolist() == np.concatenate([[0], np.cumsum([len(w) for w in want])]).tolist(), tag


_empty_cache = {}


def empty_stream(level):
    """the reference's BWTC stream of the empty input at that level (tests/golden/golden_bwtc_empty.json)"""
    if not _empty_cache:
        with open(os.path.join(bdc.ROOT, "tests", "golden", "golden_bwtc_empty.json")) as f:
            _empty_cache.update(json.load(f)["vectors"])
    return bytes.fromhex(_empty_cache["empty:bwtc:%d" % level]["out_hex"])


def check_bwtc_digests(got, ids, level, gbwtc, tag=""):
    """every stream against the reference: golden_bwtc.json["fuzz<i>" or a case name], or the reference's stream for empty input"""
    empty = empty_stream(level)
    assert len(got) == len(ids), tag
    for k, (g, i) in enumerate(zip(got, ids)):
        if i is None:
            assert g == empty, (tag, k, g.hex())
            continue
        v = gbwtc[i if isinstance(i, str) else "fuzz%d" % i]
        assert len(g) == v["out_len"] and hashlib.sha256(g).hexdigest() == v["out_sha256"], (tag, k, i, len(g), v["out_len"])


# ---- the decode entries ------------------------------------------------------------------------------------
def bz2_decode(L, h, streams, ms, cap, device=False, mem="host", prefix=b""):
    """cjs_bz2_decompress_batch or its device form, ONE call with room for `cap` bytes -> batch_decode_cases.Result"""
    flat, off = with_prefix(streams, prefix)
    n = len(streams)
    on = device and mem == "torch"
    p_in, _keep_in = _put(flat, on)                                 # (the getters keep the tensors alive through the call)
    p_off, _keep_off = _put(off, on)
    p_out, get_out = _put(np.full(cap + 8, 0xAA, np.uint8), on)
    p_oo, get_oo = _put(np.full(n + 1, 0xEEEE, np.uint64), on)
    p_st, get_st = _put(np.full(n, 77, np.int32), on)
    p_det, get_det = _put(np.full(3 * n, 0xDDDD, np.uint32), on)
    fn = L.cjs_bz2_decompress_batch_device if device else L.cjs_bz2_decompress_batch
    ret = fn(h, p_in, p_off, n, int(ms), p_out, cap, p_oo, p_st, p_det)
    _finish(on)
    assert ret >= 0, ret
    out, oo = get_out(), get_oo()
    assert (out[cap:] == 0xAA).all(), "bytes written beyond out_cap"
    assert int(oo[0]) == 0 and int(oo[-1]) == ret and (oo[1:] >= oo[:-1]).all()
    return bdc.Result(ret, oo, get_st(), get_det(), [out[int(oo[k]):int(oo[k + 1])].tobytes() for k in range(n)])


def bwtc_decode(L, h, streams, cap, device=False, mem="host", prefix=b""):
    """cjs_bwtc_decompress_batch or its device form, ONE call with room for `cap` bytes -> bwtc_batch_decode_cases.Result"""
    flat, off = with_prefix(streams, prefix)
    n = len(streams)
    on = device and mem == "torch"
    p_in, _keep_in = _put(flat, on)                                 # (the getters keep the tensors alive through the call)
    p_off, _keep_off = _put(off, on)
    p_out, get_out = _put(np.full(cap + 8, 0xAA, np.uint8), on)
    p_oo, get_oo = _put(np.full(n + 1, 0xEEEE, np.uint64), on)
    p_st, get_st = _put(np.full(n, 77, np.int32), on)
    p_de, get_de = _put(np.full(n, -777, np.int64), on)
    fn = L.cjs_bwtc_decompress_batch_device if device else L.cjs_bwtc_decompress_batch
    ret = fn(h, p_in, p_off, n, p_out, cap, p_oo, p_st, p_de)
    _finish(on)
    assert ret >= 0, ret
    out, oo = get_out(), get_oo()
    assert (out[cap:] == 0xAA).all(), "bytes written beyond out_cap"
    assert int(oo[0]) == 0 and int(oo[-1]) == ret and (oo[1:] >= oo[:-1]).all()
    return dc.Result(ret, oo, get_st(), get_de(), [out[int(oo[k]):int(oo[k + 1])].tobytes() for k in range(n)])


def check_packed(r, docs, tag=""):
    """every document decoded to its input, compared on the packed result: the offsets are the scan of the sizes, every status is
    0, and the bytes between out_off[0] and out_off[count] are the inputs back to back"""
    sizes = np.array([len(d) for d in docs], dtype=np.uint64)
    assert r.ret == int(sizes.sum()), (tag, r.ret)
    assert np.array_equal(r.out_off, np.concatenate([np.zeros(1, np.uint64), np.cumsum(sizes, dtype=np.uint64)])), tag
    assert not np.asarray(r.status).any(), (tag, np.nonzero(r.status)[0][:8])
    got = np.frombuffer(b"".join(r.docs), dtype=np.uint8)
    want = np.frombuffer(b"".join(bytes(d) for d in docs), dtype=np.uint8)
    assert got.size == want.size, tag
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, (tag, int(bad[0]))


# ---- set 1: bzip2, 2 500 documents ---------------------------------------------------------------------------
BZ2_SIZES = (0, 1, 2, 5, 17, 40, 90, 700)
BZ2_DAMAGED = tuple(range(48, COUNT, 97))


def bz2_docs():
    """2 500 documents of 0 .. 700 bytes, four kinds in rotation: random over three letters, one byte repeated (cycling over the same
    three letters, so neighbours end and start with the same byte), random bytes, "xy" tiled.  Empty documents first, last and in
    runs of five, two of the runs across a multiple of 1 024 (k0_docs_scan's chunks).  The documents of BZ2_DAMAGED are not empty."""
    rng = np.random.RandomState(2500)
    sizes = rng.choice(BZ2_SIZES, size=COUNT)
    sizes[0] = sizes[-1] = sizes[-2] = 0
    for at in (300, 1020, 2046):
        sizes[at:at + 5] = 0
    for k in BZ2_DAMAGED:
        if sizes[k] == 0:
            sizes[k] = 17
    docs = []
    for k, n in enumerate(int(x) for x in sizes):
        kind = k % 4
        if kind == 0:
            d = rng.randint(97, 100, size=n)
        elif kind == 1:
            d = np.full(n, 97 + (k // 4) % 3)
        elif kind == 2:
            d = rng.randint(0, 256, size=n)
        else:
            d = np.resize(np.array([120, 121]), n)
        docs.append(np.ascontiguousarray(d, dtype=np.uint8))
    return docs


def bz2_damage(streams):
    """every 97th stream damaged, in turn: a flipped block-CRC bit, a flipped stream-CRC bit, the last 9 bytes cut off"""
    s = list(streams)
    for j, k in enumerate(BZ2_DAMAGED):
        assert len(s[k]) > 14                                       # (a block in it)
        s[k] = (bdc.flip(s[k], 32 + 48 + 7), bdc.flip(s[k], len(s[k]) * 8 - 9), s[k][:len(s[k]) - 9])[j % 3]
    return s


# ---- set 2: BWTC, 2 500 documents ----------------------------------------------------------------------------
BWTC_EMPTY_AT = (0, 1023, 1024, COUNT - 1)


def bwtc_docs(level):
    """-> ([case number or None], [documents]): the fuzz cases of that level of at most 6 000 bytes, cycled up to 2 500, an empty
    document first, last and on both sides of the 1 024th"""
    ids0, docs0 = dc.fuzz_of_level(level, 6000)
    assert len(docs0) >= 10
    ids = [ids0[k % len(ids0)] for k in range(COUNT)]
    docs = [docs0[k % len(docs0)] for k in range(COUNT)]
    for k in BWTC_EMPTY_AT:
        ids[k], docs[k] = None, np.zeros(0, np.uint8)
    return ids, docs


def budget_for(docs):
    """-> (budget, p): a scratch budget of about half of what the batch needs (the declared sizes rounded up to 4), such that the
    admitted prefix has p documents, p no multiple of 3 (it ends inside one thread's run of the plan), and document p is not empty
    (so it does not fit)"""
    cum = np.concatenate([[0], np.cumsum([(len(d) + 3) & ~3 for d in docs])])
    p = int(np.searchsorted(cum, cum[-1] // 2))
    while p % 3 == 0 or len(docs[p]) == 0:
        p += 1
    return int(cum[p]), p


def admitted_prefix(docs, budget):
    """the admission rule of the batched decoder: the longest prefix of the documents whose sizes, each rounded up to 4, fit the budget"""
    cum = np.cumsum([(len(d) + 3) & ~3 for d in docs])
    return int(np.searchsorted(cum, budget, side="right"))


# ---- set 3: more than 64 slots ---------------------------------------------------------------------------------
def slot_docs(big_id, big_doc, before):
    """-> ([ids], [documents]): `before` one-block level-6 fuzz documents, the three-block document, small ones up to 110 blocks"""
    ids0, docs0 = dc.fuzz_of_level(6)
    assert all(0 < d.size <= 600000 for d in docs0)
    after = 110 - 3 - before
    ids = [ids0[k % len(ids0)] for k in range(before + after)]
    docs = [docs0[k % len(docs0)] for k in range(before + after)]
    return ids[:before] + [big_id] + ids[before:], docs[:before] + [big_doc] + docs[before:]


# ---- set 4: groups of the batched inverse BWT --------------------------------------------------------------------
def k6_groups(L):
    return int(L.cjs_dbg_k6_groups())


def tiny_blocks():
    """-> ([blocks], [pidx], [expected texts]) of 66 000 blocks of 1 .. 8 bytes: 40 BWTs (oracle.bwt_linear) and 10 random (T, pidx)
    pairs, cycled; the expected text of every pair is oracle.unbwt_linear's"""
    rng = np.random.RandomState(66)
    pairs, want = [], []
    for i in range(40):
        t = rng.randint(97, 101, size=1 + i % 8).astype(np.uint8)
        u, p = oracle.bwt_linear(t)
        assert oracle.unbwt_linear(u, p).tobytes() == t.tobytes()
        pairs.append((np.ascontiguousarray(u), p))
        want.append(t.tobytes())
    for i in range(10):
        n = 1 + (i * 3) % 8
        u, p = rng.randint(0, 3, size=n).astype(np.uint8), int(rng.randint(0, n + 1))
        pairs.append((u, p))
        want.append(oracle.unbwt_linear(u, p).tobytes())
    order = np.arange(K6_COUNT) % 50
    return [pairs[k][0] for k in order], [pairs[k][1] for k in order], [want[k] for k in order]


def large_blocks():
    """-> ([blocks], [pidx], [texts]): 32 blocks of 900 000 bytes (28.8 MB: the workspace of a group holds 29), text-like and random
    bytes in turn, a few small blocks between them"""
    from compressjs_amd import synth
    texts = [synth.text_like(900000, 41), np.random.RandomState(42).randint(0, 256, size=900000).astype(np.uint8)]
    small = [synth.text_like(n, 43) for n in (5, 64, 4097)]
    big_pairs = [oracle.bwt_linear(t) for t in texts]
    small_pairs = [oracle.bwt_linear(t) for t in small]
    blocks, pidxs, want = [], [], []
    for k in range(32):
        u, p = big_pairs[k % 2]
        blocks.append(u); pidxs.append(p); want.append(texts[k % 2])
        if k in (3, 27, 29):
            j = (3, 27, 29).index(k)
            blocks.append(small_pairs[j][0]); pidxs.append(small_pairs[j][1]); want.append(small[j])
    return blocks, pidxs, want


def check_unbwt(L, blocks, pidxs, want, prefix=b"", tag=""):
    """cjs_unbwt_linear_batch in ONE call; the packed texts compared with numpy; nothing written outside [off[0], off[count])"""
    flat, off = with_prefix(blocks, prefix)
    pidx = np.ascontiguousarray(np.asarray(pidxs, dtype=np.uint32))
    lo, hi = int(off[0]), int(off[-1])
    out = np.full(hi + 8, 0xAA, np.uint8)
    assert L.cjs_unbwt_linear_batch(flat.ctypes.data, off.ctypes.data, pidx.ctypes.data, len(blocks), out.ctypes.data) == 0, tag
    assert (out[:lo] == 0xAA).all() and (out[hi:] == 0xAA).all(), tag
    exp = np.concatenate([np.frombuffer(bytes(w), dtype=np.uint8) if not isinstance(w, np.ndarray) else w for w in want])
    assert exp.size == hi - lo, tag
    bad = np.nonzero(out[lo:hi] != exp)[0]
    assert bad.size == 0, (tag, int(bad[0]), int(np.searchsorted(off - off[0], bad[0], side="right")) - 1)
    return out[lo:hi]


def pinned_small_streams(L, h, gbwtc):
    """-> ([documents as bytes], [streams]): eight fuzz cases of 17 .. 1 000 bytes of each of the levels 6-9, compressed by the batch
    entry and checked against the reference's digests"""
    docs, streams = [], []
    for level in (6, 7, 8, 9):
        ids, ds = dc.fuzz_of_level(level, 1000)
        pick = [k for k in range(len(ds)) if ds[k].size >= 17][:8]
        ss = dc.compress_many(L, h, [ds[k] for k in pick], level)
        for k, s in zip(pick, ss):
            assert hashlib.sha256(s).hexdigest() == gbwtc["fuzz%d" % ids[k]]["out_sha256"], ids[k]
        docs += [ds[k].tobytes() for k in pick]
        streams += ss
    assert len(streams) >= 24
    return docs, streams


# ---- set 5: off[0] > 0 -----------------------------------------------------------------------------------------
PREFIXES = (0, 5, 261)
OFFSET_LEVEL = 7


def offset_docs():
    """-> ([case number or None], [documents]): four level-7 fuzz cases of at most 1 000 bytes and an empty document in third
    place; the first document begins with a run"""
    ids0, docs0 = dc.fuzz_of_level(OFFSET_LEVEL, 1000)
    first = next(k for k in range(len(docs0)) if docs0[k].size >= 8 and (docs0[k][:4] == docs0[k][0]).all())
    rest = [k for k in range(len(docs0)) if k != first and docs0[k].size >= 17][:3]
    assert len(rest) == 3
    ids = [ids0[first], ids0[rest[0]], None, ids0[rest[1]], ids0[rest[2]]]
    docs = [docs0[first], docs0[rest[0]], np.zeros(0, np.uint8), docs0[rest[1]], docs0[rest[2]]]
    return ids, docs


def check_offsets(L, h, gbwtc, forms, mem):
    """All four batch entries and cjs_unbwt_linear_batch with the documents behind a prefix of 0, 5 and 261 bytes that ends in the
    first document's first byte, the offsets shifted by the prefix length.  forms: (False,) the host forms, (False, True) the device
    forms as well.  Every result against its arbiter - the oracle's stream, the reference's digest, the input bytes - and equal
    to what the call without a prefix gave."""
    ids, docs = offset_docs()
    plain = [d.tobytes() for d in docs]
    total = sum(len(p) for p in plain)
    bz = [oracle.bz2_compress(d, 1) for d in docs]
    bz_in = bz[:1] + [b""] + bz[1:]                                 # an empty stream among them: "Not bzip data", no bytes
    first = {}
    for n in PREFIXES:
        for device in forms:
            tag = "prefix %d device %d" % (n, device)
            # bzip2 compress: the oracle's streams
            oo, got = compress(L, h, "bz2", docs, 1, device, mem, prefix_for(plain[0], n))
            check_streams_exact(oo, got, bz, tag)
            assert int(L.cjs_last_block_count(h)) == 4, tag
            # bzip2 decode: the oracle's outcome for every document
            r = bz2_decode(L, h, bz_in, False, total + 64, device, mem, prefix_for(bz_in[0], n))
            bdc.check_vs_oracle(r, bz_in, False, tag)
            assert int(r.status[1]) == -2 and r.ret == total, tag
            # BWTC compress: the reference's digests
            oo, got = compress(L, h, "bwtc", docs, OFFSET_LEVEL, device, mem, prefix_for(plain[0], n))
            check_bwtc_digests(got, ids, OFFSET_LEVEL, gbwtc, tag)
            key = ("bwtc", device)
            if n == 0:
                first[key] = (oo.tolist(), got)
            assert first[key] == (oo.tolist(), got), tag
            # BWTC decode: the inputs; an empty stream among them is "Bad magic" and gives no bytes
            streams = got[:1] + [b""] + got[1:]
            r = bwtc_decode(L, h, streams, total + 64, device, mem, prefix_for(streams[0], n))
            assert r.ret == total and [int(x) for x in r.status] == [0, -30, 0, 0, 0, 0], (tag, r.ret, r.status.tolist())
            assert r.docs == plain[:1] + [b""] + plain[1:], tag
            assert [int(x) for x in r.declared] == [len(plain[0]), -1] + [len(p) for p in plain[1:]], tag
            assert dc.fallbacks(L, h) == 0, tag
        # the batched inverse BWT: the texts
        pairs = [oracle.bwt_linear(d) if d.size else (np.zeros(0, np.uint8), 0) for d in docs]
        blocks = [np.ascontiguousarray(u) for u, _p in pairs]
        check_unbwt(L, blocks, [p for _u, p in pairs], docs, prefix_for(blocks[0].tobytes(), n), "unbwt prefix %d" % n)
