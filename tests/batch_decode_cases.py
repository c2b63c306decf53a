"""Document sets and checkers of the batched-decode tests (tests/test_emu_batch_decode.py on the CPU logic build,
tests/test_gpu_batch_decode.py on the GPU): every document of a batch must come out as the single call - whose arbiter is
oracle.bz2_decompress, pinned to the reference by the suite - gives it for that document alone; for the catalogue of
decode_cases the arbiter is the reference-made record in tests/golden/golden_decode.json."""
import hashlib
import json
import os

import numpy as np

import oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DETAIL = {1: "bad magic", 2: "level out of range", 3: "initial position out of bounds"}


def pack(streams):
    """-> (flat uint8, off uint64[count + 1])"""
    off = np.zeros(len(streams) + 1, np.uint64)
    off[1:] = np.cumsum([len(s) for s in streams], dtype=np.uint64) if streams else 0
    flat = np.frombuffer(b"".join(bytes(s) for s in streams), dtype=np.uint8).copy() if int(off[-1]) else np.zeros(0, np.uint8)
    return flat, off


class Result:
    def __init__(self, ret, out_off, status, detail, docs):
        self.ret, self.out_off, self.status, self.detail, self.docs = ret, out_off, status, detail, docs


def run_batch(L, h, streams, ms, device=False, cap=None, with_detail=True):
    """One call; the buffers are pre-filled with stale values.  cap None: first a call with no room (-21), then the bytes through
    cjs_bz2_last_size / cjs_bz2_fetch - unless the batch decodes to nothing."""
    flat, off = pack(streams)
    n = len(streams)
    out_off = np.full(n + 1, 0xEEEE, np.uint64)
    status = np.full(n, 77, np.int32)
    detail = np.full(3 * n, 0xDDDD, np.uint32) if with_detail else None
    fn = L.cjs_bz2_decompress_batch_device if device else L.cjs_bz2_decompress_batch
    out = np.full(max(cap or 0, 1), 0xAA, np.uint8)
    ret = fn(h, flat.ctypes.data if flat.size else None, off.ctypes.data, n, int(ms), out.ctypes.data, cap or 0,
             out_off.ctypes.data, status.ctypes.data, detail.ctypes.data if with_detail else None)
    if ret == -21 and cap is None:
        total = int(L.cjs_bz2_last_size(h))
        assert total == int(out_off[-1]) > 0
        out = np.full(total, 0xAA, np.uint8)
        assert L.cjs_bz2_fetch(h, out.ctypes.data, total) == total
        ret = total
    if ret < 0:
        return Result(ret, out_off, status, detail, None)
    assert int(out_off[0]) == 0 and int(out_off[-1]) == ret
    assert all(int(out_off[k]) <= int(out_off[k + 1]) for k in range(n))
    docs = [out[int(out_off[k]):int(out_off[k + 1])].tobytes() for k in range(n)]
    return Result(ret, out_off, status, detail, docs)


def check_vs_oracle(r, streams, ms, tag=""):
    """Every document: the oracle's outcome on that document alone - bytes, or code, detail number and zero bytes."""
    assert r.ret >= 0, (tag, r.ret)
    for k, s in enumerate(streams):
        n, det, data, _tab = oracle.bz2_decompress(bytes(s), bool(ms))
        if n < 0:
            assert int(r.status[k]) == n and r.docs[k] == b"", (tag, k, int(r.status[k]), n, bytes(s).hex()[:200])
            if r.detail is not None:
                assert int(r.detail[3 * k]) == det, (tag, k, int(r.detail[3 * k]), det)
        else:
            assert int(r.status[k]) == 0 and r.docs[k] == data, (tag, k, int(r.status[k]), len(r.docs[k]), n, bytes(s).hex()[:200])
            if r.detail is not None:
                assert int(r.detail[3 * k]) == 0, (tag, k)


def golden_decode():
    with open(os.path.join(ROOT, "tests", "golden", "golden_decode.json")) as f:
        return json.load(f)["vectors"]


def check_vs_golden(r, ids, g, tag=""):
    """Every document against the reference-made record: ok / out_len / out_sha256, or error_code and the detail-to-message mapping
    of decode_check.check_stream."""
    assert r.ret >= 0, (tag, r.ret)
    for k, sid in enumerate(ids):
        v = g[sid]
        st, doc = int(r.status[k]), r.docs[k]
        if v["ok"]:
            assert st == 0 and len(doc) == v["out_len"], (tag, sid, st, len(doc), v)
            assert hashlib.sha256(doc).hexdigest() == v["out_sha256"], (tag, sid)
            continue
        assert st == v["error_code"] and doc == b"", (tag, sid, st, len(doc), v)
        det, got, want = (int(x) for x in r.detail[3 * k:3 * k + 3])
        exp = {**DETAIL, 4: "Bad block CRC (got %x expected %x)" % (got, want),
               5: "Bad stream CRC (got %x expected %x)" % (got, want)}.get(det)
        if exp:
            assert v["message"].endswith(": " + exp), (tag, sid, det, v["message"], exp)
        else:
            assert ": " not in v["message"], (tag, sid, det, v["message"])


def catalogue(max_len=None):
    """-> {multistream flag: ([ids], [streams])} of decode_cases.streams(), at most max_len bytes each"""
    import decode_cases
    by = {False: ([], []), True: ([], [])}
    for sid, s, ms in decode_cases.streams():
        if s is None or (max_len is not None and len(s) > max_len):
            continue
        by[bool(ms)][0].append(sid)
        by[bool(ms)][1].append(s)
    return by


def flip(s, bit):
    b = bytearray(s)
    b[bit >> 3] ^= 0x80 >> (bit & 7)
    return bytes(b)


def one_block(seed, n=600, level=9):
    """A valid one-block stream of n random letters."""
    return oracle.bz2_compress(np.random.RandomState(seed).randint(97, 123, size=n).astype(np.uint8), level)


def three_blocks():
    """Level 1, three blocks (the catalogue's lcg250000)."""
    import cases
    s = oracle.bz2_compress(cases.case_input("lcg250000"), 1)
    tab = oracle.bz2_decompress(s)[3]
    assert len(tab) == 3
    return s, tab


def isolation_set():
    """12 documents; 2, 5 and 11 are corrupt: a flipped block-CRC bit, a flipped stream-CRC bit in a three-block document whose
    SECOND block also has a bad CRC (the block CRC must win: the reference meets it first), a truncation."""
    docs = [one_block(100 + k, 300 + 97 * k, 1 + k % 9) for k in range(12)]
    docs[2] = flip(docs[2], 32 + 48 + 7)
    s3, tab = three_blocks()
    docs[5] = flip(flip(s3, tab[1][0] + 48 + 11), len(s3) * 8 - 3)
    docs[7] = s3                                   # (a valid multi-block document behind the corrupt one)
    docs[11] = docs[11][:len(docs[11]) - 13]
    return docs


def slot_batch_set():
    """About 150 one-block documents of at most 2 kB with two three-block level-1 documents placed so that their blocks are
    candidates 63-65 and 127-129 of the batch: with 16 (or 64) slots they lie across a slot batch boundary.  One document in
    every stretch of 16 is corrupt in a way that keeps its block on the chain (a flipped block-CRC or stream-CRC bit), so the
    candidate numbers stay what they are."""
    s3, _tab = three_blocks()
    docs = [one_block(1000 + k, 40 + (k * 131) % 1900, 1 + k % 9) for k in range(63)] + [s3]
    docs += [one_block(2000 + k, 40 + (k * 197) % 1900, 1 + k % 9) for k in range(61)] + [s3]
    docs += [one_block(3000 + k, 40 + (k * 211) % 1900, 1 + k % 9) for k in range(24)]
    for k in range(5, len(docs), 16):
        if len(docs[k]) < 4096:
            docs[k] = flip(docs[k], 32 + 48 + 9) if (k // 16) % 2 else flip(docs[k], len(docs[k]) * 8 - 9)     # (at most 7 padding bits behind the stream CRC)
    docs[-2] = docs[-2][:len(docs[-2]) - 9]
    return docs


def fuzz_batches(seed, batches, max_docs, exact=False):
    """-> yields (streams, multistream): 1..max_docs (exact: max_docs) documents from decode_fuzz.gen_input, mutate and
    concatenation"""
    import decode_fuzz
    rng = np.random.RandomState(seed)
    for _ in range(batches):
        docs = []
        for _k in range(max_docs if exact else int(rng.randint(1, max_docs + 1))):
            s = oracle.bz2_compress(decode_fuzz.gen_input(rng), int(rng.randint(1, 10)))
            if rng.randint(0, 4) == 0:
                s = s + oracle.bz2_compress(decode_fuzz.gen_input(rng), int(rng.randint(1, 10)))
            for _m in range(int(rng.randint(0, 3))):
                s = decode_fuzz.mutate(rng, s)
            docs.append(s)
        yield docs, bool(rng.randint(0, 2))
