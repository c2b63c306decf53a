"""cjs_bwtc_compress_batch on the CPU logic build (tests/emu): N documents in, N BWTC streams out, each bit-identical to the single
call on that document - the arbiter is the reference (tests/golden/golden_bwtc.json, golden.json).  A context of 2 blocks in
flight, so that documents cross sub-batches and the coder state of a document crosses k11_code launches.  Levels 6-9 run the
device range coder (k11_bwtc_coder.hip), levels 1-5 the host tail.  Not a parity claim for the GPU build
(tests/test_gpu_bwtc_batch.py is)."""
import hashlib
import json
import os

import numpy as np
import pytest

import batch_cases as bc
import bwtc_cases
import cases
import stagelib
from compressjs_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def emu_ctx():
    L = _lib.load(stagelib.build_emu())
    h = L.cjs_create(0, 2)
    assert h
    yield L, h
    L.cjs_destroy(h)


@pytest.fixture(scope="module")
def gbwtc():
    with open(os.path.join(ROOT, "tests", "golden", "golden_bwtc.json")) as f:
        return json.load(f)["vectors"]


def _batch(Lh, docs, level, cap=None, device=False):
    """-> (return value, out_off, [streams])"""
    L, h = Lh
    flat, off = bc.pack(docs)
    if cap is None:
        cap = int(L.cjs_bwtc_compress_batch_bound(int(off[-1]), len(docs)))
    out = np.full(cap + 8, 0xAA, np.uint8)              # stale bytes: the call must write every byte it returns
    out_off = np.full(len(docs) + 1, 0xEEEE, np.uint64)
    fn = L.cjs_bwtc_compress_batch_device if device else L.cjs_bwtc_compress_batch     # (host memory serves as device memory in this build)
    n = fn(h, flat.ctypes.data, off.ctypes.data, len(docs), level, out.ctypes.data, cap, out_off.ctypes.data)
    if n < 0:
        return n, out_off, None
    assert (out[cap:] == 0xAA).all()
    return n, out_off, [out[int(out_off[k]):int(out_off[k + 1])].tobytes() for k in range(len(docs))]


def _check_digests(Lh, docs, level, want, device=False):
    """want: golden entries (out_len, out_sha256) per document"""
    n, out_off, got = _batch(Lh, docs, level, device=device)
    assert n >= 0, n
    assert int(out_off[0]) == 0 and int(out_off[-1]) == n == sum(v["out_len"] for v in want)
    for k, (g, v) in enumerate(zip(got, want)):
        assert len(g) == v["out_len"] and hashlib.sha256(g).hexdigest() == v["out_sha256"], (k, docs[k].size, level)
    return got


@pytest.mark.parametrize("level", range(1, 10))
def test_fuzz_cases_of_a_level_as_one_batch_vs_reference(emu_ctx, gbwtc, level):
    ids, docs = [], []
    for i in range(bwtc_cases.N_SMALL):
        d, lv = bwtc_cases.case(i)
        if lv == level and d.size <= 6000:
            ids.append(i)
            docs.append(d)
    assert len(docs) >= 15
    _check_digests(emu_ctx, docs, level, [gbwtc["fuzz%d" % i] for i in ids])


def test_fuzz_cases_device_form(emu_ctx, gbwtc):
    for level in (3, 8):
        ids = [i for i in range(0, bwtc_cases.N_SMALL) if bwtc_cases.case(i)[1] == level and bwtc_cases.case(i)[0].size <= 1000][:8]
        _check_digests(emu_ctx, [bwtc_cases.case(i)[0] for i in ids], level, [gbwtc["fuzz%d" % i] for i in ids], device=True)


def test_empty_documents_everywhere(emu_ctx, golden):
    e = np.zeros(0, np.uint8)
    a1, a1000 = (np.ascontiguousarray(cases.case_input(c), dtype=np.uint8) for c in ("a1", "a1000"))
    ge, g1, g1000 = golden["empty:bwtc:9"], golden["a1:bwtc:9"], golden["a1000:bwtc:9"]
    got = _check_digests(emu_ctx, [e, a1, e, e, a1000, e], 9, [ge, g1, ge, ge, g1000, ge])
    assert got[0].hex() == ge["out_hex"] and got[1].hex() == g1["out_hex"] and got[4].hex() == g1000["out_hex"]
    n, out_off, got = _batch(emu_ctx, [e, e, e], 9)
    assert n == 30 and out_off.tolist() == [0, 10, 20, 30] and [g.hex() for g in got] == [ge["out_hex"]] * 3
    n, out_off, got = _batch(emu_ctx, [e, e, e], 2)             # (the host tail's empty documents)
    assert n == 30 and out_off.tolist() == [0, 10, 20, 30] and all(g[:5] == got[0][:5] and len(g) == 10 for g in got)
    L, h = emu_ctx
    assert L.cjs_bwtc_compress_batch(h, None, None, 0, 9, None, 0, None) == 0
    assert L.cjs_bwtc_compress_batch_device(h, None, None, 0, 9, None, 0, None) == 0


@pytest.mark.parametrize("cid", ["rand250k_l1", "rand250k_l2"])
def test_multi_block_documents_on_the_host_tail(emu_ctx, gbwtc, cid):
    big = {c: (d, lv) for c, d, lv in bwtc_cases.big_cases()}
    d, level = big[cid]
    small = [i for i in range(bwtc_cases.N_SMALL) if bwtc_cases.case(i)[1] == level and bwtc_cases.case(i)[0].size <= 1000][:4]
    assert len(small) == 4
    docs = [bwtc_cases.case(i)[0] for i in small[:2]] + [d] + [bwtc_cases.case(i)[0] for i in small[2:]]
    want = [gbwtc["fuzz%d" % i] for i in small[:2]] + [gbwtc[cid]] + [gbwtc["fuzz%d" % i] for i in small[2:]]
    _check_digests(emu_ctx, docs, level, want)
    L, h = emu_ctx
    assert L.cjs_last_block_count(h) == 4 + -(-d.size // (level * 100000))


def test_coder_state_carried_across_two_launches(emu_ctx):
    """A two-block level-6 document behind a small one: with 2 blocks in flight its blocks fall into two sub-batches, so its
    coder state waits in HBM between two k11_code launches.  Against the single call (about 20 s each on this build)."""
    from compressjs_amd import synth
    L, h = emu_ctx
    big = synth.text_like(600001, 9)
    n, out_off, got = _batch(emu_ctx, [bc._b(b"hello hello"), big], 6)
    assert n > 0 and L.cjs_last_block_count(h) == 3
    cap = int(L.cjs_bwtc_compress_bound(big.size))
    out = np.zeros(cap, np.uint8)
    m = L.cjs_bwtc_compress(h, big.ctypes.data, big.size, 6, out.ctypes.data, cap, big.size)
    assert m > 0 and got[1] == out[:m].tobytes()


def test_error_codes_and_levels_outside_1_to_9(emu_ctx, golden):
    L, h = emu_ctx
    docs = [bc._b(b"hello hello"), bc._b(b"world"), np.ascontiguousarray(cases.case_input("a1000"), dtype=np.uint8)]
    flat, off = bc.pack(docs)
    out = np.zeros(16384, np.uint8)
    oo = np.zeros(4, np.uint64)
    for fn in (L.cjs_bwtc_compress_batch, L.cjs_bwtc_compress_batch_device):
        assert fn(None, flat.ctypes.data, off.ctypes.data, 3, 9, out.ctypes.data, 16384, oo.ctypes.data) == -22
        assert fn(h, flat.ctypes.data, None, 3, 9, out.ctypes.data, 16384, oo.ctypes.data) == -22
        assert fn(h, flat.ctypes.data, off.ctypes.data, 3, 9, None, 16384, oo.ctypes.data) == -22
        assert fn(h, flat.ctypes.data, off.ctypes.data, 3, 9, out.ctypes.data, 16384, None) == -22
        assert fn(h, None, off.ctypes.data, 3, 9, out.ctypes.data, 16384, oo.ctypes.data) == -22
        bad = np.array([0, 11, 5, 1016], dtype=np.uint64)                 # decreasing offsets
        for level in (3, 9):
            assert fn(h, flat.ctypes.data, bad.ctypes.data, 3, level, out.ctypes.data, 16384, oo.ctypes.data) == -22
    for level in (4, 9):
        n, out_off, want = _batch(emu_ctx, docs, level)
        assert n > 0
        for device in (False, True):
            short, oo2, _ = _batch(emu_ctx, docs, level, cap=n - 1, device=device)
            assert short == -21 and oo2.tolist() == out_off.tolist()      # out_off complete all the same
            exact, oo3, got = _batch(emu_ctx, docs, level, cap=n, device=device)
            assert exact == n and got == want and oo3.tolist() == out_off.tolist()
    nine = _batch(emu_ctx, docs, 9)[2]
    assert hashlib.sha256(nine[2]).hexdigest() == golden["a1000:bwtc:9"]["out_sha256"]
    for level in (0, 12, -3):
        assert _batch(emu_ctx, docs, level)[2] == nine
        assert _batch(emu_ctx, docs, level, device=True)[2] == nine


def test_sync_count_does_not_grow_with_the_documents(emu_ctx):
    L, h = emu_ctx
    counts = []
    for k in (1, 40):
        docs = [bc._b(b"abracadabra" * (1 + j % 5)) for j in range(k)]
        assert _batch(emu_ctx, docs, 7, device=True)[0] > 0
        counts.append(L.cjs_dbg_bwtc_batch_syncs(h))
    assert counts[0] == counts[1] == 3


def test_single_call_unchanged_after_a_batch_call(emu_ctx, golden):
    L, h = emu_ctx
    d = np.ascontiguousarray(cases.case_input("bytes40"), dtype=np.uint8)
    assert _batch(emu_ctx, [d, d[:100]], 6)[0] > 0
    cap = int(L.cjs_bwtc_compress_bound(d.size))
    out = np.zeros(cap, np.uint8)
    m = L.cjs_bwtc_compress(h, d.ctypes.data, d.size, 6, out.ctypes.data, cap, d.size)
    assert out[:m].tobytes().hex() == golden["bytes40:bwtc:6"]["out_hex"]
    assert _batch(emu_ctx, [d], 6)[2][0].hex() == golden["bytes40:bwtc:6"]["out_hex"]
