"""Batched BWTC decode on the MI355X (cjs_bwtc_decompress_batch / _batch_device): N streams in one call, every document as the single
call gives it for that stream alone - levels 6-9 by one range decoder per document on the GPU (k12_bwtc_decoder.hip) and the
batched inverse BWT (k6_unbwt_batch).  The streams are made by the existing compress entries and checked against the reference's
digests (tests/golden/golden_bwtc.json, golden.json); the arbiter of a decoded document is its input, of a damaged stream the
single call on the same build.  The sets are those of tests/test_emu_bwtc_batch_decode.py (tests/bwtc_batch_decode_cases.py)."""
import hashlib
import json
import os

import numpy as np
import pytest

import bwtc_batch_decode_cases as dc
import bwtc_cases

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def gbwtc():
    with open(os.path.join(ROOT, "tests", "golden", "golden_bwtc.json")) as f:
        return json.load(f)["vectors"]


@pytest.fixture(scope="module")
def ctx():
    from compressjs_amd.bzip2 import Context
    c = Context(0, 8)
    yield c
    c.close()


@pytest.fixture(scope="module")
def ctx2():
    from compressjs_amd.bzip2 import Context
    c = Context(0, 2)
    yield c
    c.close()


@pytest.fixture(scope="module")
def fuzz_streams(ctx, gbwtc):
    """level -> ([documents], [their streams]): all fuzz cases of levels 6-9 and 3, made by the batch compress and checked against
    the reference's digests"""
    by = {}
    for level in (3, 6, 7, 8, 9):
        ids, docs = dc.fuzz_of_level(level)
        streams = dc.compress_many(ctx.L, ctx.h, docs, level)
        for i, s in zip(ids, streams):
            assert hashlib.sha256(s).hexdigest() == gbwtc["fuzz%d" % i]["out_sha256"], i
        by[level] = (docs, streams)
    return by


@pytest.fixture(scope="module")
def small_streams(fuzz_streams):
    docs, streams = [], []
    for level in (6, 7, 8, 9):
        ds, ss = fuzz_streams[level]
        pick = [k for k in range(len(ds)) if 17 <= ds[k].size <= 1000][:8]
        docs += [ds[k].tobytes() for k in pick]
        streams += [ss[k] for k in pick]
    assert len(streams) >= 24
    return docs, streams


@pytest.mark.parametrize("level", (6, 7, 8, 9))
def test_all_fuzz_cases_of_a_level_as_one_batch(ctx, fuzz_streams, level):
    L, h = ctx.L, ctx.h
    docs, streams = fuzz_streams[level]
    assert len(docs) >= 20
    r = dc.run_batch(L, h, streams)
    dc.check_inputs(r, docs, level)
    assert dc.fallbacks(L, h) == 0 and dc.syncs(L, h) == 3
    assert [int(x) for x in r.declared] == [d.size for d in docs]
    r = dc.run_batch(L, h, streams, device=True, mem="torch")
    dc.check_inputs(r, docs, level)
    assert dc.fallbacks(L, h) == 0 and dc.syncs(L, h) == 3


def test_tree_shapes(ctx):
    L, h = ctx.L, ctx.h
    docs = dc.tree_shape_docs()
    r = dc.run_batch(L, h, dc.compress_many(L, h, docs, 7))
    dc.check_inputs(r, docs)
    assert dc.fallbacks(L, h) == 0


def test_runs_and_ends(ctx, golden):
    L, h = ctx.L, ctx.h
    docs = dc.runs_and_ends_docs()
    streams = dc.compress_many(L, h, docs, 9)
    assert streams[0].hex() == golden["empty:bwtc:9"]["out_hex"] and streams[2].hex() == golden["a1000:bwtc:9"]["out_hex"]
    for device in (False, True):
        r = dc.run_batch(L, h, streams, device=device, mem="torch")
        dc.check_inputs(r, docs)
        assert dc.fallbacks(L, h) == 0
    r = dc.run_batch(L, h, [streams[0]] * 3)
    assert r.ret == 0 and r.out_off.tolist() == [0, 0, 0, 0] and r.status.tolist() == [0, 0, 0]


def test_alignment_and_isolation(ctx, small_streams):
    L, h = ctx.L, ctx.h
    docs, streams = small_streams
    batch = dc.alignment_streams(streams[3])
    for device in (False, True):
        r = dc.run_batch(L, h, batch, device=device, mem="torch")
        dc.check_vs_single(L, h, r, batch)
        for k in range(1, 16, 2):
            assert int(r.status[k]) == 0 and r.docs[k] == docs[3], k
        assert r.status[0] == -30


def test_three_damaged_documents_among_twelve(ctx, small_streams):
    L, h = ctx.L, ctx.h
    docs, streams = small_streams
    batch = dc.isolation_streams(streams)
    for device in (False, True):
        r = dc.run_batch(L, h, batch, device=device, mem="torch")
        dc.check_vs_single(L, h, r, batch)
        assert int(r.status[5]) == -30 and int(r.status[2]) == -31
        for k in range(12):
            if k not in (2, 5, 9):
                assert int(r.status[k]) == 0 and r.docs[k] == docs[k], k


def test_sweep_of_flips_and_cuts_equals_the_single_call(ctx, small_streams):
    L, h = ctx.L, ctx.h
    docs, streams = small_streams
    sweep = dc.sweep_streams(streams)
    batch = [s for _kind, s, _k in sweep]
    r = dc.run_batch(L, h, batch)
    want = dc.check_vs_single(L, h, r, batch)
    assert dc.outcome_classes(want, docs, sweep) == {-30, -31, "same", "other"}


def test_host_path_documents_between_fast_ones(ctx, fuzz_streams):
    L, h = ctx.L, ctx.h
    d8, s8 = fuzz_streams[8]
    d3, s3 = fuzz_streams[3]
    doc = next(d for d in d8 if d.size >= 200)     # (longer than the 5 bytes one of the headers below declares)
    host = [(d3[k], s3[k]) for k in range(6)]
    host += [(doc, dc.compress_one(L, h, doc, 8, declared)) for declared in (-1, 0, 5, 1 << 40)]
    fast_more = dc.compress_one(L, h, doc, 8, doc.size + 1000)     # declares more than it holds: stays on the fast path
    docs, batch = [], []
    for k, (d, s) in enumerate(host):
        docs += [d8[k], d]
        batch += [s8[k], s]
    docs += [doc, d8[0]]
    batch += [fast_more, s8[0]]
    for device in (False, True):
        r = dc.run_batch(L, h, batch, device=device, mem="torch")
        dc.check_inputs(r, docs)
        assert dc.fallbacks(L, h) == len(host)
        dc.check_vs_single(L, h, r, batch)


@pytest.mark.parametrize("level,cids", ((6, ("gap1300k_l6", "rand1250k_l6")), (9, ("rand1850k_l9",))))
def test_multi_block_documents(ctx2, gbwtc, fuzz_streams, level, cids):
    """multi-block documents with small documents and an empty one around them, on a context of 2 blocks"""
    L, h = ctx2.L, ctx2.h
    big = {cid: (d, lv) for cid, d, lv in bwtc_cases.big_cases()}
    small, small_s = fuzz_streams[6]
    docs = [big[c][0] for c in cids] + [np.zeros(0, np.uint8)]
    streams = dc.compress_many(L, h, docs, level)
    for c, s in zip(cids, streams):
        assert hashlib.sha256(s).hexdigest() == gbwtc[c]["out_sha256"], c
    batch = [small_s[0], streams[0], streams[-1]] + list(streams[1:-1]) + [small_s[1]]
    want = [small[0], docs[0], docs[-1]] + docs[1:-1] + [small[1]]
    total = sum(w.size for w in want)
    dc.check_inputs(dc.run_batch(L, h, batch, cap=total), want, level)
    assert dc.fallbacks(L, h) == 0
    dc.check_inputs(dc.run_batch(L, h, batch, device=True, mem="torch", cap=total), want, level)


def test_call_level(ctx, small_streams, golden):
    import torch
    L, h = ctx.L, ctx.h
    docs, streams = small_streams
    batch = streams[:3]
    flat, off = dc.pack(batch)
    out = np.zeros(16384, np.uint8)
    oo, st = np.zeros(4, np.uint64), np.zeros(3, np.int32)
    bad = np.array([0, 40, 5, int(off[-1])], dtype=np.uint64)
    a = (flat.ctypes.data, off.ctypes.data, 3, out.ctypes.data, 16384, oo.ctypes.data, st.ctypes.data, None)
    t = [torch.from_numpy(x).cuda() for x in (flat, off.astype(np.int64), out, oo.astype(np.int64), st, bad.astype(np.int64))]
    b = (t[0].data_ptr(), t[1].data_ptr(), 3, t[2].data_ptr(), 16384, t[3].data_ptr(), t[4].data_ptr(), None)
    for fn, a, badp in ((L.cjs_bwtc_decompress_batch, a, bad.ctypes.data), (L.cjs_bwtc_decompress_batch_device, b, t[5].data_ptr())):
        assert fn(None, *a) == -22
        assert fn(h, a[0], None, *a[2:]) == -22
        assert fn(h, *a[:5], None, a[6], None) == -22
        assert fn(h, *a[:6], None, None) == -22
        assert fn(h, None, *a[1:]) == -22                      # null `in` with bytes to read
        assert fn(h, a[0], badp, *a[2:]) == -22                # decreasing offsets
        assert fn(h, None, None, 0, None, 0, None, None, None) == 0
    total = sum(len(d) for d in docs[:3])
    for device in (False, True):
        short = dc.run_batch(L, h, batch, device=device, mem="torch", cap=total - 1)
        assert short.ret == -21 and int(short.out_off[-1]) == total and short.status.tolist() == [0, 0, 0]
        assert int(L.cjs_bwtc_last_size(h)) == total
        kept = np.zeros(total, np.uint8)
        assert L.cjs_bwtc_fetch(h, kept.ctypes.data, total) == total and kept.tobytes() == b"".join(docs[:3])
        exact = dc.run_batch(L, h, batch, device=device, mem="torch", cap=total)
        assert exact.ret == total and exact.docs == docs[:3]
    s = bytes.fromhex(golden["a1000:bwtc:9"]["out_hex"])
    assert dc.single(L, h, s) == (0, b"a" * 1000, 1000)
    sa = np.frombuffer(s, dtype=np.uint8)
    room = np.zeros(1000, np.uint8)
    assert L.cjs_bwtc_decompress(h, sa.ctypes.data, sa.size, room.ctypes.data, 1000, None) == 1000 and room.tobytes() == b"a" * 1000


def test_sync_count_does_not_grow_with_the_documents(ctx, small_streams):
    L, h = ctx.L, ctx.h
    _docs, streams = small_streams
    counts = []
    for k in (8, 200):
        batch = [streams[j % len(streams)] for j in range(k)]
        assert dc.run_batch(L, h, batch, device=True, mem="torch", cap=1 << 18).ret > 0
        assert dc.fallbacks(L, h) == 0
        counts.append(dc.syncs(L, h))
    assert counts[0] == counts[1] == 3


def test_unbwt_linear_batch(ctx, golden):
    dc.check_unbwt_batch(ctx.L, golden)


def test_decompress_files_api():
    from compressjs_amd import BWT, BWTC
    import oracle
    docs = [b"", b"hello hello", bytearray(b"a" * 1000), np.arange(300, dtype=np.uint8)]
    plain = [bytes(d) if not isinstance(d, np.ndarray) else d.tobytes() for d in docs]
    for lv in (9, 6, 2):
        streams = BWTC.compressFiles(docs, lv)
        assert BWTC.decompressFiles(streams) == plain
        assert BWTC.decompressFiles([bytearray(s) for s in streams]) == plain
        assert BWTC.decompressFiles([np.frombuffer(s, dtype=np.uint8) for s in streams]) == plain
    assert BWTC.decompressFiles([]) == []
    streams = BWTC.compressFiles(docs, 8)
    bad = [streams[1], b"bwtx" + streams[2][4:], streams[2], streams[3][:-9]]
    with pytest.raises(RuntimeError, match="Bad magic") as ei:
        BWTC.decompressFiles(bad)
    assert ei.value.index == 1
    res = BWTC.decompressFiles(bad, return_errors=True)
    assert res[0] == plain[1] and res[2] == plain[2]
    assert isinstance(res[1], RuntimeError) and res[1].index == 1
    for k in (1, 3):
        with pytest.raises(type(res[k])):
            BWTC.decompressFile(bad[k])
    assert res[3].index == 3
    t = np.frombuffer(b"the quick brown fox jumps over the lazy dog", dtype=np.uint8)
    u, p = oracle.bwt_linear(t)
    assert BWT.unbwtransform_many([u, np.zeros(0, np.uint8), u], [p, 0, p]) == [t.tobytes(), b"", t.tobytes()]
    assert BWT.unbwtransform_many([], []) == []
