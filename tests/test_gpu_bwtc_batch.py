"""Batched BWTC on the MI355X (cjs_bwtc_compress_batch / _batch_device through compressjs_amd.bzip2): N documents in one call, every
stream bit-identical to the single call on that document, levels 6-9 coded by one range coder per document on the GPU
(k11_bwtc_coder.hip).  The arbiter is the reference: tests/golden/golden_bwtc.json (308 reference-made streams) and golden.json."""
import hashlib
import json
import os

import numpy as np
import pytest

import batch_cases as bc
import bwtc_cases
from compressjs_amd import synth

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
    c = Context(0, 2)                                  # sub-batches of 2 blocks: multi-block documents span them and k11_code launches
    yield c
    c.close()


@pytest.fixture(scope="module")
def fuzz():
    """level -> ([case numbers], [documents]): all 300 fuzz cases, grouped by their level"""
    by = {lv: ([], []) for lv in range(1, 10)}
    for i in range(bwtc_cases.N_SMALL):
        d, lv = bwtc_cases.case(i)
        by[lv][0].append(i)
        by[lv][1].append(d)
    return by


@pytest.fixture(scope="module")
def big():
    return {cid: (d, lv) for cid, d, lv in bwtc_cases.big_cases()}


def _device(c, docs, level):
    import torch
    flat, off = bc.pack(docs)
    cap = int(c.L.cjs_bwtc_compress_batch_bound(int(off[-1]), len(docs)))
    d_in = torch.from_numpy(flat).cuda()
    d_off = torch.from_numpy(off.astype(np.int64)).cuda()
    d_out = torch.full((cap,), 0xAA, dtype=torch.uint8, device="cuda")
    d_oo = torch.full((len(docs) + 1,), -1, dtype=torch.int64, device="cuda")
    n = c.bwtc_compress_many_device(d_in, d_off, d_out, d_oo, level)
    oo = d_oo.cpu().numpy()
    out = d_out[:n].cpu().numpy()
    assert int(oo[0]) == 0 and int(oo[-1]) == n
    return [out[int(oo[k]):int(oo[k + 1])].tobytes() for k in range(len(docs))]


def _against(got, want, what):
    assert len(got) == len(want)
    for k, (g, v) in enumerate(zip(got, want)):
        assert len(g) == v["out_len"] and hashlib.sha256(g).hexdigest() == v["out_sha256"], (what, k)


@pytest.mark.parametrize("level", range(1, 10))
def test_all_fuzz_cases_of_a_level_as_one_batch(ctx, gbwtc, fuzz, level):
    ids, docs = fuzz[level]
    assert len(docs) >= 20
    want = [gbwtc["fuzz%d" % i] for i in ids]
    _against(ctx.bwtc_compress_many(docs, level), want, level)
    if level >= 6:
        assert int(ctx.L.cjs_dbg_bwtc_batch_syncs(ctx.h)) == 4     # the device form's three and the download
    if level >= 6 or level == 3:
        _against(_device(ctx, docs, level), want, level)
        if level >= 6:
            assert int(ctx.L.cjs_dbg_bwtc_batch_syncs(ctx.h)) == 3


def test_multi_block_documents_level_6(ctx2, gbwtc, fuzz, big):
    ids, small = fuzz[6]
    docs = [small[0], big["gap1300k_l6"][0], np.zeros(0, np.uint8), big["rand1250k_l6"][0], small[1]]
    want = [gbwtc["fuzz%d" % ids[0]], gbwtc["gap1300k_l6"], None, gbwtc["rand1250k_l6"], gbwtc["fuzz%d" % ids[1]]]
    got = ctx2.bwtc_compress_many(docs, 6)
    assert ctx2.last_block_count == 1 + 3 + 0 + 3 + 1
    assert got[2] == ctx2.bwtc_compress(docs[2], 6)
    _against(got[:2] + got[3:], want[:2] + want[3:], "l6")
    for g, d in zip(got, docs):
        assert ctx2.bwtc_decompress(np.frombuffer(g, dtype=np.uint8)) == d.tobytes()
    assert _device(ctx2, docs, 6) == got


def test_multi_block_document_level_9(ctx2, gbwtc, golden, big):
    docs = [big["rand1850k_l9"][0], np.full(1000, 97, np.uint8)]
    got = ctx2.bwtc_compress_many(docs, 9)
    _against(got, [gbwtc["rand1850k_l9"], golden["a1000:bwtc:9"]], "l9")
    for g, d in zip(got, docs):
        assert ctx2.bwtc_decompress(np.frombuffer(g, dtype=np.uint8)) == d.tobytes()


def test_sixty_four_slices_equal_the_single_call():
    from compressjs_amd.bzip2 import Context
    ctx = Context(0, 32)                               # two streams, sub-batches of 16 blocks: four of them, two per workspace
    try:
        _sixty_four_slices(ctx)
    finally:
        ctx.close()


def _sixty_four_slices(ctx):
    rng = np.random.RandomState(64)
    text, runs = synth.text_like(400000, 31), synth.runs_mixed(200000, 32)
    docs = []
    for k in range(64):
        src = text if k % 3 else runs
        n = int(rng.randint(0, 3001))
        at = int(rng.randint(0, src.size - n))
        docs.append(np.ascontiguousarray(src[at:at + n]))
    got = ctx.bwtc_compress_many(docs, 7)
    for k, d in enumerate(docs):
        assert got[k] == ctx.bwtc_compress(d, 7), (k, d.size)


def test_device_division_is_exact(ctx):
    """floor(range / tot) of k11_code (lib/RangeCoder.js:81) for every tot the format can have and the ranges where a wrong floor
    would show: the multiples of tot around every power of two and their neighbours, and the ends."""
    L = ctx.L
    tot = np.arange(1, 65536, dtype=np.uint64)
    rs, ts = [], []
    for k in range(8, 32):
        q = (np.uint64(1) << np.uint64(k)) // tot
        for dm in (-1, 0, 1):
            m = q.astype(np.int64) + dm
            for dd in (-1, 0, 1):
                r = m * tot.astype(np.int64) + dd
                ok = (r >= 0) & (r <= 0xFFFFFFFF)
                rs.append(r[ok]); ts.append(tot[ok])
    for r0 in (0xFFFFFFFF, 0x00800001):
        rs.append(np.full(tot.size, r0, np.int64)); ts.append(tot)
    r = np.ascontiguousarray(np.concatenate(rs).astype(np.uint32))
    t = np.ascontiguousarray(np.concatenate(ts).astype(np.uint32))
    assert r.size > 12_000_000
    out = np.zeros(r.size, np.uint32)
    assert L.cjs_dbg_rc_div_device(r.ctypes.data, t.ctypes.data, r.size, out.ctypes.data) == 0
    bad = np.nonzero(out != r // t)[0]
    assert bad.size == 0, (int(r[bad[0]]), int(t[bad[0]]), int(out[bad[0]]))


def test_compress_files_api():
    from compressjs_amd import BWTC
    docs = [b"", b"hello hello", bytearray(b"a" * 1000), np.arange(300, dtype=np.uint8)]
    for lv in (9, 6, 2):
        assert BWTC.compressFiles(docs, lv) == [BWTC.compressFile(d, None, lv) for d in docs]
    assert BWTC.compressFiles(docs) == BWTC.compressFiles(docs, 0) == BWTC.compressFiles(docs, 9)
    assert BWTC.compressFiles([]) == []
