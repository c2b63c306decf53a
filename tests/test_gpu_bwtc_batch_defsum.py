"""Levels 1-5 of the batched BWTC compress on the MI355X: DefSumModel on the GPU (k13_defsum_model.hip) feeding the device range coder
(k11_bwtc_coder.hip).  1. the model alone (cjs_dbg_defsum_triples) against the host model behind a recorder and the plain restatement
of lib/DefSumModel.js (defsum_cases.py), word for word; 2. the streams against the reference (golden_bwtc.json and the hostile
documents of golden_bwtc_defsum.json) and the single call, with 3 host<->device waits per device call and 4 per host call."""
import hashlib
import json
import os

import numpy as np
import pytest

import batch_cases as bc
import bwtc_cases
import defsum_cases as dc
from compressjs_amd import synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _vectors(name):
    with open(os.path.join(ROOT, "tests", "golden", name)) as f:
        return json.load(f)["vectors"]


@pytest.fixture(scope="module")
def gbwtc():
    return _vectors("golden_bwtc.json")


@pytest.fixture(scope="module")
def gdefsum():
    return _vectors("golden_bwtc_defsum.json")


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


def _syncs(c):
    return int(c.L.cjs_dbg_bwtc_batch_syncs(c.h))


def _host(c, docs, level, cap=None, lead=0):
    """cjs_bwtc_compress_batch through the C ABI -> (return value, out_off list, [streams] or None)"""
    flat, off = bc.pack(docs)
    if lead:
        flat = np.concatenate([np.full(lead, 0x5A, np.uint8), flat])
        off = off + np.uint64(lead)
    if cap is None:
        cap = int(c.L.cjs_bwtc_compress_batch_bound(int(off[-1] - off[0]), len(docs)))
    out = np.full(cap + 8, 0xAA, np.uint8)
    oo = np.full(len(docs) + 1, 0xEEEE, np.uint64)
    n = int(c.L.cjs_bwtc_compress_batch(c.h, flat.ctypes.data, off.ctypes.data, len(docs), level, out.ctypes.data, cap, oo.ctypes.data))
    assert (out[cap:] == 0xAA).all()
    if n < 0:
        return n, oo.tolist(), None
    return n, oo.tolist(), [out[int(oo[k]):int(oo[k + 1])].tobytes() for k in range(len(docs))]


def _device(c, docs, level, cap=None, lead=0):
    """cjs_bwtc_compress_batch_device on tensors -> (return value, out_off list, [streams] or None)"""
    import torch
    flat, off = bc.pack(docs)
    if lead:
        flat = np.concatenate([np.full(lead, 0x5A, np.uint8), flat])
        off = off + np.uint64(lead)
    if cap is None:
        cap = int(c.L.cjs_bwtc_compress_batch_bound(int(off[-1] - off[0]), len(docs)))
    d_in = torch.from_numpy(flat).cuda()
    d_off = torch.from_numpy(off.astype(np.int64)).cuda()
    d_out = torch.full((cap + 8,), 0xAA, dtype=torch.uint8, device="cuda")
    d_oo = torch.full((len(docs) + 1,), -1, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    n = int(c.L.cjs_bwtc_compress_batch_device(c.h, d_in.data_ptr(), d_off.data_ptr(), len(docs), level, d_out.data_ptr(), cap, d_oo.data_ptr()))
    waits = _syncs(c)
    torch.cuda.synchronize()
    oo = d_oo.cpu().numpy()
    out = d_out.cpu().numpy()
    assert (out[cap:] == 0xAA).all()
    if n < 0:
        return n, oo.tolist(), None
    assert waits == 3, waits
    return n, oo.tolist(), [out[int(oo[k]):int(oo[k + 1])].tobytes() for k in range(len(docs))]


def _against(got, want, what):
    assert len(got) == len(want)
    for k, (g, v) in enumerate(zip(got, want)):
        assert len(g) == v["out_len"] and hashlib.sha256(g).hexdigest() == v["out_sha256"], (what, k)


# ---- 1. the model alone --------------------------------------------------------------------------------------------------
def test_k13_rows_one_launch_each(ctx):
    dc.check_families()
    dc.assert_rows_equal(dc.run_model(ctx.L, dc.rows(), True), dc.rows(), "host")
    for r in dc.rows():
        dc.assert_rows_equal(dc.run_model(ctx.L, [r], False), [r], "k13 nb=1")


def test_k13_seventy_rows_in_one_launch(ctx):
    sel = dc.seventy()
    assert len(sel) == 70
    got = dc.run_model(ctx.L, sel, False)
    dc.assert_rows_equal(got, sel, "k13 nb=70")
    for (n, a, t), (hn, ha, ht) in zip(got, dc.run_model(ctx.L, sel, True)):
        assert n == hn and np.array_equal(a, ha) and np.array_equal(t, ht)


# ---- 2. the batch ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("level", range(1, 6))
def test_fuzz_cases_of_a_level_both_forms_and_their_waits(ctx, gbwtc, level):
    ids = [i for i in range(bwtc_cases.N_SMALL) if bwtc_cases.case(i)[1] == level and bwtc_cases.case(i)[0].size <= 6000]
    docs = [bwtc_cases.case(i)[0] for i in ids]
    assert len(docs) >= 15
    want = [gbwtc["fuzz%d" % i] for i in ids]
    n, oo, got = _host(ctx, docs, level)
    assert n > 0 and oo[0] == 0 and oo[-1] == n and _syncs(ctx) == 4     # the device form's three and the download
    _against(got, want, ("host", level))
    n, oo, got = _device(ctx, docs, level)                                 # (asserts its 3 waits)
    assert n > 0 and oo[0] == 0 and oo[-1] == n
    _against(got, want, ("device", level))


@pytest.mark.parametrize("level", range(1, 6))
def test_reference_made_hostile_documents(ctx, gdefsum, level):
    ids = [i for i in range(dc.N_DOCS) if dc.doc(i)[1] == level]
    assert len(ids) == 8
    docs, want = [dc.doc(i)[0] for i in ids], [gdefsum["doc%d" % i] for i in ids]
    _against(_host(ctx, docs, level)[2], want, ("host", level))
    _against(_device(ctx, docs, level)[2], want, ("device", level))


@pytest.mark.parametrize("level", (1, 5))
def test_sync_count_does_not_grow_with_the_documents(ctx, level):
    for k in (1, 40):
        docs = [bc._b(b"abracadabra" * (1 + j % 5)) for j in range(k)]
        n, _, got = _host(ctx, docs, level)
        assert n > 0 and _syncs(ctx) == 4 and got[0] == ctx.bwtc_compress(docs[0], level)
        assert _device(ctx, docs, level)[2] == got                         # (asserts its 3 waits)


def test_coder_state_carried_across_two_launches_level_1(ctx2, gdefsum):
    big = dc.big_doc()
    docs = [bc._b(b"hello hello"), big, np.zeros(0, np.uint8), synth.text_like(700, 4)]
    want = [ctx2.bwtc_compress(d, 1) for d in docs]
    assert _host(ctx2, docs, 1)[2] == want and ctx2.last_block_count == 1 + 2 + 0 + 1
    assert _device(ctx2, docs, 1)[2] == want
    _against(want[1:2], [gdefsum[dc.BIG_ID]], "text100001")


@pytest.mark.parametrize("cid", ["rand250k_l1", "rand250k_l2"])
def test_multi_block_random_documents_between_small_ones(ctx2, gbwtc, cid):
    big = {c: (d, lv) for c, d, lv in bwtc_cases.big_cases()}
    d, level = big[cid]
    small = [i for i in range(bwtc_cases.N_SMALL) if bwtc_cases.case(i)[1] == level and bwtc_cases.case(i)[0].size <= 1000][:4]
    docs = [bwtc_cases.case(i)[0] for i in small[:2]] + [d] + [bwtc_cases.case(i)[0] for i in small[2:]]
    want = [gbwtc["fuzz%d" % i] for i in small[:2]] + [gbwtc[cid]] + [gbwtc["fuzz%d" % i] for i in small[2:]]
    _against(_host(ctx2, docs, level)[2], want, cid)
    _against(_device(ctx2, docs, level)[2], want, cid)


def test_one_hundred_and_thirty_documents_level_3(ctx):
    """more than two waves of k11_code in one call"""
    rng = np.random.RandomState(130)
    text, runs = synth.text_like(200000, 31), synth.runs_mixed(100000, 32)
    docs = []
    for k in range(130):
        src = text if k % 3 else runs
        n = int(rng.randint(0, 2001))
        at = int(rng.randint(0, src.size - n))
        docs.append(np.ascontiguousarray(src[at:at + n]))
    got = _device(ctx, docs, 3)[2]
    assert _host(ctx, docs, 3)[2] == got
    for k, d in enumerate(docs):
        assert got[k] == ctx.bwtc_compress(d, 3), (k, d.size)


def test_offsets_empty_documents_and_no_space(ctx):
    e = np.zeros(0, np.uint8)
    docs = [bc._b(b"hello hello"), e, synth.text_like(3000, 6)]
    for fn in (_host, _device):
        n, oo, got = fn(ctx, docs, 3, lead=37)                              # off[0] != 0
        assert n > 0 and oo[0] == 0 and got == [ctx.bwtc_compress(d, 3) for d in docs]
        n, oo, got = fn(ctx, [e, e, e], 2)
        assert n == 30 and oo == [0, 10, 20, 30] and got == [ctx.bwtc_compress(e, 2)] * 3
    docs = [bc._b(b"hello hello"), bc._b(b"world"), np.full(1000, 97, np.uint8)]
    n, oo, want = _host(ctx, docs, 4)
    assert n > 0 and want == [ctx.bwtc_compress(d, 4) for d in docs]
    for fn in (_host, _device):
        short, oo2, _ = fn(ctx, docs, 4, cap=n - 1)
        assert short == -21 and oo2 == oo                                   # out_off complete all the same
        exact, oo3, got = fn(ctx, docs, 4, cap=n)
        assert exact == n and got == want and oo3 == oo


def test_compress_files_api_levels_1_to_5():
    from compressjs_amd import BWTC
    docs = [b"", b"hello hello", bytearray(b"a" * 1000), np.arange(300, dtype=np.uint8), dc.doc(0)[0], dc.doc(5)[0]]
    for lv in range(1, 6):
        assert BWTC.compressFiles(docs, lv) == [BWTC.compressFile(d, None, lv) for d in docs]
