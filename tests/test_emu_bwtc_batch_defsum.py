"""Levels 1-5 of cjs_bwtc_compress_batch* on the CPU logic build (tests/emu): DefSumModel runs on the device (k13_defsum_model.hip),
its triples go to the device range coder (k11_bwtc_coder.hip), and no host code is left between upload and download.
1. the model alone (cjs_dbg_defsum_triples): K13 against the host model behind a recorder and against the plain restatement of
   lib/DefSumModel.js in defsum_cases.py, word for word;
2. the streams against the reference (golden_bwtc.json, golden_bwtc_defsum.json) and against the single call, and the number of
   host<->device waits of a call: 3 for the device form, 4 for the host form, whatever the level and the number of documents.
Not a parity claim for the GPU build (tests/test_gpu_bwtc_batch_defsum.py is)."""
import hashlib
import json
import os

import numpy as np
import pytest

import batch_cases as bc
import bwtc_cases
import defsum_cases as dc
import stagelib
from compressjs_amd import _lib, synth

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


@pytest.fixture(scope="module")
def gdefsum():
    with open(os.path.join(ROOT, "tests", "golden", "golden_bwtc_defsum.json")) as f:
        return json.load(f)["vectors"]


def _batch(Lh, docs, level, cap=None, device=False, lead=0):
    """-> (return value, out_off, [streams]); lead: bytes in front of the first document (off[0] != 0)"""
    L, h = Lh
    flat, off = bc.pack(docs)
    if lead:
        flat = np.concatenate([np.full(lead, 0x5A, np.uint8), flat])
        off = off + np.uint64(lead)
    if cap is None:
        cap = int(L.cjs_bwtc_compress_batch_bound(int(off[-1] - off[0]), len(docs)))
    out = np.full(cap + 8, 0xAA, np.uint8)              # stale bytes: the call must write every byte it returns
    out_off = np.full(len(docs) + 1, 0xEEEE, np.uint64)
    fn = L.cjs_bwtc_compress_batch_device if device else L.cjs_bwtc_compress_batch     # (host memory serves as device memory in this build)
    n = fn(h, flat.ctypes.data, off.ctypes.data, len(docs), level, out.ctypes.data, cap, out_off.ctypes.data)
    if n < 0:
        return n, out_off, None
    assert (out[cap:] == 0xAA).all()
    return n, out_off, [out[int(out_off[k]):int(out_off[k + 1])].tobytes() for k in range(len(docs))]


def _single(Lh, d, level):
    L, h = Lh
    cap = int(L.cjs_bwtc_compress_bound(d.size))
    out = np.zeros(cap, np.uint8)
    m = L.cjs_bwtc_compress(h, d.ctypes.data, d.size, level, out.ctypes.data, cap, d.size)
    assert m > 0
    return out[:m].tobytes()


def _check_digests(Lh, docs, level, want, device=False):
    n, out_off, got = _batch(Lh, docs, level, device=device)
    assert n >= 0, n
    assert int(out_off[0]) == 0 and int(out_off[-1]) == n == sum(v["out_len"] for v in want)
    for k, (g, v) in enumerate(zip(got, want)):
        assert len(g) == v["out_len"] and hashlib.sha256(g).hexdigest() == v["out_sha256"], (k, docs[k].size, level)
    return got


# ---- 1. the model alone --------------------------------------------------------------------------------------------------
def test_row_families_reach_the_rare_branches():
    dc.check_families()


def test_host_recorder_equals_the_restatement(emu_ctx):
    L, _ = emu_ctx
    dc.assert_rows_equal(dc.run_model(L, dc.rows(), True), dc.rows(), "host")


def test_k13_rows_one_launch_each(emu_ctx):
    L, _ = emu_ctx
    for r in dc.rows():
        dc.assert_rows_equal(dc.run_model(L, [r], False), [r], "k13 nb=1")


def test_k13_seventy_rows_in_one_launch(emu_ctx):
    L, _ = emu_ctx
    sel = dc.seventy()
    assert len(sel) == 70 and len({r[1].size for r in sel}) >= 12
    got = dc.run_model(L, sel, False)
    dc.assert_rows_equal(got, sel, "k13 nb=70")
    host = dc.run_model(L, sel, True)
    for (n, a, t), (hn, ha, ht) in zip(got, host):
        assert n == hn and np.array_equal(a, ha) and np.array_equal(t, ht)


def test_k13_reports_rows_that_are_too_short(emu_ctx):
    """rows of 2 x stride always suffice; a caller with shorter rows gets K10_OVERFLOW, and nothing is written past its row"""
    L, _ = emu_ctx
    r = next(x for x in dc.rows() if x[0] == "sorted")
    sym, nsym, alpha, stride = dc.pack_rows([r, r])
    ostride = stride + 8                                  # < the 7 839 triples of the row
    sylt = np.full(2 * ostride + 64, 0xDDDDDDDD, np.uint32)
    tot = np.full(2 * ostride + 64, 0xDDDDDDDD, np.uint32)
    ntri = np.zeros(2, np.uint32)
    assert L.cjs_dbg_defsum_triples(sym.ctypes.data, nsym.ctypes.data, alpha.ctypes.data, 2, stride, sylt.ctypes.data, tot.ctypes.data,
                                    ntri.ctypes.data, ostride, 0) == 0
    assert ntri.tolist() == [0xFFFFFFFF, 0xFFFFFFFF]
    assert (sylt[2 * ostride:] == 0xDDDDDDDD).all() and (tot[2 * ostride:] == 0xDDDDDDDD).all()
    assert np.array_equal(sylt[ostride:ostride + 64], r[3][:64])          # row 1 starts where it should: row 0 stayed inside its own


# ---- 2. the batch ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("level", range(1, 6))
def test_fuzz_cases_of_a_level_both_forms_and_their_waits(emu_ctx, gbwtc, level):
    L, h = emu_ctx
    ids = [i for i in range(bwtc_cases.N_SMALL) if bwtc_cases.case(i)[1] == level and bwtc_cases.case(i)[0].size <= 6000]
    docs = [bwtc_cases.case(i)[0] for i in ids]
    assert len(docs) >= 15
    want = [gbwtc["fuzz%d" % i] for i in ids]
    _check_digests(emu_ctx, docs, level, want)
    assert L.cjs_dbg_bwtc_batch_syncs(h) == 4             # the device form's three and the download
    _check_digests(emu_ctx, docs, level, want, device=True)
    assert L.cjs_dbg_bwtc_batch_syncs(h) == 3


@pytest.mark.parametrize("level", (1, 5))
def test_sync_count_does_not_grow_with_the_documents(emu_ctx, level):
    L, h = emu_ctx
    for device, want in ((True, 3), (False, 4)):
        counts = []
        for k in (1, 40):
            docs = [bc._b(b"abracadabra" * (1 + j % 5)) for j in range(k)]
            n, _, got = _batch(emu_ctx, docs, level, device=device)
            assert n > 0 and got[0] == _single(emu_ctx, docs[0], level)
            counts.append(L.cjs_dbg_bwtc_batch_syncs(h))
        assert counts == [want, want]


@pytest.mark.parametrize("level", range(1, 6))
def test_reference_made_hostile_documents(emu_ctx, gdefsum, level):
    ids = [i for i in range(dc.N_DOCS) if dc.doc(i)[1] == level and dc.doc(i)[0].size <= 9000]
    assert len(ids) >= 4
    _check_digests(emu_ctx, [dc.doc(i)[0] for i in ids], level, [gdefsum["doc%d" % i] for i in ids])


def test_coder_state_carried_across_two_launches_level_1(emu_ctx, gdefsum):
    """[small, 100 001 bytes, empty, small] with 2 blocks in flight: the long document is a full block and a block of one byte, in
    two sub-batches, so its coder state waits in HBM between two k11_code launches"""
    L, h = emu_ctx
    big = dc.big_doc()
    assert big.size == 100001
    docs = [bc._b(b"hello hello"), big, np.zeros(0, np.uint8), synth.text_like(700, 4)]
    for device in (False, True):
        n, out_off, got = _batch(emu_ctx, docs, 1, device=device)
        assert n > 0 and L.cjs_last_block_count(h) == 1 + 2 + 0 + 1
        assert got == [_single(emu_ctx, d, 1) for d in docs]
    v = gdefsum[dc.BIG_ID]
    assert len(got[1]) == v["out_len"] and hashlib.sha256(got[1]).hexdigest() == v["out_sha256"]


@pytest.mark.parametrize("cid", ["rand250k_l1", "rand250k_l2"])
def test_multi_block_random_documents_between_small_ones(emu_ctx, gbwtc, cid):
    big = {c: (d, lv) for c, d, lv in bwtc_cases.big_cases()}
    d, level = big[cid]
    small = [i for i in range(bwtc_cases.N_SMALL) if bwtc_cases.case(i)[1] == level and bwtc_cases.case(i)[0].size <= 1000][:4]
    docs = [bwtc_cases.case(i)[0] for i in small[:2]] + [d] + [bwtc_cases.case(i)[0] for i in small[2:]]
    want = [gbwtc["fuzz%d" % i] for i in small[:2]] + [gbwtc[cid]] + [gbwtc["fuzz%d" % i] for i in small[2:]]
    _check_digests(emu_ctx, docs, level, want, device=True)
    L, h = emu_ctx
    assert L.cjs_dbg_bwtc_batch_syncs(h) == 3


def test_offsets_that_do_not_start_at_zero(emu_ctx):
    docs = [bc._b(b"hello hello"), np.zeros(0, np.uint8), synth.text_like(3000, 6)]
    for device in (False, True):
        n, out_off, got = _batch(emu_ctx, docs, 3, device=device, lead=37)
        assert n > 0 and int(out_off[0]) == 0 and got == [_single(emu_ctx, d, 3) for d in docs]


def test_three_empty_documents_level_2(emu_ctx):
    e = np.zeros(0, np.uint8)
    for device in (False, True):
        n, out_off, got = _batch(emu_ctx, [e, e, e], 2, device=device)
        assert n == 30 and out_off.tolist() == [0, 10, 20, 30] and got == [_single(emu_ctx, e, 2)] * 3


def test_no_space_level_4(emu_ctx):
    docs = [bc._b(b"hello hello"), bc._b(b"world"), np.full(1000, 97, np.uint8)]
    n, out_off, want = _batch(emu_ctx, docs, 4)
    assert n > 0 and want == [_single(emu_ctx, d, 4) for d in docs]
    for device in (False, True):
        short, oo2, _ = _batch(emu_ctx, docs, 4, cap=n - 1, device=device)
        assert short == -21 and oo2.tolist() == out_off.tolist()          # out_off complete all the same
        exact, oo3, got = _batch(emu_ctx, docs, 4, cap=n, device=device)
        assert exact == n and got == want and oo3.tolist() == out_off.tolist()
