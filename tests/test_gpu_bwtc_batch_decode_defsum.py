"""Batched BWTC decode of levels 1-5 on the MI355X: cjs_bwtc_decompress_batch_ex / _batch_device_ex with CJS_BWTC_DEC_DEFSUM_DEVICE run
DefSumModel's decoder on the GPU (k14_defsum_decoder.hip), one wave per document, between the batch's three waits.  The case list is
tests/bwtc_batch_decode_defsum_cases.py (shared with tests/test_emu_bwtc_batch_decode_defsum.py): the streams are made by the existing
compress entries and checked against the reference's digests, the arbiter of a decoded document is its input, of a damaged stream
the single call on the same build."""
import numpy as np
import pytest

import bwtc_batch_decode_cases as dc
import bwtc_batch_decode_defsum_cases as cs
import defsum_cases

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def E():
    from compressjs_amd.bzip2 import Context
    c, c2 = Context(0, 8), Context(0, 2)
    yield cs.Env(c.L, c.h, c2.h, "torch", False)
    c.close()
    c2.close()


@pytest.mark.parametrize("level", (1, 2, 3, 4, 5))
def test_all_fuzz_cases_of_a_level_as_one_batch(E, level):
    cs.fuzz_level(E, level)


@pytest.mark.parametrize("level", (1, 2, 3, 4, 5))
def test_hostile_documents_of_a_level(E, level):
    cs.hostile_level(E, level)


def test_table_shapes(E):
    cs.table_shapes(E)


@pytest.mark.parametrize("level", (1, 5))
def test_runs_and_ends(E, level):
    cs.runs_and_ends(E, level)


@pytest.mark.parametrize("cid", (defsum_cases.BIG_ID, "rand250k_l1", "rand250k_l2"))
def test_multi_block_documents(E, cid):
    cs.multi_block(E, cid)


def test_levels_1_to_9_interleaved_run_both_kernels(E):
    cs.levels_interleaved(E)


def test_alignment_and_isolation(E):
    cs.alignment_and_isolation(E)


def test_sweep_of_flips_and_cuts_equals_the_single_call(E):
    cs.sweep(E)


def test_host_path_documents_between_fast_ones_with_the_flag(E):
    cs.host_path_between_fast_ones(E)


def test_budget_bounds_the_scratch(E, monkeypatch):
    cs.budget(E, monkeypatch)


def test_call_level(E, golden):
    cs.call_level(E, golden)


def test_sync_count_does_not_grow_with_the_documents(E):
    cs.waits(E, (8, 200))


def test_python_api_takes_the_device_path():
    import torch
    from compressjs_amd import BWTC
    from compressjs_amd.bzip2 import Context
    docs = [b"", b"hello hello", bytearray(b"a" * 1000), np.arange(300, dtype=np.uint8), np.resize(np.arange(7, dtype=np.uint8), 5000)]
    plain = [d.tobytes() if isinstance(d, np.ndarray) else bytes(d) for d in docs]
    for lv in (1, 2, 3, 4, 5):
        assert BWTC.decompressFiles(BWTC.compressFiles(docs, lv)) == plain
    c = Context(0, 8)
    try:
        streams = c.bwtc_compress_many([np.frombuffer(p, dtype=np.uint8) for p in plain], 4)
        flat, off = dc.pack(streams)
        d_in, d_off = torch.from_numpy(flat).cuda(), torch.from_numpy(off.astype(np.int64)).cuda()
        d_out = torch.zeros(8192, dtype=torch.uint8, device="cuda")
        d_oo = torch.zeros(len(docs) + 1, dtype=torch.int64, device="cuda")
        d_st = torch.full((len(docs),), 7, dtype=torch.int32, device="cuda")
        n = c.bwtc_decompress_many_device(d_in, d_off, d_out, d_oo, d_st)
        assert int(c.L.cjs_dbg_bwtc_dec_batch_fallbacks(c.h)) == 0 and int(c.L.cjs_dbg_bwtc_dec_batch_syncs(c.h)) == 3
        assert n == sum(len(p) for p in plain) and d_st.cpu().tolist() == [0] * len(docs)
        assert d_out.cpu().numpy()[:n].tobytes() == b"".join(plain)
        assert c.bwtc_decompress_many(streams) == plain
        assert int(c.L.cjs_dbg_bwtc_dec_batch_fallbacks(c.h)) == 0
    finally:
        c.close()
