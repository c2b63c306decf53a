"""cjs_bwtc_decompress_batch_ex* with CJS_BWTC_DEC_DEFSUM_DEVICE on the CPU logic build (tests/emu): BWTC streams of levels 1-5 decoded
by k14_defsum_decoder.hip, one "wave" per document, between the batch's three waits.  A context of 2 blocks in flight; documents of
at most 6 000 bytes where the set allows.  Reduced against the GPU file: of the 40 hostile documents of defsum_cases.doc(i) the 10 of
30 000 bytes are left out here (those of 300, 2 000 and 9 000 bytes run), and the multi-block cases run the host form alone.  The case list is tests/bwtc_batch_decode_defsum_cases.py, shared with
tests/test_gpu_bwtc_batch_decode_defsum.py.  Not a parity claim for the GPU build."""
import pytest

import bwtc_batch_decode_defsum_cases as cs
import defsum_cases
import stagelib
from compressjs_amd import _lib


@pytest.fixture(scope="module")
def E():
    L = _lib.load(stagelib.build_emu())
    h = L.cjs_create(0, 2)
    assert h
    yield cs.Env(L, h, h, "host", True)
    L.cjs_destroy(h)


@pytest.mark.parametrize("level", (1, 2, 3, 4, 5))
def test_fuzz_cases_of_a_level_as_one_batch(E, level):
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
    cs.waits(E, (1, 40))
