"""The single-call bzip2 decoder across slot batches on the CPU logic build (tests/emu): the cases of decode_chain_cases.py - a
40-stream file on 16 slots, clean and broken at chosen blocks, the partial result and the synchronisation count of the call,
cjs_bz2_decompress_block on the same file.  The device form takes host pointers here.  Not a parity claim for the GPU build
(tests/test_gpu_decode_chain.py is)."""
import pytest

import decode_chain_cases as dcc
import stagelib
from compressjs_amd import _lib


@pytest.fixture(scope="module")
def emu_ctx():
    L = _lib.load(stagelib.build_emu())
    with dcc.sixteen_slots():
        h = L.cjs_create(0, 2)          # fresh: its first decode sizes the slab
        assert h
        yield L, h
        L.cjs_destroy(h)


def test_clean_file_bytes_table_and_sync_count(emu_ctx):
    dcc.check_clean(*emu_ctx, dcc.host_ptr)


@pytest.mark.parametrize("name", sorted(dcc.PARENT_PARTIAL))
def test_error_and_partial_result_at_a_chosen_block(emu_ctx, name):
    dcc.check_broken(*emu_ctx, dcc.host_ptr, name)


def test_block_entry_on_the_same_file(emu_ctx):
    dcc.check_block_entry(*emu_ctx)
