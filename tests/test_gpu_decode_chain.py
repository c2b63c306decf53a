"""The single-call bzip2 decoder across slot batches on the MI355X: the cases of decode_chain_cases.py - a 40-stream file on 16
slots, clean and broken at chosen blocks, the partial result and the synchronisation count of the call,
cjs_bz2_decompress_block on the same file - through the host form and, on torch tensors, the device form."""
import pytest

import decode_chain_cases as dcc

pytestmark = pytest.mark.gpu


def _to_dev(a):
    import torch
    t = torch.from_numpy(a).cuda()
    return t.data_ptr(), t


@pytest.fixture(scope="module")
def ctx():
    from compressjs_amd.bzip2 import Context
    with dcc.sixteen_slots():
        c = Context(0, 8)               # fresh: its first decode sizes the slab
        try:
            yield c.L, c.h
        finally:
            c.close()


def test_clean_file_bytes_table_and_sync_count(ctx):
    dcc.check_clean(*ctx, _to_dev)


@pytest.mark.parametrize("name", sorted(dcc.PARENT_PARTIAL))
def test_error_and_partial_result_at_a_chosen_block(ctx, name):
    dcc.check_broken(*ctx, _to_dev, name)


def test_block_entry_on_the_same_file(ctx):
    dcc.check_block_entry(*ctx)
