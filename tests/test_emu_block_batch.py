"""The batched block fetch (cjs_bz2_decompress_blocks) on the CPU logic build (tests/emu): the cases of block_batch_cases.py - the
reference-made block records, a shuffled list of blocks, end magics and misses on 16 slots, the synchronisation count of the call,
broken blocks, the call level, the neighbouring entries on the same context.  The device form takes host pointers here.  Not a
parity claim for the GPU build (tests/test_gpu_block_batch.py is)."""
import pytest

import block_batch_cases as bbc
import decode_chain_cases as dcc
import stagelib
from compressjs_amd import _lib

FORMS = {"host": bbc.HostMem(), "device": bbc.HostAsDevice()}


@pytest.fixture(scope="module")
def emu_ctx():
    L = _lib.load(stagelib.build_emu())
    with dcc.sixteen_slots():
        h = L.cjs_create(0, 2)          # fresh: its first decode sizes the slab
        assert h
        yield L, h
        L.cjs_destroy(h)


def test_reference_made_block_outcomes(emu_ctx):
    assert bbc.check_golden(*emu_ctx, bbc.HostMem(), max_len=1200) >= 3          # (enc:text1k:9 at 32, 33 and 40)


@pytest.mark.parametrize("form", sorted(FORMS))
def test_shuffled_blocks_ends_and_misses_across_slot_batches(emu_ctx, form):
    bbc.check_mixed(*emu_ctx, FORMS[form])


def test_equal_to_a_loop_of_single_calls(emu_ctx):
    bbc.check_mixed_vs_single_calls(*emu_ctx, bbc.HostMem())


@pytest.mark.parametrize("form", sorted(FORMS))
def test_waits_do_not_depend_on_the_request_count(emu_ctx, form):
    bbc.check_waits(*emu_ctx, FORMS[form])


@pytest.mark.parametrize("form", sorted(FORMS))
@pytest.mark.parametrize("name", bbc.BROKEN)
def test_broken_blocks(emu_ctx, name, form):
    bbc.check_broken(*emu_ctx, FORMS[form], name)


def test_call_level(emu_ctx):
    bbc.check_call_level(*emu_ctx)


def test_neighbours_undisturbed(emu_ctx):
    L, h = emu_ctx
    bbc.check_neighbours(L, h, bbc.ctx_factory(L, 2))
