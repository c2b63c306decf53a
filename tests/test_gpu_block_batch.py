"""The batched block fetch (cjs_bz2_decompress_blocks) on the MI355X: the cases of block_batch_cases.py - the reference-made block
records, a shuffled list of blocks, end magics and misses on 16 slots, the synchronisation count of the call, broken blocks,
full-size blocks, the call level, the neighbouring entries on the same context - through the host form and, on torch tensors, the
device form, and through the Python entries."""
import numpy as np
import pytest

import batch_decode_cases as bdc
import block_batch_cases as bbc
import decode_chain_cases as dcc

pytestmark = pytest.mark.gpu


class TorchMem:
    """the caller's arrays as CUDA tensors (64- and 32-bit unsigned as the signed types of the same width)"""
    device = True
    SIGNED = {np.dtype(np.uint64): np.int64, np.dtype(np.uint32): np.int32}

    def up(self, a):
        import torch
        t = torch.from_numpy(a.view(self.SIGNED.get(a.dtype, a.dtype))).cuda()
        return t.data_ptr(), (t, a.dtype)

    def down(self, owner):
        t, dt = owner
        return t.cpu().numpy().view(dt)


FORMS = {"host": bbc.HostMem(), "device": TorchMem()}


@pytest.fixture(scope="module")
def ctx():
    from compressjs_amd.bzip2 import Context
    with dcc.sixteen_slots():
        c = Context(0, 8)               # fresh: its first decode sizes the slab
        try:
            yield c.L, c.h
        finally:
            c.close()


@pytest.mark.parametrize("form", sorted(FORMS))
def test_reference_made_block_outcomes(form):
    from compressjs_amd.bzip2 import Context
    c = Context(0, 8)                   # (sample4's blocks on the slot count of a default context)
    try:
        assert bbc.check_golden(c.L, c.h, FORMS[form]) >= 4
    finally:
        c.close()


@pytest.mark.parametrize("form", sorted(FORMS))
def test_shuffled_blocks_ends_and_misses_across_slot_batches(ctx, form):
    bbc.check_mixed(*ctx, FORMS[form])


def test_equal_to_a_loop_of_single_calls(ctx):
    bbc.check_mixed_vs_single_calls(*ctx, bbc.HostMem())


@pytest.mark.parametrize("form", sorted(FORMS))
def test_waits_do_not_depend_on_the_request_count(ctx, form):
    bbc.check_waits(*ctx, FORMS[form])


@pytest.mark.parametrize("form", sorted(FORMS))
@pytest.mark.parametrize("name", bbc.BROKEN)
def test_broken_blocks(ctx, name, form):
    bbc.check_broken(*ctx, FORMS[form], name)


@pytest.mark.parametrize("form", sorted(FORMS))
def test_full_size_blocks(form):
    """Level 1: three blocks requested in reverse order.  Level 9: both blocks of a 1 000 000-byte text, the first at capacity."""
    import cases
    from compressjs_amd import synth
    from compressjs_amd.bzip2 import Context
    import oracle
    c = Context(0, 8)
    try:
        s3, tab = bdc.three_blocks()
        data = cases.case_input("lcg250000").tobytes()
        cut = np.concatenate([[0], np.cumsum([z for _p, z in tab])]).tolist()
        assert cut[-1] == len(data)
        order = [2, 1, 0]
        r = bbc.run_blocks(c.L, c.h, s3, [tab[k][0] for k in order], FORMS[form], cap=len(data), tail=64)
        assert r.ret == len(data) and [int(x) for x in r.status] == [0, 0, 0]
        assert r.out[:len(data)].tobytes() == b"".join(data[cut[k]:cut[k + 1]] for k in order)
        assert bytes(r.out[len(data):]) == b"\xaa" * 64

        text = synth.text_like(1000000, 11)
        s = c.compress(text, 9)
        tab = oracle.bz2_decompress(s)[3]
        assert len(tab) == 2 and tab[0][1] + tab[1][1] == text.size and tab[0][1] > 890000
        r = bbc.run_blocks(c.L, c.h, s, [tab[1][0], tab[0][0]], FORMS[form], cap=text.size)
        assert r.ret == text.size and [int(x) for x in r.out_off] == [0, tab[1][1], text.size]
        assert r.doc(0) == text[tab[0][1]:].tobytes() and r.doc(1) == text[:tab[0][1]].tobytes()
    finally:
        c.close()


def test_call_level(ctx):
    bbc.check_call_level(*ctx)


def test_neighbours_undisturbed(ctx):
    L, h = ctx
    bbc.check_neighbours(L, h, bbc.ctx_factory(L, 8))


def test_python_entries(ctx):
    """Context.decompress_blocks / decompress_blocks_device and Bzip2.decompressBlocks: bytes, errors with .index."""
    import torch
    from compressjs_amd import Bzip2
    from compressjs_amd.bzip2 import Context
    f = dcc.the_file()
    pos = [f.tab[30][0], dcc.end_magic(f, 2), f.tab[4][0], f.tab[4][0] + 1, f.tab[30][0]]
    want = [bbc.want_of("file", f.data, p) for p in pos]
    c = Context(0, 8)
    try:
        got = c.decompress_blocks(f.data, pos, return_errors=True)
        for k, w in enumerate(want):
            if w[0] < 0:
                assert isinstance(got[k], TypeError) and (got[k].errorCode, got[k].index, str(got[k])) == (-2, k, "Not bzip data")
            else:
                assert got[k] == w[2], k
        with pytest.raises(TypeError) as e:
            c.decompress_blocks(f.data, pos)
        assert e.value.index == 3 and e.value.errorCode == -2
        assert c.decompress_blocks(f.data, []) == []
        assert Bzip2.decompressBlocks(f.data, pos[:3]) == [w[2] for w in want[:3]]
        d_in = torch.from_numpy(np.frombuffer(f.data, np.uint8).copy()).cuda()
        d_pos = torch.tensor(pos, dtype=torch.int64, device="cuda")
        d_out = torch.full((8192,), 0xAA, dtype=torch.uint8, device="cuda")
        d_oo = torch.full((len(pos) + 1,), -1, dtype=torch.int64, device="cuda")
        d_st = torch.full((len(pos),), 77, dtype=torch.int32, device="cuda")
        n = c.decompress_blocks_device(d_in, d_pos, d_out, d_oo, d_st)
        assert n == sum(w[0] for w in want if w[0] > 0) and d_st.tolist() == [min(w[0], 0) for w in want]
        assert d_out[:n].cpu().numpy().tobytes() == b"".join(w[2] for w in want if w[0] > 0) and d_oo.tolist()[-1] == n
    finally:
        c.close()
