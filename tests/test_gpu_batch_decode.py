"""Batched bzip2 decode on the MI355X (cjs_bz2_decompress_batch / _batch_device through compressjs_amd.bzip2): N documents in one
call, every one as the single call gives it for that document alone - bytes, or the reference's error.  Arbiters: the reference-
made records of tests/golden/golden_decode.json for the catalogue, oracle.bz2_decompress (pinned to the reference by the suite)
for everything else."""
import os

import numpy as np
import pytest

import batch_cases as bc
import batch_decode_cases as bdc
import oracle
from compressjs_amd import synth

pytestmark = pytest.mark.gpu
ROOT = bdc.ROOT


@pytest.fixture(scope="module")
def ctx():
    from compressjs_amd.bzip2 import Context
    c = Context(0, 8)
    yield c
    c.close()


def _device(c, streams, ms, cap=None):
    """The device form on torch tensors pre-filled with stale values -> bdc.Result"""
    import torch
    flat, off = bdc.pack(streams)
    n = len(streams)
    if cap is None:
        cap = sum(max(oracle.bz2_decompress(bytes(s), bool(ms))[0], 0) for s in streams) + 64
    d_in = torch.from_numpy(flat if flat.size else np.zeros(1, np.uint8)).cuda()
    d_off = torch.from_numpy(off.astype(np.int64)).cuda()
    d_out = torch.full((cap,), 0xAA, dtype=torch.uint8, device="cuda")
    d_oo = torch.full((n + 1,), -1, dtype=torch.int64, device="cuda")
    d_st = torch.full((n,), 77, dtype=torch.int32, device="cuda")
    d_det = torch.full((3 * n,), 0xDDDD, dtype=torch.int32, device="cuda")
    total = c.decompress_many_device(d_in, d_off, d_out, d_oo, d_st, ms, d_det)
    oo = d_oo.cpu().numpy().astype(np.uint64)
    out = d_out[:total].cpu().numpy()
    assert int(oo[0]) == 0 and int(oo[-1]) == total
    docs = [out[int(oo[k]):int(oo[k + 1])].tobytes() for k in range(n)]
    return bdc.Result(total, oo, d_st.cpu().numpy(), d_det.cpu().numpy().view(np.uint32), docs)


def test_whole_catalogue_host_and_device_forms(ctx):
    by, g = bdc.catalogue(), bdc.golden_decode()
    assert len(by[False][0]) + len(by[True][0]) == 142
    for ms in (False, True):
        ids, streams = by[ms]
        bdc.check_vs_golden(bdc.run_batch(ctx.L, ctx.h, streams, ms), ids, g, "host ms=%d" % ms)
        r = _device(ctx, streams, ms, sum(g[sid]["out_len"] for sid in ids if g[sid]["ok"]) + 64)
        bdc.check_vs_golden(r, ids, g, "device ms=%d" % ms)


def test_documents_across_slot_batches():
    """16 slots (CJS_DEC_MAX_SLOTS is read per call; the slab never shrinks, hence a fresh context whose first decode this is):
    the three-block documents' blocks are candidates 63-65 and 127-129, across slot batch boundaries; a corrupt document in every
    slot batch."""
    from compressjs_amd.bzip2 import Context
    docs = bdc.slot_batch_set()
    assert 145 <= len(docs) <= 155
    old = os.environ.get("CJS_DEC_MAX_SLOTS")
    os.environ["CJS_DEC_MAX_SLOTS"] = "16"
    c = Context(0, 8)
    try:
        r = bdc.run_batch(c.L, c.h, docs, False)
        bdc.check_vs_oracle(r, docs, False, "host")
        assert sum(1 for x in r.status if x) >= len(range(5, len(docs), 16))       # (one flipped CRC bit in every stretch of 16)
        bdc.check_vs_oracle(_device(c, docs, False), docs, False, "device")
    finally:
        c.close()
        if old is None:
            del os.environ["CJS_DEC_MAX_SLOTS"]
        else:
            os.environ["CJS_DEC_MAX_SLOTS"] = old


def test_round_trip_with_the_batched_encoder(ctx):
    import torch
    docs = bc.set_a() + bc.set_b(7)
    want = [d.tobytes() for d in docs]
    streams = ctx.compress_many(docs, bc.LEVEL)
    assert ctx.decompress_many(streams) == want
    # device forms end to end: the encoder's output tensors are the decoder's input
    flat, off = bc.pack(docs)
    cap = int(ctx.L.cjs_bz2_compress_batch_bound(int(off[-1]), len(docs)))
    d_in, d_off = torch.from_numpy(flat).cuda(), torch.from_numpy(off.astype(np.int64)).cuda()
    d_z = torch.zeros(cap, dtype=torch.uint8, device="cuda")
    d_zoff = torch.zeros(len(docs) + 1, dtype=torch.int64, device="cuda")
    ctx.compress_many_device(d_in, d_off, d_z, d_zoff, bc.LEVEL)
    d_back = torch.full((flat.size + 64,), 0xAA, dtype=torch.uint8, device="cuda")
    d_boff = torch.full((len(docs) + 1,), -1, dtype=torch.int64, device="cuda")
    d_st = torch.full((len(docs),), 77, dtype=torch.int32, device="cuda")
    n = ctx.decompress_many_device(d_z, d_zoff, d_back, d_boff, d_st)
    assert n == flat.size and not d_st.any().item()
    assert torch.equal(d_boff, d_off) and torch.equal(d_back[:n], d_in)


def test_three_hundred_small_documents_default_context():
    from compressjs_amd.bzip2 import Context
    rng = np.random.RandomState(300)
    text, runs = synth.text_like(400000, 31), synth.runs_mixed(200000, 32)
    docs = []
    for k in range(300):
        src = text if k % 3 else runs
        n = int(rng.randint(0, 2001))
        at = int(rng.randint(0, src.size - n))
        docs.append(np.ascontiguousarray(src[at:at + n]))
    c = Context()
    try:
        streams = c.compress_many(docs, 1)
        assert c.decompress_many(streams) == [d.tobytes() for d in docs]
    finally:
        c.close()


def test_differential_fuzz_and_sync_count(ctx):
    n = 0
    for docs, ms in bdc.fuzz_batches(20261019, 15, 10, exact=True):
        r = _device(ctx, docs, ms) if n & 1 else bdc.run_batch(ctx.L, ctx.h, docs, ms)
        bdc.check_vs_oracle(r, docs, ms, "batch %d" % n)
        n += len(docs)
    assert n == 150
    # no per-document host<->device traffic: 200 one-block documents cost as many synchronisations as 2
    s = [bdc.one_block(50 + k % 7, 200 + k) for k in range(200)]
    counts = []
    for docs in (s, s[:2], s):
        r = _device(ctx, docs, False)
        assert not r.status.any()
        counts.append(ctx.L.cjs_dbg_dec_syncs())
    assert counts[0] == counts[1] == counts[2] and 0 < counts[0] <= 8, counts


def test_python_api():
    from compressjs_amd import Bzip2
    docs = bdc.isolation_set()
    good = [d for k, d in enumerate(docs) if k not in (2, 5, 11)]
    assert Bzip2.decompressFiles([]) == []
    assert Bzip2.decompressFiles(good) == [Bzip2.decompressFile(d) for d in good]
    assert Bzip2.decompressFiles([bytearray(good[0]), np.frombuffer(good[1], dtype=np.uint8)], True) == [Bzip2.decompressFile(d) for d in good[:2]]
    singles = {}
    for k in (2, 5, 11):
        with pytest.raises(TypeError) as e:
            Bzip2.decompressFile(docs[k])
        singles[k] = e.value
    with pytest.raises(TypeError) as e:
        Bzip2.decompressFiles(docs)
    assert e.value.index == 2 and e.value.errorCode == singles[2].errorCode and str(e.value) == str(singles[2])
    res = Bzip2.decompressFiles(docs, False, True)
    for k, x in enumerate(res):
        if k in singles:
            assert type(x) is type(singles[k]) and x.index == k and x.errorCode == singles[k].errorCode and str(x) == str(singles[k])
        else:
            assert x == Bzip2.decompressFile(docs[k])
