"""Batched bzip2 on the MI355X (cjs_bz2_compress_batch / _batch_device through compressjs_amd.bzip2): N documents in one call, every
stream bit-identical to the single call on that document.  The arbiter is the oracle, which the suite pins to the reference."""
import numpy as np
import pytest

import batch_cases as bc
import oracle
from compressjs_amd import synth

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from compressjs_amd.bzip2 import Context
    c = Context(0, 8)                                  # sub-batches of 8 blocks: set A's documents cross them
    yield c
    c.close()


def _device(c, docs, level):
    import torch
    flat, off = bc.pack(docs)
    cap = int(c.L.cjs_bz2_compress_batch_bound(int(off[-1]), len(docs)))
    d_in = torch.from_numpy(flat).cuda()
    d_off = torch.from_numpy(off.astype(np.int64)).cuda()
    d_out = torch.full((cap,), 0xAA, dtype=torch.uint8, device="cuda")
    d_oo = torch.full((len(docs) + 1,), -1, dtype=torch.int64, device="cuda")
    n = c.compress_many_device(d_in, d_off, d_out, d_oo, level)
    oo = d_oo.cpu().numpy()
    out = d_out[:n].cpu().numpy()
    assert int(oo[0]) == 0 and int(oo[-1]) == n
    return [out[int(oo[k]):int(oo[k + 1])].tobytes() for k in range(len(docs))]


def _same(got, want, docs):
    assert len(got) == len(want)
    for k, (g, w) in enumerate(zip(got, want)):
        assert g == w, (k, docs[k].size, len(g), len(w))


@pytest.mark.parametrize("which", ["A", "B", "B7"])
def test_sets_host_and_device_forms(ctx, which):
    docs = bc.set_a() if which == "A" else bc.set_b(7 if which == "B7" else 0)
    want = bc.reference(bc.set_a(), bc.LEVEL, "A") if which == "A" else bc.reference(bc.set_b(0), bc.LEVEL, "B")
    if which == "B7":
        want = [oracle.bz2_compress(docs[0], bc.LEVEL)] + want
    got = ctx.compress_many(docs, bc.LEVEL)
    _same(got, want, docs)
    if which == "A":
        assert ctx.last_block_count == 10
        assert ctx.decompress(np.frombuffer(b"".join(got), dtype=np.uint8), multistream=True) == b"".join(d.tobytes() for d in docs)
    _same(_device(ctx, docs, bc.LEVEL), want, docs)


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
    want = [oracle.bz2_compress(d, 1) for d in docs]
    c = Context()
    try:
        _same(c.compress_many(docs, 1), want, docs)
    finally:
        c.close()


def test_documents_that_span_sub_batches(ctx):
    docs = [synth.text_like(250000, 40 + k) if k % 2 else synth.runs_mixed(250000, 40 + k) for k in range(5)]
    want = [oracle.bz2_compress(d, 1) for d in docs]
    _same(ctx.compress_many(docs, 1), want, docs)
    _same(_device(ctx, docs, 1), want, docs)


def test_compress_files_api_and_bad_level():
    from compressjs_amd import Bzip2
    docs = [b"", b"hello hello hello", bytearray(b"a" * 1000), np.arange(300, dtype=np.uint8)]
    got = Bzip2.compressFiles(docs, 9)
    assert got == [Bzip2.compressFile(d, None, 9) for d in docs] == [oracle.bz2_compress(d, 9) for d in docs]
    assert Bzip2.compressFiles([]) == []
    for bad in (0, 10, 2.5):
        with pytest.raises(ValueError) as e1:
            Bzip2.compressFiles(docs, bad)
        with pytest.raises(ValueError) as e2:
            Bzip2.compressFile(docs[1], None, bad)
        assert str(e1.value) == str(e2.value) == "Invalid block size multiplier"
