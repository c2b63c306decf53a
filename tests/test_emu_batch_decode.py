"""cjs_bz2_decompress_batch on the CPU logic build (tests/emu): N .bz2 documents in, the decoded bytes or the reference's error
of each out, every one as the single call gives it for that document alone.  A context of 2 blocks; output, out_off, status and
detail are pre-filled with stale values.  Not a parity claim for the GPU build (tests/test_gpu_batch_decode.py is)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import batch_decode_cases as bdc
import oracle
import stagelib
from compressjs_amd import _lib

ROOT = stagelib.ROOT


@pytest.fixture(scope="module")
def emu_ctx():
    L = _lib.load(stagelib.build_emu())
    h = L.cjs_create(0, 2)
    assert h
    yield L, h
    L.cjs_destroy(h)


@pytest.fixture(scope="module")
def small_catalogue():
    return bdc.catalogue(4096), bdc.golden_decode()


def test_catalogue_as_one_batch_per_flag(emu_ctx, small_catalogue):
    """Truncations sit directly in front of valid neighbours here: a document that read past its end would decode the next one's
    bytes instead of zeros."""
    L, h = emu_ctx
    by, g = small_catalogue
    assert (len(by[False][0]), len(by[True][0])) == (93, 5)
    ok = sum(1 for ms in by for sid in by[ms][0] if g[sid]["ok"])
    assert (ok, 98 - ok) == (37, 61)
    for ms in (False, True):
        ids, streams = by[ms]
        r = bdc.run_batch(L, h, streams, ms)
        bdc.check_vs_golden(r, ids, g, "ms=%d" % ms)


@pytest.mark.parametrize("filler", [1, 3, 4, 7, 15])
def test_every_alignment_behind_a_garbage_document(emu_ctx, small_catalogue, filler):
    L, h = emu_ctx
    by, g = small_catalogue
    ids, streams = by[False]
    junk = bytes(np.random.RandomState(filler).randint(0, 256, size=filler).astype(np.uint8).tolist())
    r = bdc.run_batch(L, h, [junk] + streams, False)
    assert int(r.status[0]) == -2 and int(r.detail[0]) == 1 and r.docs[0] == b""          # 'bad magic'
    rest = bdc.Result(r.ret, r.out_off[1:] - r.out_off[1], r.status[1:], r.detail[3:], r.docs[1:])
    bdc.check_vs_golden(rest, ids, g, "filler=%d" % filler)


def test_magic_straddling_a_document_end(emu_ctx):
    L, h = emu_ctx
    s = bdc.one_block(5)
    sets = [[s[:7], s[7:], s],                               # cut inside the block magic
            [s[:len(s) - 7], s[len(s) - 7:], s],             # cut inside the end-of-stream magic
            [s[:len(s) - 5], s, s[:len(s) - 4], s]]          # the stream CRC cut off: zeros, not the neighbour's "BZh9"
    pad = bdc.one_block(6, 900)
    while len(pad) % 256:                                    # a document whose length is an exact multiple of 256, then a valid one
        pad += b"\x00"
    sets.append([pad, s])
    sets.append([pad[:256], s, pad[:512], s])
    for ms in (False, True):
        for k, docs in enumerate(sets):
            bdc.check_vs_oracle(bdc.run_batch(L, h, docs, ms), docs, ms, "set %d ms=%d" % (k, ms))


def test_empty_inputs(emu_ctx):
    L, h = emu_ctx
    assert L.cjs_bz2_decompress_batch(h, None, None, 0, 0, None, 0, None, None, None) == 0
    assert L.cjs_bz2_decompress_batch_device(h, None, None, 0, 0, None, 0, None, None, None) == 0
    for count in (1, 5):
        r = bdc.run_batch(L, h, [b""] * count, False)
        assert r.ret == 0 and r.out_off.tolist() == [0] * (count + 1)
        assert r.status.tolist() == [-2] * count and r.detail[0::3].tolist() == [1] * count
    empty = oracle.bz2_compress(np.zeros(0, np.uint8), 9)      # enc:empty decodes to 0 bytes
    docs = [bdc.one_block(1), empty, bdc.one_block(2)]
    r = bdc.run_batch(L, h, docs, False)
    bdc.check_vs_oracle(r, docs, False)
    assert int(r.status[1]) == 0 and r.out_off[1] == r.out_off[2]


@pytest.mark.parametrize("device", [False, True])
def test_error_isolation_and_gap_closing(emu_ctx, device):
    L, h = emu_ctx
    docs = bdc.isolation_set()
    r = bdc.run_batch(L, h, docs, False, device=device)
    bdc.check_vs_oracle(r, docs, False)
    bad = [k for k in range(12) if int(r.status[k])]
    assert bad == [2, 5, 11]
    assert [int(r.detail[3 * k]) for k in bad][:2] == [4, 4]           # block CRCs; in document 5 the one of its second block
    want5 = oracle.bz2_decompress(docs[5])
    assert want5[0] == -5 and want5[1] == 4
    for k in bad:
        assert r.out_off[k] == r.out_off[k + 1]
    assert r.ret == sum(len(d) for d in r.docs) == sum(max(oracle.bz2_decompress(d)[0], 0) for d in docs)


def test_call_level_codes(emu_ctx):
    L, h = emu_ctx
    docs = [bdc.one_block(3), bdc.one_block(4, 50)]
    want = [oracle.bz2_decompress(d)[2] for d in docs]
    total = sum(len(w) for w in want)
    flat, off = bdc.pack(docs)
    bad = np.array([0, len(docs[0]), 5], dtype=np.uint64)             # decreasing offsets
    for fn in (L.cjs_bz2_decompress_batch, L.cjs_bz2_decompress_batch_device):
        out = np.full(total + 64, 0xAA, np.uint8)
        oo = np.full(3, 0xEEEE, np.uint64)
        st = np.full(2, 77, np.int32)
        det = np.full(6, 0xDDDD, np.uint32)
        a = [h, flat.ctypes.data, off.ctypes.data, 2, 0, out.ctypes.data, total + 64, oo.ctypes.data, st.ctypes.data, det.ctypes.data]

        def call(**kw):
            b = list(a)
            for k, v in kw.items():
                b[int(k[1:])] = v
            return fn(*b)
        assert call(_0=None) == -22                                   # ctx
        assert call(_1=None) == -22                                   # null `in` with a non-empty batch
        assert call(_2=None) == -22                                   # off
        assert call(_7=None) == -22                                   # out_off
        assert call(_8=None) == -22                                   # status
        assert call(_2=bad.ctypes.data) == -22
        assert call(_6=total - 1) == -21                              # one byte short: the outcomes are there, the bytes stay fetchable
        assert oo.tolist() == [0, len(want[0]), total] and st.tolist() == [0, 0] and det.tolist() == [0] * 6
        assert L.cjs_bz2_last_size(h) == total
        got = np.zeros(total, np.uint8)
        assert L.cjs_bz2_fetch(h, got.ctypes.data, total) == total and got.tobytes() == b"".join(want)
        oo[:] = 0xEEEE
        st[:] = 77
        assert call(_9=None) == total                                 # detail == NULL is accepted
        assert out[:total].tobytes() == b"".join(want) and oo.tolist() == [0, len(want[0]), total] and st.tolist() == [0, 0]
        assert call(_6=total) == total


def test_single_call_unchanged_after_a_batch_call(emu_ctx, small_catalogue):
    from decode_check import check_stream
    L, h = emu_ctx
    by, g = small_catalogue
    ids, streams = by[False]
    r = bdc.run_batch(L, h, streams[:20], False)
    assert r.ret > 0
    for sid in ("enc:text1k:9", "trunc:text1k:40", "flip:blockcrc", "flip:streamcrc"):
        check_stream(L, h, sid, streams[ids.index(sid)], False, g[sid])


def test_differential_fuzz_vs_oracle():
    """40 batches of 1..12 generated, mutated and concatenated documents with a random flag.  In a subprocess with a timeout: a
    hang must fail, not block the suite."""
    stagelib.build_emu()
    code = r"""
import sys
sys.path.insert(0, %r); sys.path.insert(0, %r); sys.path.insert(0, %r)
import stagelib
import batch_decode_cases as bdc
from compressjs_amd import _lib
L = _lib.load(stagelib.EMU_SO)
h = L.cjs_create(0, 2)
n = 0
for docs, ms in bdc.fuzz_batches(20261018, 40, 12):
    bdc.check_vs_oracle(bdc.run_batch(L, h, docs, ms, device=bool(n & 1)), docs, ms, "batch %%d" %% n)
    n += 1
print("ok", n)
""" % (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "golden"))
    out = subprocess.check_output([sys.executable, "-c", code], timeout=600).decode()
    assert out.strip().endswith("ok 40")


def test_sync_count_does_not_grow_with_the_documents(emu_ctx):
    """No per-document host<->device traffic: 200 one-block documents cost as many synchronisations as 2 (both batches lie inside
    one slot batch)."""
    L, h = emu_ctx
    s = [bdc.one_block(50 + k % 7, 200 + k) for k in range(200)]
    want = [oracle.bz2_decompress(x)[2] for x in s[:7]]
    counts = []
    for docs in (s, s[:2], s):
        r = bdc.run_batch(L, h, docs, False, device=True, cap=1 << 20)
        assert r.ret > 0 and not r.status.any() and r.docs[:2] == want[:2]
        counts.append(L.cjs_dbg_dec_syncs())
    assert counts[0] == counts[1] == counts[2] and 0 < counts[0] <= 8, counts
