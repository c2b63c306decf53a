"""The batch entries on the MI355X beyond the sizes the other batch tests have: more than 1 024 documents, more than 64 block slots
in a sub-batch, more than one group of the batched inverse BWT, and documents that do not start at in[0].  Seven paths exist only
there (numbered as in the docstrings below):
  1  per = ceil(count / 1024) >= 2 in k11_plan, k11_offsets and k12_plan: a thread owns a run of documents
  2  k0_docs_scan's second chunk of 1 024 documents and its carry
  3  k9_docs_meta with several workgroups, k9_docs_gather over many failed documents
  4  k11_code's second workgroup: a sub-batch of more than 64 block slots
  5  cut_groups / run_groups of cjs_bwtc_batch_dec.hip: a second group of k6_unbwt_batch
  6  CJS_BWTC_DEC_BUDGET: the budget prefix of k12_plan across the threads' runs
  7  off[0] > 0
Every comparison is bit-exact against the oracle (which the suite pins to the reference), the reference-made digests of
tests/golden/, or the input bytes; every document is compared; every output buffer is pre-filled with stale values.  The sets and
runners are in tests/batch_scale_cases.py."""
import json
import os

import numpy as np
import pytest

import batch_cases as bc
import batch_decode_cases as bdc
import batch_scale_cases as sc
import bwtc_batch_decode_cases as dc
import bwtc_cases
import oracle

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def gbwtc():
    with open(os.path.join(ROOT, "tests", "golden", "golden_bwtc.json")) as f:
        return json.load(f)["vectors"]


@pytest.fixture(scope="module")
def ctx():
    from compressjs_amd.bzip2 import Context
    c = Context()                                      # the default: 128 blocks in flight, sub-batches of 64
    yield c
    c.close()


@pytest.fixture(scope="module")
def bz2_set():
    """-> ([documents], [the oracle's level-1 stream of each]), made once"""
    docs = sc.bz2_docs()
    assert len(docs) == sc.COUNT and docs[0].size == docs[-1].size == 0
    return docs, bc.reference(docs, 1, "scale")


@pytest.fixture(scope="module")
def bwtc7(ctx):
    """-> ([case numbers], [documents], out_off, [streams]) of the 2 500 level-7 documents through the host form"""
    ids, docs = sc.bwtc_docs(7)
    oo, streams = sc.compress(ctx.L, ctx.h, "bwtc", docs, 7)
    return ids, docs, oo, streams


def test_bz2_compress_2500_documents(ctx, bz2_set):
    """paths 2 and 3 (compress side of 2): 2 500 documents of 0 .. 700 bytes at level 1 - k0_docs_scan walks three chunks of 1 024
    documents with its carry, runs of empty documents lie across the chunk boundaries.  Every stream is the oracle's, out_off is
    exact, one block per non-empty document; host and device forms."""
    L, h = ctx.L, ctx.h
    docs, want = bz2_set
    for device in (False, True):
        oo, got = sc.compress(L, h, "bz2", docs, 1, device, "torch")
        sc.check_streams_exact(oo, got, want, "device %d" % device)
        assert int(L.cjs_last_block_count(h)) == sum(1 for d in docs if d.size)


def test_bz2_decode_2500_streams_26_of_them_damaged(ctx, bz2_set):
    """path 3: 2 500 streams, so k9_docs_meta runs 2500 / 256 + 1 = 10 workgroups, and every 97th stream (26 of them) is damaged -
    a flipped block-CRC bit, a flipped stream-CRC bit, 9 bytes cut off, in turn - so k9_docs_gather closes 26 gaps.  Every document
    is the oracle's outcome: bytes, or code and detail and no bytes; the result has no gaps; host and device forms."""
    L, h = ctx.L, ctx.h
    docs, streams = bz2_set
    batch = sc.bz2_damage(streams)
    sizes = [max(oracle.bz2_decompress(s, False)[0], 0) for s in batch]
    assert sum(1 for k in sc.BZ2_DAMAGED if sizes[k] == 0) == len(sc.BZ2_DAMAGED) == 26
    want_off = np.concatenate([[0], np.cumsum(sizes)]).tolist()
    r = bdc.run_batch(L, h, batch, False)              # (no room first: the retained result, fetched)
    bdc.check_vs_oracle(r, batch, False, "host")
    assert r.out_off.tolist() == want_off
    for device in (False, True):
        r = sc.bz2_decode(L, h, batch, False, want_off[-1] + 64, device, "torch")
        bdc.check_vs_oracle(r, batch, False, "device %d" % device)
        assert r.out_off.tolist() == want_off
        assert int(np.count_nonzero(r.status)) == 26


def test_bwtc_compress_2500_documents_level_7(ctx, gbwtc, bwtc7):
    """path 1, compress side: 2 500 documents give per = 3 in k11_plan and k11_offsets, thread 833 owns the one document of the
    partial last run and 190 threads own nothing; empty documents at 0, 1 023, 1 024 and 2 499.  Every stream against the
    reference's digest; host and device forms; the device form waits three times."""
    L, h = ctx.L, ctx.h
    ids, docs, _oo, streams = bwtc7
    sc.check_bwtc_digests(streams, ids, 7, gbwtc, "host")
    _oo, got = sc.compress(L, h, "bwtc", docs, 7, True, "torch")
    assert int(L.cjs_dbg_bwtc_batch_syncs(h)) == 3
    sc.check_bwtc_digests(got, ids, 7, gbwtc, "device")


def test_bwtc_compress_2500_documents_level_3_host_tail(ctx, gbwtc):
    """path 1 with the host tail (DefSumModel): k11_plan with per = 3 cuts the blocks, the host codes 2 500 documents in order"""
    ids, docs = sc.bwtc_docs(3)
    _oo, got = sc.compress(ctx.L, ctx.h, "bwtc", docs, 3)
    sc.check_bwtc_digests(got, ids, 3, gbwtc, "level 3")


def test_bwtc_decode_2500_streams(ctx, bwtc7):
    """path 1, decode side: k12_plan with per = 3 and a partial last run.  Every document equals its input, none takes the host path,
    three waits, the declared sizes are the inputs'; host and device forms."""
    L, h = ctx.L, ctx.h
    _ids, docs, _oo, streams = bwtc7
    for device in (False, True):
        r = dc.run_batch(L, h, streams, device=device, mem="torch")
        dc.check_inputs(r, docs, "device %d" % device)
        assert dc.fallbacks(L, h) == 0 and dc.syncs(L, h) == 3
        assert [int(x) for x in r.declared] == [d.size for d in docs]


def test_bwtc_decode_budget_ends_inside_a_threads_run(ctx, bwtc7, monkeypatch):
    """path 6: CJS_BWTC_DEC_BUDGET at about half of the batch's scratch.  With 2 500 documents the budget prefix of k12_plan runs
    through the threads' runs of 3 and ends inside one (p % 3 != 0).  The documents behind the admitted prefix take the host path:
    count - p of them, where p is the longest prefix whose sizes, rounded up to 4, fit the budget; every document still equals its
    input."""
    L, h = ctx.L, ctx.h
    _ids, docs, _oo, streams = bwtc7
    budget, p = sc.budget_for(docs)
    assert p % 3 != 0 and sc.COUNT // 3 < p < 2 * sc.COUNT // 3 + 100 and sc.admitted_prefix(docs, budget) == p
    monkeypatch.setenv("CJS_BWTC_DEC_BUDGET", str(budget))
    total = sum(d.size for d in docs)
    for device in (False, True):
        r = dc.run_batch(L, h, streams, device=device, mem="torch", cap=total)
        print("budget %d: admitted %d, host path %d" % (budget, p, dc.fallbacks(L, h)))
        dc.check_inputs(r, docs, "device %d" % device)
        assert dc.fallbacks(L, h) == sc.COUNT - p


@pytest.mark.parametrize("big_id,before", (("gap1300k_l6", 62), ("rand1250k_l6", 63)))
def test_sub_batch_of_100_slots(gbwtc, big_id, before):
    """path 4: a context of 200 blocks in flight has two streams with a share of 500 / 1000 each, so sub_blocks = 200 * 500 / 1000
    = 100 slots and k11_code launches two workgroups for the first sub-batch (b0 = blockIdx.x * 64 + threadIdx.x).  110 one-block
    level-6 documents, except one of three blocks that lies on slots 62-64 (then 63-65): the lane of workgroup 0 that owns it codes on
    across slot 64, lane 0 of workgroup 1 steps aside.  Every stream against the reference's digest, host and device forms, and the
    batch decoded back to the inputs."""
    from compressjs_amd.bzip2 import Context
    big = {cid: d for cid, d, _lv in bwtc_cases.big_cases()}[big_id]
    ids, docs = sc.slot_docs(big_id, big, before)
    assert len(docs) == 108 and sum((d.size + 599999) // 600000 for d in docs[:before]) == before
    c = Context(0, 200)
    try:
        L, h = c.L, c.h
        for device in (False, True):
            _oo, got = sc.compress(L, h, "bwtc", docs, 6, device, "torch")
            assert int(L.cjs_last_block_count(h)) == 110
            sc.check_bwtc_digests(got, ids, 6, gbwtc, "device %d" % device)
            r = dc.run_batch(L, h, got, device=device, mem="torch", cap=sum(d.size for d in docs))
            dc.check_inputs(r, docs, "device %d" % device)
            assert dc.fallbacks(L, h) == 0
    finally:
        c.close()


def test_k6_groups_66000_tiny_blocks(ctx):
    """path 5 by the block count: 66 000 blocks of 1 .. 8 bytes in ONE cjs_unbwt_linear_batch call are two groups, 65 535 + 465
    (K6_GROUP_MAX).  40 BWTs and 10 random (T, pidx) pairs that are no BWT, cycled; the texts are oracle.unbwt_linear's."""
    blocks, pidxs, want = sc.tiny_blocks()
    assert len(blocks) == sc.K6_COUNT
    sc.check_unbwt(ctx.L, blocks, pidxs, want)
    assert sc.k6_groups(ctx.L) >= 2


def test_k6_groups_32_large_blocks(ctx):
    """path 5 by the workspace: 32 blocks of 900 000 bytes (28.8 MB) in ONE call; the 128 Mi words of list-ranking workspace hold 29
    of them, so the 30th starts a second group at wsAt = 0 with its own max_n.  Text-like and random blocks in turn, three small
    blocks between them; the texts are the inputs of oracle.bwt_linear."""
    blocks, pidxs, want = sc.large_blocks()
    assert sum(1 for b in blocks if b.size == 900000) == 32
    assert oracle.unbwt_linear(blocks[1], pidxs[1]).tobytes() == want[1].tobytes()
    sc.check_unbwt(ctx.L, blocks, pidxs, want)
    assert sc.k6_groups(ctx.L) >= 2


def test_k6_groups_bwtc_decode_66000_streams(ctx, gbwtc):
    """paths 5 and 1: 66 000 BWTC streams (about 30 reference-pinned ones of levels 6-9, cycled) in one call: per = 65 in k12_plan,
    66 000 block rows in two groups of k6_unbwt_batch with d_rows + g0.  Every document equals its input (compared on the packed
    result), none takes the host path, three waits; host and device forms."""
    L, h = ctx.L, ctx.h
    docs0, streams0 = sc.pinned_small_streams(L, h, gbwtc)
    docs = [docs0[k % len(docs0)] for k in range(sc.K6_COUNT)]
    batch = [streams0[k % len(streams0)] for k in range(sc.K6_COUNT)]
    total = sum(len(d) for d in docs)
    for device in (False, True):
        r = dc.run_batch(L, h, batch, device=device, mem="torch", cap=total)
        sc.check_packed(r, docs, "device %d" % device)
        assert dc.fallbacks(L, h) == 0 and dc.syncs(L, h) == 3
        assert sc.k6_groups(L) >= 2
        assert np.array_equal(np.asarray(r.declared), np.array([len(d) for d in docs], dtype=np.int64))


def test_documents_need_not_start_at_offset_zero(ctx, gbwtc):
    """path 7, off[0] > 0: five documents (one empty, the first begins with a run) behind 0, 5 and 261 bytes that end in a run of the
    first document's first byte, through all four batch entries in host and device forms and cjs_unbwt_linear_batch - bzip2
    against the oracle, BWTC against the reference's digests, the decoders against the inputs"""
    sc.check_offsets(ctx.L, ctx.h, gbwtc, (False, True), "torch")
