"""The shared case list of the batched BWTC decode with DefSumModel on the device (cjs_bwtc_decompress_batch_ex* with
CJS_BWTC_DEC_DEFSUM_DEVICE; k14_defsum_decoder.hip), run by tests/test_emu_bwtc_batch_decode_defsum.py on the CPU logic build and by
tests/test_gpu_bwtc_batch_decode_defsum.py on the GPU.  The streams come from the existing compress entries and are pinned to the
reference by the digests of golden_bwtc.json / golden_bwtc_defsum.json; the arbiter of a decoded document is its input, of a damaged
stream cjs_bwtc_decompress on it alone, on the same build.  The document sets and checkers are those of bwtc_batch_decode_cases.py,
defsum_cases.py and bwtc_cases.py.

An Env carries what differs between the two builds: the library, a context (and one of 2 blocks in flight), how the device form's
buffers are made, and whether the documents are kept small (the CPU build: at most 6 000 bytes where the set allows)."""
import hashlib
import json
import os

import numpy as np

import bwtc_batch_decode_cases as dc
import bwtc_cases
import defsum_cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEFSUM = 1                                                 # CJS_BWTC_DEC_DEFSUM_DEVICE

TABLE_SHAPES = (1, 2, 3, 4, 61, 62, 63, 64, 125, 126, 127, 128, 189, 190, 191, 254, 255, 256)


class _Ex:
    """the library with the two batch decode entries bound to their _ex forms and a flags word, so that the helpers of
    bwtc_batch_decode_cases.py (run_batch and what it checks around a call) serve the new entries unchanged"""

    def __init__(self, L, flags):
        self._L, self._flags = L, flags

    def cjs_bwtc_decompress_batch(self, *a):
        return self._L.cjs_bwtc_decompress_batch_ex(*a, self._flags)

    def cjs_bwtc_decompress_batch_device(self, *a):
        return self._L.cjs_bwtc_decompress_batch_device_ex(*a, self._flags)

    def __getattr__(self, name):
        return getattr(self._L, name)


def run_batch(L, h, streams, flags=DEFSUM, **kw):
    """dc.run_batch through cjs_bwtc_decompress_batch_ex / _batch_device_ex with `flags`"""
    return dc.run_batch(_Ex(L, flags), h, streams, **kw)


def _vectors(name):
    with open(os.path.join(ROOT, "tests", "golden", name)) as f:
        return json.load(f)["vectors"]


class Env:
    def __init__(self, L, h, h2, mem, small):
        self.L, self.h, self.h2, self.mem, self.small = L, h, h2, mem, small
        self.gbwtc = _vectors("golden_bwtc.json")
        self.gdefsum = _vectors("golden_bwtc_defsum.json")
        self._fuzz, self._head = {}, {}

    def run(self, streams, device=False, flags=DEFSUM, h=None, docs=None, **kw):
        """`docs`: the documents the streams should decode to.  The CPU build gives the call exactly their room, one call a form,
        where the GPU build goes through dc.run_batch's no-room call, the fetch of the retained result and the call again (the CPU
        build keeps that protocol in call_level)"""
        if self.small and docs is not None and "cap" not in kw:
            kw["cap"] = sum(len(d) for d in docs)
        return run_batch(self.L, h or self.h, streams, flags=flags, device=device, mem=self.mem, **kw)

    def both_forms(self):
        return (False, True)

    def fuzz(self, level):
        """-> ([documents], [streams]) of the fuzz cases of a level, made once by the batch compress, digests checked"""
        if level not in self._fuzz:
            ids, docs = dc.fuzz_of_level(level, 6000 if self.small else None)
            streams = dc.compress_many(self.L, self.h, docs, level)
            for i, s in zip(ids, streams):
                assert hashlib.sha256(s).hexdigest() == self.gbwtc["fuzz%d" % i]["out_sha256"], i
            self._fuzz[level] = (docs, streams)
        return self._fuzz[level]

    def fuzz_head(self, level, n=10):
        """the first n fuzz cases of a level alone (levels 6-9, of which the cases here need a few documents only)"""
        if level in self._fuzz:
            return self._fuzz[level][0][:n], self._fuzz[level][1][:n]
        if level not in self._head:
            ids, docs = dc.fuzz_of_level(level, 6000 if self.small else None)
            ids, docs = ids[:n], docs[:n]
            streams = dc.compress_many(self.L, self.h, docs, level)
            for i, s in zip(ids, streams):
                assert hashlib.sha256(s).hexdigest() == self.gbwtc["fuzz%d" % i]["out_sha256"], i
            self._head[level] = (docs, streams)
        return self._head[level]

    def small_streams(self):
        """25 small streams of levels 1-5, five a level: ([documents as bytes], [streams])"""
        docs, streams = [], []
        for level in (1, 2, 3, 4, 5):
            ds, ss = self.fuzz(level)
            pick = [k for k in range(len(ds)) if 17 <= ds[k].size <= 1000][:5]
            assert len(pick) == 5, level
            docs += [ds[k].tobytes() for k in pick]
            streams += [ss[k] for k in pick]
        assert len(streams) >= 24
        return docs, streams

    def pointers(self, arrays):
        """-> (what keeps them alive, [address of every array as the device form takes it])"""
        if self.mem != "torch":
            return arrays, [a.ctypes.data for a in arrays]
        import torch
        t = [torch.from_numpy(a.astype(np.int64) if a.dtype == np.uint64 else a).cuda() for a in arrays]
        return t, [x.data_ptr() for x in t]

    def clean(self):
        return dc.fallbacks(self.L, self.h) == 0 and dc.syncs(self.L, self.h) == 3


# ---- 1
def fuzz_level(E, level):
    docs, streams = E.fuzz(level)
    assert len(docs) >= 15
    for device in E.both_forms():
        r = E.run(streams, device=device, docs=docs)
        dc.check_inputs(r, docs, level)
        assert [int(x) for x in r.declared] == [d.size for d in docs]
        assert E.clean(), (dc.fallbacks(E.L, E.h), dc.syncs(E.L, E.h))


# ---- 2
def hostile_level(E, level):
    """the documents of defsum_cases.doc(i) of one level: the threshold-rule refusal, the cap of 40, re-escapes.  The set has
    documents of 300, 2 000, 9 000 and 30 000 bytes; the CPU build leaves the 30 000-byte ones to the GPU file, which runs all 40"""
    ids = [i for i in range(defsum_cases.N_DOCS) if defsum_cases.doc(i)[1] == level]
    if E.small:
        ids = [i for i in ids if defsum_cases.doc(i)[0].size <= 9000]
    assert len(ids) >= 4
    docs = [defsum_cases.doc(i)[0] for i in ids]
    streams = dc.compress_many(E.L, E.h, docs, level)
    for i, s in zip(ids, streams):
        assert hashlib.sha256(s).hexdigest() == E.gdefsum["doc%d" % i]["out_sha256"], i
    for device in E.both_forms():
        dc.check_inputs(E.run(streams, device=device, docs=docs), docs, level)
        assert E.clean()


# ---- 3
def table_shape_docs():
    """alphabets of k symbols, 700 shuffled bytes each (several rebuilds): the rebuild walks k + 2 entries, 64 a round, and the
    lookup counts over the same rounds - these k sit on both sides of every round boundary"""
    rng = np.random.RandomState(1414)
    return [rng.permutation(np.resize(np.arange(k), 700)).astype(np.uint8) for k in TABLE_SHAPES]


def table_shapes(E):
    docs = table_shape_docs()
    streams = dc.compress_many(E.L, E.h, docs, 2)
    for device in E.both_forms():
        dc.check_inputs(E.run(streams, device=device, docs=docs), docs)
        assert E.clean()


# ---- 4
def runs_and_ends(E, level):
    docs = dc.runs_and_ends_docs()
    streams = dc.compress_many(E.L, E.h, docs, level)
    for device in E.both_forms():
        dc.check_inputs(E.run(streams, device=device, docs=docs), docs)
        assert E.clean()
    r = E.run([streams[0]] * 3)
    assert r.ret == 0 and r.out_off.tolist() == [0, 0, 0, 0] and r.status.tolist() == [0, 0, 0]
    assert dc.fallbacks(E.L, E.h) == 0


# ---- 5
def multi_block(E, cid):
    """a multi-block document between small documents and an empty one, on the context of 2 blocks, cap = the exact total"""
    if cid == defsum_cases.BIG_ID:
        big, level, digest = defsum_cases.big_doc(), defsum_cases.BIG_LEVEL, E.gdefsum[cid]["out_sha256"]
    else:
        big, level = {c: (d, lv) for c, d, lv in bwtc_cases.big_cases()}[cid]
        digest = E.gbwtc[cid]["out_sha256"]
    small, small_s = E.fuzz(level)
    streams = dc.compress_many(E.L, E.h2, [big, np.zeros(0, np.uint8)], level)
    assert hashlib.sha256(streams[0]).hexdigest() == digest, cid
    batch = [small_s[0], streams[0], streams[1], small_s[1]]
    want = [small[0], big, np.zeros(0, np.uint8), small[1]]
    total = sum(w.size for w in want)
    for device in ((False,) if E.small else E.both_forms()):    # (the CPU build: the host form alone - the forms differ in delivery only)
        dc.check_inputs(E.run(batch, device=device, h=E.h2, cap=total), want, cid)
        assert dc.fallbacks(E.L, E.h2) == 0 and dc.syncs(E.L, E.h2) == 3


# ---- 6
def levels_interleaved(E):
    """levels 1..9, two documents each, interleaved: both decode kernels run in one call"""
    per = {lv: E.fuzz(lv) if lv <= 5 else E.fuzz_head(lv) for lv in range(1, 10)}
    docs, batch = [], []
    for k in range(2):
        for lv in range(1, 10):
            docs.append(per[lv][0][k])
            batch.append(per[lv][1][k])
    for device in E.both_forms():
        r = E.run(batch, device=device, docs=docs)
        dc.check_inputs(r, docs)
        assert E.clean()
        r0 = E.run(batch, device=device, flags=0, docs=docs)
        assert r0.docs == r.docs and r0.status.tolist() == r.status.tolist() and r0.declared.tolist() == r.declared.tolist()
        assert dc.fallbacks(E.L, E.h) == 10


# ---- 7
def alignment_and_isolation(E):
    docs, streams = E.small_streams()
    k2 = 5                                                      # the first level-2 stream
    batch = dc.alignment_streams(streams[k2])
    for device in E.both_forms():
        r = E.run(batch, device=device)
        dc.check_vs_single(E.L, E.h, r, batch)
        for k in range(1, 16, 2):
            assert int(r.status[k]) == 0 and r.docs[k] == docs[k2], k
        assert r.status[0] == -30
    pick = list(range(0, 24, 2))                               # twelve streams over levels 1-5
    d12, s12 = [docs[k] for k in pick], [streams[k] for k in pick]
    batch = dc.isolation_streams(s12)
    for device in E.both_forms():
        r = E.run(batch, device=device)
        dc.check_vs_single(E.L, E.h, r, batch)
        assert int(r.status[5]) == -30 and int(r.status[2]) == -31
        for k in range(12):
            if k not in (2, 5, 9):
                assert int(r.status[k]) == 0 and r.docs[k] == d12[k], k


# ---- 8
SWEEP_CLASSES = {-30, -31, "same", "other"}                    # computed on the CPU logic build with the default seed (5)


def sweep(E):
    """every outcome equals the single call's, in both forms.  The class that matters most is 'other' - a damaged stream that decodes
    without error: it is where the device guards and the host guards could part, but only if the stream was decoded on the device (a
    flip in the size or the level byte can send it to the host path, where it agrees with the single call trivially).  So the
    'other' streams go through a batch of their own, with the flag and without: without it every DefSumModel stream among them is
    counted on the host path, with it those that K14 decoded are not - at least one must be (the default seed gives 13, all of them
    on the device; no further seed was needed)"""
    docs, streams = E.small_streams()
    sw = dc.sweep_streams(streams)
    batch = [s for _kind, s, _k in sw]
    r = E.run(batch)
    assert dc.fallbacks(E.L, E.h) < len(batch) // 4
    want = dc.check_vs_single(E.L, E.h, r, batch)
    assert dc.outcome_classes(want, docs, sw) == SWEEP_CLASSES
    rd = E.run(batch, device=True, cap=r.ret)
    assert rd.docs == r.docs and rd.status.tolist() == r.status.tolist() and rd.declared.tolist() == r.declared.tolist()
    other = [j for j, ((st, data), (_kind, _s, k)) in enumerate(zip(want, sw)) if st == 0 and data != docs[k]]
    assert other
    ro = E.run([batch[j] for j in other])
    on_host = dc.fallbacks(E.L, E.h)
    assert ro.status.tolist() == [0] * len(other) and ro.docs == [want[j][1] for j in other]
    r0 = E.run([batch[j] for j in other], flags=0)
    assert r0.docs == ro.docs
    assert dc.fallbacks(E.L, E.h) - on_host >= 1, "no damaged stream that decodes without error was decoded by K14"


# ---- 9
def host_path_between_fast_ones(E):
    """the construction of test_host_path_documents_between_fast_ones with the flag: the level-3 documents are on the device now,
    the four headers that declare -1, 0, 5 and 2^40 (level-3 streams here: K14 is what hands the 0 and the 5 back) still take the
    host path, a level-3 stream that declares more than it holds stays on the fast path"""
    L, h = E.L, E.h
    d8, s8 = E.fuzz_head(8)
    d3, s3 = E.fuzz(3)
    doc = next(d for d in d3 if d.size >= 200)
    mid = [(d3[k], s3[k]) for k in range(6)]
    mid += [(doc, dc.compress_one(L, h, doc, 3, declared)) for declared in (-1, 0, 5, 1 << 40)]
    fast_more = dc.compress_one(L, h, doc, 3, doc.size + 1000)
    docs, batch = [], []
    for k, (d, s) in enumerate(mid):
        docs += [d8[k], d]
        batch += [s8[k], s]
    docs += [doc, d8[0]]
    batch += [fast_more, s8[0]]
    for device in E.both_forms():
        r = E.run(batch, device=device, docs=docs)
        dc.check_inputs(r, docs)
        assert dc.fallbacks(L, h) == 4
        dc.check_vs_single(L, h, r, batch)


# ---- 10
def budget(E, monkeypatch):
    docs, streams = E.fuzz(3)
    monkeypatch.setenv("CJS_BWTC_DEC_BUDGET", "10000")
    r = E.run(streams)
    dc.check_inputs(r, docs)
    assert 0 < dc.fallbacks(E.L, E.h) < len(docs)


# ---- 11
def call_level(E, golden):
    L, h = E.L, E.h
    docs, streams = E.small_streams()
    batch = streams[:3]
    flat, off = dc.pack(batch)
    out = np.zeros(16384, np.uint8)
    oo, st = np.zeros(4, np.uint64), np.zeros(3, np.int32)
    bad = np.array([0, 40, 5, int(off[-1])], dtype=np.uint64)
    keep, ptr = E.pointers((flat, off, out, oo, st, bad))
    a_host = (flat.ctypes.data, off.ctypes.data, 3, out.ctypes.data, 16384, oo.ctypes.data, st.ctypes.data, None)
    a_dev = (ptr[0], ptr[1], 3, ptr[2], 16384, ptr[3], ptr[4], None)
    for fn, a, badp in ((L.cjs_bwtc_decompress_batch_ex, a_host, bad.ctypes.data), (L.cjs_bwtc_decompress_batch_device_ex, a_dev, ptr[5])):
        for flags in (2, 3, 0x80000000, 0x100):
            assert fn(h, *a, flags) == -22                     # an unknown bit
            assert fn(h, None, None, 0, None, 0, None, None, None, flags) == -22
        for flags in (0, DEFSUM):
            assert fn(None, *a, flags) == -22
            assert fn(h, a[0], None, *a[2:], flags) == -22
            assert fn(h, *a[:5], None, a[6], None, flags) == -22
            assert fn(h, *a[:6], None, None, flags) == -22
            assert fn(h, None, *a[1:], flags) == -22           # null `in` with bytes to read
            assert fn(h, a[0], badp, *a[2:], flags) == -22     # decreasing offsets
            assert fn(h, None, None, 0, None, 0, None, None, None, flags) == 0
    del keep
    total = sum(len(d) for d in docs[:3])
    for device in E.both_forms():
        short = E.run(batch, device=device, cap=total - 1)
        assert short.ret == -21 and int(short.out_off[-1]) == total and short.status.tolist() == [0, 0, 0]
        assert int(L.cjs_bwtc_last_size(h)) == total
        kept = np.zeros(total, np.uint8)
        assert L.cjs_bwtc_fetch(h, kept.ctypes.data, total) == total and kept.tobytes() == b"".join(docs[:3])
        exact = E.run(batch, device=device, cap=total)
        assert exact.ret == total and exact.docs == docs[:3]
        assert dc.fallbacks(L, h) == 0
    s = bytes.fromhex(golden["a1000:bwtc:9"]["out_hex"])        # the single call after a batch call: unchanged
    assert dc.single(L, h, s) == (0, b"a" * 1000, 1000)
    assert dc.single(L, h, streams[0]) == (0, docs[0], len(docs[0]))


# ---- 12
def waits(E, counts):
    _docs, streams = E.small_streams()
    s1 = streams[:5]                                           # level 1
    seen = []
    for k in counts:
        batch = [s1[j % len(s1)] for j in range(k)]
        assert E.run(batch, device=True, cap=1 << 18).ret > 0
        assert dc.fallbacks(E.L, E.h) == 0
        seen.append(dc.syncs(E.L, E.h))
    assert seen == [3] * len(counts)
