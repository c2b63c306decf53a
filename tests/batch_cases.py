"""Document sets of the batched-compression tests (tests/test_emu_batch.py on the CPU logic build, tests/test_gpu_batch.py on the
GPU): every stream of a batch must equal what the oracle gives for that document alone."""
import numpy as np

import oracle
from compressjs_amd import synth

LEVEL = 1
CAP = 99981                      # level 1: 100000 - 19 (lib/Bzip2.js:892-900)


def _b(x) -> np.ndarray:
    return np.frombuffer(bytes(x), dtype=np.uint8)


def set_a():
    """Empty documents in front, in the middle and at the end; tiny ones; exactly one full block; two blocks; three blocks with a
    block boundary inside a long run."""
    e = np.zeros(0, np.uint8)
    return [e, _b(b"a"), _b(b"a" * 7), _b(b"a" * 300), synth.text_like(5000, 3), e,
            synth.lcg_ascii(CAP, 5), synth.lcg_ascii(CAP + 1, 6),
            np.concatenate([synth.lcg_ascii(CAP - 2, 7), np.full(600, 66, np.uint8), synth.text_like(120000, 8)]), e]


def set_b(filler: int = 0):
    """Boundary hazards over the alphabet {a, b}: documents that end in a run whose byte the next one starts with, runs of exactly 4
    and of exactly 255 + 4 bytes at a document's end, empty documents in between, and 9 000 equal bytes (three 4096-byte tiles)
    between neighbours that end / start with the same byte.  filler: bytes of a leading document that shifts every document
    start (1..15: every alignment mod 16)."""
    rng = np.random.RandomState(20261018)
    docs = []
    if filler:
        docs.append(np.random.RandomState(filler).randint(97, 99, size=filler).astype(np.uint8))   # (its own generator: the set stays the same)
    last = None                                  # the byte the document in front ended with
    for i in range(40):
        kind = i % 10
        if kind == 7:
            docs.append(np.zeros(0, np.uint8))   # (an empty document between two that share the boundary byte)
            continue
        if i == 23:
            c = last if last is not None else 97
            docs.append(np.full(9000, c, np.uint8))
            continue
        parts = []
        if last is not None:
            parts.append(np.full(int(rng.randint(1, 6)), last, np.uint8))          # starts with the byte the neighbour ended with
        parts.append(rng.randint(97, 99, size=int(rng.randint(0, 120))).astype(np.uint8))
        c = int(rng.randint(97, 99))
        parts.append(np.full(1, 195 - c, np.uint8))                                # the other letter: the tail run starts here
        tail = 4 if kind in (2, 5) else (259 if kind in (3, 8) else int(rng.randint(1, 9)))
        parts.append(np.full(tail, c, np.uint8))
        docs.append(np.concatenate(parts))
        last = c
    return docs


_ref_cache = {}


def reference(docs, level, key):
    """oracle.bz2_compress of every document, computed once per set."""
    if key not in _ref_cache:
        _ref_cache[key] = [oracle.bz2_compress(d, level) for d in docs]
    return _ref_cache[key]


def pack(docs):
    off = np.zeros(len(docs) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([d.size for d in docs], dtype=np.uint64)
    flat = np.concatenate(docs) if len(docs) and int(off[-1]) else np.zeros(1, np.uint8)
    return np.ascontiguousarray(flat, dtype=np.uint8), off
