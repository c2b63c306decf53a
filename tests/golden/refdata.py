"""The reference's test inputs, stored in the repository under tests/golden/fixtures: test/sample0..5.ref
(xz-compressed, sampleK.ref.xz) and the libbzip2-made test/sample0..4.bz2 the decoder cases read (as they are).
read(name) gives the original bytes of test/<name>; nothing here looks outside the repository."""
from __future__ import annotations

import functools
import lzma
import os

import numpy as np

DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "fixtures")


@functools.lru_cache(maxsize=None)
def _load(name: str):
    p = os.path.join(DIR, name)
    if os.path.exists(p):
        with open(p, "rb") as f:
            return f.read()
    if os.path.exists(p + ".xz"):
        with open(p + ".xz", "rb") as f:
            return lzma.decompress(f.read())
    return None


def read(name: str):
    """test/<name> as a fresh np.uint8 array, or None if no such fixture is stored."""
    b = _load(name)
    return None if b is None else np.frombuffer(b, dtype=np.uint8).copy()


def read_bytes(name: str):
    return _load(name)
