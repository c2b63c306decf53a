"""off[0] > 0 on the CPU logic build (tests/emu), host forms: the four batch entries and cjs_unbwt_linear_batch with the documents
behind a prefix of 0, 5 and 261 bytes (tests/batch_scale_cases.check_offsets).  The other sets of batch_scale_cases need an MI355X:
this build takes minutes for 1 100 documents (tests/test_gpu_batch_scale.py runs them)."""
import json
import os

import pytest

import batch_scale_cases as sc
import stagelib
from compressjs_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def emu():
    L = _lib.load(stagelib.build_emu())
    h = L.cjs_create(0, 2)
    assert h
    yield L, h
    L.cjs_destroy(h)


def test_documents_need_not_start_at_offset_zero(emu):
    """path 7, off[0] > 0: five documents (one empty, the first begins with a run) behind 0, 5 and 261 bytes that end in a run of the
    first document's first byte - bzip2 against the oracle, BWTC against the reference's digests, the decoders against the inputs"""
    with open(os.path.join(ROOT, "tests", "golden", "golden_bwtc.json")) as f:
        gbwtc = json.load(f)["vectors"]
    sc.check_offsets(emu[0], emu[1], gbwtc, (False,), "host")
