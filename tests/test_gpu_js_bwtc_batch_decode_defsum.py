"""BWTC.decompressFiles of the Node.js drop-in on streams of levels 1, 3 and 5 (js/index.js -> addon.bwtcDecompressMany ->
cjs_bwtc_decompress_batch_ex with CJS_BWTC_DEC_DEFSUM_DEVICE, the decoder on the GPU: k14_defsum_decoder.hip): every document equals
its input, and a damaged stream among good ones gives the error object of BWTC.decompressFile."""
import json
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


def test_node_bwtc_decompress_files_levels_1_3_and_5():
    if shutil.which("node") is None or not os.path.exists(os.path.join(ROOT, "build", "compressjs_amd.node")):
        pytest.skip("node or the addon is not available on this box")
    out = subprocess.check_output(["node", os.path.join(ROOT, "js", "bwtcbatchdecdefsumtest.js")], cwd=ROOT, timeout=300)
    r = json.loads(out.decode().strip().splitlines()[-1])
    assert len(r["names"]) == 5 and len(set(r["input"])) == 5 and r["exact"] is True
    for level in ("1", "3", "5"):
        assert r["decoded"][level] == r["input"], level
    mixed, single = r["mixed"], r["mixed_single"]
    assert [mixed[k] for k in (0, 2, 4)] == [r["input"][1], r["input"][2], r["input"][3]]
    for k in (1, 3):
        assert mixed[k]["index"] == k
        assert {"name": mixed[k]["name"], "message": mixed[k]["message"]} == single[k], k
    assert mixed[1]["message"] == "Bad magic"
    assert r["thrown"] == single[1]
