"""BWTC.decompressFiles of the Node.js drop-in (js/index.js -> addon.bwtcDecompressMany -> cjs_bwtc_decompress_batch): every document
of a batch against its input and BWTC.decompressFile on the same stream; damaged streams throw with .index or keep their place."""
import json
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


def test_node_bwtc_decompress_files():
    if shutil.which("node") is None or not os.path.exists(os.path.join(ROOT, "build", "compressjs_amd.node")):
        pytest.skip("node or the addon is not available on this box")
    out = subprocess.check_output(["node", os.path.join(ROOT, "js", "bwtcbatchdectest.js")], cwd=ROOT, timeout=300)
    r = json.loads(out.decode().strip().splitlines()[-1])
    assert len(r["names"]) == 5 and len(set(r["inputs"])) == 5
    for level in ("9", "6", "3"):
        assert r["batch"][level] == r["inputs"] == r["single"][level], level
    assert r["exact"] is True and r["none"] == 0
    assert r["thrown"] == {"message": "Bad magic", "index": 1}
    assert r["single_thrown"]["message"] == "Bad magic"
    assert r["kept"][0] == r["inputs"][1] and r["kept"][2] == r["inputs"][3]
    assert r["kept"][1] == {"message": "Bad magic", "index": 1}
    assert r["kept"][3] == {"message": r["single_cut"]["message"], "index": 3}
