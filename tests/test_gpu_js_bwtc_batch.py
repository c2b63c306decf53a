"""BWTC.compressFiles of the Node.js drop-in (js/index.js -> addon.bwtcCompressMany -> cjs_bwtc_compress_batch): every stream of a
batch against BWTC.compressFile on the same input and, for the committed cases, the reference-made golden digests."""
import json
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


def test_node_bwtc_compress_files(golden):
    if shutil.which("node") is None or not os.path.exists(os.path.join(ROOT, "build", "compressjs_amd.node")):
        pytest.skip("node or the addon is not available on this box")
    out = subprocess.check_output(["node", os.path.join(ROOT, "js", "bwtcbatchtest.js")], cwd=ROOT, timeout=300)
    r = json.loads(out.decode().strip().splitlines()[-1])
    assert r["names"][:3] == ["empty", "a1000", "bytes40"] and len(r["names"]) == 5
    for level in ("9", "6", "3"):
        assert len(r["batch"][level]) == 5 and r["batch"][level] == r["single"][level], level
    assert r["batch"]["9"][1] == golden["a1000:bwtc:9"]["out_sha256"]
    assert r["batch"]["9"][0] == golden["empty:bwtc:9"]["out_sha256"]
    assert r["batch"]["6"][2] == golden["bytes40:bwtc:6"]["out_sha256"]
    assert r["exact"] is True and r["none"] == 0
    assert r["badlevel"] == r["batch"]["9"][:3]
