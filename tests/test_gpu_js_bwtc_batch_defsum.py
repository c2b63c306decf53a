"""BWTC.compressFiles of the Node.js drop-in at levels 1 and 5 (js/index.js -> addon.bwtcCompressMany -> cjs_bwtc_compress_batch, the
model on the GPU: k13_defsum_model.hip): every stream of a batch against BWTC.compressFile on the same input."""
import json
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


def test_node_bwtc_compress_files_levels_1_and_5():
    if shutil.which("node") is None or not os.path.exists(os.path.join(ROOT, "build", "compressjs_amd.node")):
        pytest.skip("node or the addon is not available on this box")
    out = subprocess.check_output(["node", os.path.join(ROOT, "js", "bwtcbatchdefsumtest.js")], cwd=ROOT, timeout=300)
    r = json.loads(out.decode().strip().splitlines()[-1])
    assert len(r["names"]) == 6
    for level in ("1", "5"):
        assert len(r["batch"][level]) == 6 and r["batch"][level] == r["single"][level], level
        assert len(set(r["batch"][level])) == 6
    assert r["batch"]["1"] != r["batch"]["5"] and r["exact"] is True
