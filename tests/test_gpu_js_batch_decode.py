"""Bzip2.decompressFiles of the Node.js drop-in (js/index.js -> addon.decompressMany -> cjs_bz2_decompress_batch): every Buffer of a
batch against Bzip2.decompressFile on the same input, and the errors of corrupt documents against what decompressFile throws."""
import json
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


def test_node_decompress_files():
    if shutil.which("node") is None or not os.path.exists(os.path.join(ROOT, "build", "compressjs_amd.node")):
        pytest.skip("node or the addon is not available on this box")
    out = subprocess.check_output(["node", os.path.join(ROOT, "js", "batchdecodetest.js")], cwd=ROOT, timeout=300)
    r = json.loads(out.decode().strip().splitlines()[-1])
    assert len(r["inputs"]) == 10 and r["batch"] == r["single"] == r["inputs"] and r["none"] == 0
    assert r["bad"] == [3, 6]
    single = {int(k): v for k, v in r["single_err"].items()}
    for k in (3, 6):
        assert single[k]["ctor"] == "TypeError" and single[k]["errorCode"] in (-2, -5), single
    assert single[3]["message"].startswith("Data error: Bad block CRC")
    assert r["thrown"] == dict(single[3], index=3)                   # the first failing document
    for k, x in enumerate(r["kept"]):
        if k in single:
            assert x == dict(single[k], index=k), (k, x)
        else:
            assert x == r["inputs"][k], k
