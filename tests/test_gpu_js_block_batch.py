"""Bzip2.decompressBlocks of the Node.js drop-in (js/index.js -> addon.decompressBlocks -> cjs_bz2_decompress_blocks): the shuffled
positions of block_batch_cases.mixed_positions - blocks, end magics, misses, duplicates, positions behind the end up to 2^64 - 1 -
against the oracle's outcome for every position alone, with and without returnErrors."""
import json
import os
import shutil
import subprocess

import pytest

import block_batch_cases as bbc
import decode_chain_cases as dcc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


def test_node_decompress_blocks(tmp_path):
    if shutil.which("node") is None or not os.path.exists(os.path.join(ROOT, "build", "compressjs_amd.node")):
        pytest.skip("node or the addon is not available on this box")
    f = dcc.the_file()
    pos = bbc.mixed_positions()
    (tmp_path / "file.bz2").write_bytes(f.data)
    (tmp_path / "pos.json").write_text(json.dumps([str(p) for p in pos]))
    out = subprocess.check_output(["node", os.path.join(ROOT, "js", "blockbatchtest.js"), str(tmp_path / "file.bz2"),
                                   str(tmp_path / "pos.json")], cwd=ROOT, timeout=300)
    r = json.loads(out.decode().strip().splitlines()[-1])
    assert r["count"] == len(pos) == len(r["kept"]) and r["none"] == 0
    first_bad = None
    for k, p in enumerate(pos):
        n, det, data = bbc.want_of("file", f.data, p)
        if n < 0:
            assert (n, det) == (-2, 0)                                   # (the clean file: misses only)
            want = {"ctor": "TypeError", "errorCode": -2, "message": "Not bzip data", "index": k}
            assert r["kept"][k] == want, (k, p, r["kept"][k])
            first_bad = k if first_bad is None else first_bad
        else:
            want = bbc.sha(data)
            assert r["kept"][k] == want, (k, p)
        if k < len(r["single"]) and r["single"][k] != "skipped":
            assert r["single"][k] == (want if n >= 0 else {x: y for x, y in want.items() if x != "index"}), (k, p)
    assert first_bad is not None
    assert r["thrown"] == {"ctor": "TypeError", "errorCode": -2, "message": "Not bzip data", "index": first_bad}
