#!/usr/bin/env python3
"""Regenerate tests/golden/golden_bwtc_empty.json: the REFERENCE's BWTC stream of the empty input at every level (the batch tests
of tests/batch_scale_cases.py put empty documents into batches of levels 3, 6 and 7; golden.json has levels 1 and 9 only).  Runs
cscott/compressjs under node through ref_runner.js, like make_golden.py.  Build-container only; the tests never execute this.
Usage: python tests/golden/make_golden_bwtc_empty.py"""
import json
import os
import subprocess
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))


def main():
    tmp = tempfile.mkdtemp(prefix="golden-")
    p = os.path.join(tmp, "empty.bin")
    open(p, "wb").close()
    jobs = [dict(id="empty:bwtc:%d" % lv, kind="bwtc", input=p, level=lv) for lv in range(1, 10)]
    jp, rp = os.path.join(tmp, "jobs.json"), os.path.join(tmp, "res.json")
    json.dump(jobs, open(jp, "w"))
    subprocess.check_call(["node", os.path.join(HERE, "ref_runner.js"), jp, rp])
    gold = {}
    for r in json.load(open(rp)):
        gold[r.pop("id")] = {k: r[k] for k in ("kind", "level", "in_len", "out_len", "out_hex", "out_sha256")}
    meta = dict(node=subprocess.check_output(["node", "--version"]).decode().strip(),
                reference="cscott/compressjs @ /root/reference (package.json version 1.0.3-git)")
    json.dump(dict(meta=meta, vectors=gold), open(os.path.join(HERE, "golden_bwtc_empty.json"), "w"), indent=0, sort_keys=True)
    print("wrote", len(gold), "vectors")


if __name__ == "__main__":
    main()
