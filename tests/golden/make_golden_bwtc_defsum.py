#!/usr/bin/env python3
"""tests/golden/golden_bwtc_defsum.json: the REFERENCE's BWTC output (length + sha256) at levels 1-5 (DefSumModel, lib/BWTC.js:107)
for the documents of tests/defsum_cases.py, whose BWT + MTF output is hostile to the model.  Needs node and the reference (ref_runner.js finds it, COMPRESSJS_REF overrides); ref_runner.js is used as it is, kind "bwtc".
Usage: python tests/golden/make_golden_bwtc_defsum.py"""
import json
import os
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))
import defsum_cases as dc  # noqa: E402


def main():
    tmp = tempfile.mkdtemp(prefix="golden-bwtc-defsum-")
    jobs = []
    for i in range(dc.N_DOCS):
        d, lv = dc.doc(i)
        p = os.path.join(tmp, "d%d.bin" % i)
        d.tofile(p)
        jobs.append(dict(id="doc%d" % i, kind="bwtc", input=p, level=lv))
    p = os.path.join(tmp, dc.BIG_ID + ".bin")
    dc.big_doc().tofile(p)
    jobs.append(dict(id=dc.BIG_ID, kind="bwtc", input=p, level=dc.BIG_LEVEL))
    jp, rp = os.path.join(tmp, "jobs.json"), os.path.join(tmp, "res.json")
    json.dump(jobs, open(jp, "w"))
    subprocess.check_call(["node", os.path.join(HERE, "ref_runner.js"), jp, rp])
    gold = {}
    for r in json.load(open(rp)):
        gold[r["id"]] = dict(level=r["level"], in_len=r["in_len"], in_sha256=r["in_sha256"], out_len=r["out_len"], out_sha256=r["out_sha256"])
    meta = dict(node=subprocess.check_output(["node", "--version"]).decode().strip(),
                reference="cscott/compressjs (package.json version 1.0.3-git)")
    json.dump(dict(meta=meta, vectors=gold), open(os.path.join(HERE, "golden_bwtc_defsum.json"), "w"), indent=0, sort_keys=True)
    print("wrote", len(gold), "vectors")


if __name__ == "__main__":
    main()
