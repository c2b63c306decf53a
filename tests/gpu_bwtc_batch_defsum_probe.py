"""Throughput probe of the batched BWTC compress at levels 1-5 (not a test): N independent documents of synth.enwik_like through
cjs_bwtc_compress_batch_device (device-resident) and cjs_bwtc_compress_batch (host to host) of THIS build - DefSumModel on the GPU,
k13_defsum_model.hip - against the same two calls of a library built from the parent commit (--parent-lib), which codes these
levels on the host, document after document.  Every shape is warmed up on both libraries first; then the two alternate for
--rounds rounds in the same process on the same GPU.  One sha256 over all streams of a call must be equal for both libraries and
both forms; the waits of a call come from cjs_dbg_bwtc_batch_syncs.  The condition: this build is faster than the parent's same
call by more than the spread of the rounds (its slowest round against the parent's fastest), at every shape, level and form.
    python tests/gpu_bwtc_batch_defsum_probe.py --parent-lib PATH [--levels 1,5] [--shapes 1000x100000,10000x10000] [--rounds 3]"""
import argparse
import hashlib
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
from compressjs_amd import _lib, synth

ap = argparse.ArgumentParser()
ap.add_argument("--parent-lib", required=True)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--shapes", default="1000x100000,10000x10000")
ap.add_argument("--levels", default="1,5")
ap.add_argument("--blocks", type=int, default=128)
args = ap.parse_args()

libs = [("this build", _lib.load()), ("parent build", _lib.load(args.parent_lib))]
ctxs = []
for name, L in libs:
    h = L.cjs_create(0, args.blocks)
    assert h, name
    ctxs.append((name, L, h))
gate_ok = True
for level in (int(x) for x in args.levels.split(",")):
    for shape in args.shapes.split(","):
        count, size = (int(x) for x in shape.split("x"))
        flat = np.ascontiguousarray(synth.enwik_like(count * size, 77))
        off = (np.arange(count + 1, dtype=np.uint64) * np.uint64(size))
        total = count * size
        tag = "%d x %d B, level %d" % (count, size, level)
        cap = int(libs[0][1].cjs_bwtc_compress_batch_bound(total, count))
        d_in = torch.from_numpy(flat).cuda()
        d_off = torch.from_numpy(off.astype(np.int64)).cuda()
        d_out = torch.empty(cap, dtype=torch.uint8, device="cuda")
        d_oo = torch.empty(count + 1, dtype=torch.int64, device="cuda")
        out = np.zeros(cap, np.uint8)
        out_off = np.zeros(count + 1, np.uint64)

        def device(L, h):
            """-> (seconds, bytes, waits, sha256 of the streams back to back)"""
            d_out.zero_()
            torch.cuda.synchronize()
            a = time.perf_counter()
            n = int(L.cjs_bwtc_compress_batch_device(h, d_in.data_ptr(), d_off.data_ptr(), count, level, d_out.data_ptr(), cap, d_oo.data_ptr()))
            w = time.perf_counter() - a
            assert n > 0, n
            waits = int(L.cjs_dbg_bwtc_batch_syncs(h))
            torch.cuda.synchronize()
            assert int(d_oo[-1].item()) == n
            return w, n, waits, hashlib.sha256(d_out[:n].cpu().numpy().tobytes()).hexdigest()[:16]

        def host(L, h):
            out[:] = 0
            a = time.perf_counter()
            n = int(L.cjs_bwtc_compress_batch(h, flat.ctypes.data, off.ctypes.data, count, level, out.ctypes.data, cap, out_off.ctypes.data))
            w = time.perf_counter() - a
            assert n > 0 and int(out_off[-1]) == n, n
            return w, n, int(L.cjs_dbg_bwtc_batch_syncs(h)), hashlib.sha256(out[:n].tobytes()).hexdigest()[:16]

        forms = (("device-resident", device), ("host to host", host))
        for name, L, h in ctxs:                            # warm-up of every path at this shape (workspaces grow, code objects load)
            for _, fn in forms:
                fn(L, h)
        times = {(f, name): [] for f, _ in forms for name, _, _ in ctxs}
        waits, digests, nbytes = {}, set(), set()
        for r in range(args.rounds):
            for f, fn in forms:
                for name, L, h in ctxs:
                    w, n, s, dg = fn(L, h)
                    times[(f, name)].append(w)
                    waits[(f, name)] = s
                    digests.add(dg)
                    nbytes.add(n)
            print("%s: round %d: " % (tag, r + 1) + "; ".join("%s %s %.2f ms" % (f, name, times[(f, name)][-1] * 1e3) for f, _ in forms for name, _, _ in ctxs), flush=True)
        assert len(digests) == 1 and len(nbytes) == 1, (digests, nbytes)
        for f, _ in forms:
            mine, theirs = times[(f, "this build")], times[(f, "parent build")]
            print("%s: %s: this build %.2f .. %.2f ms (%.0f MB/s best, %d waits), parent build %.2f .. %.2f ms (%.0f MB/s best, %d waits); parent's fastest / this build's slowest = %.2fx"
                  % (tag, f, min(mine) * 1e3, max(mine) * 1e3, total / min(mine) / 1e6, waits[(f, "this build")], min(theirs) * 1e3, max(theirs) * 1e3,
                     total / min(theirs) / 1e6, waits[(f, "parent build")], min(theirs) / max(mine)), flush=True)
            if max(mine) >= min(theirs):
                print("%s: %s: CONDITION NOT MET - this build's slowest round is not faster than the parent's fastest" % (tag, f), flush=True)
                gate_ok = False
        print("%s: %d -> %d bytes; digest of all streams %s, equal for both builds and both forms" % (tag, total, nbytes.pop(), digests.pop()), flush=True)
        del d_in, d_out
for name, L, h in ctxs:
    L.cjs_destroy(h)
sys.exit(0 if gate_ok else 1)
