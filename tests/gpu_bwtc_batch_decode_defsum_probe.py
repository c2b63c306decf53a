"""Throughput probe of the batched BWTC decode at levels 1-5 (not a test): N independent documents of synth.enwik_like, compressed
once by bwtc_compress_many, back through cjs_bwtc_decompress_batch_device_ex (device-resident) and cjs_bwtc_decompress_batch_ex (host
to host) of THIS build with CJS_BWTC_DEC_DEFSUM_DEVICE - DefSumModel's decoder on the GPU, k14_defsum_decoder.hip - against the plain
entries of a library built from the parent commit (--parent-lib) on the same bytes, which decodes these levels on the host,
document after document.  Every shape is warmed up on both libraries first; then the two alternate for --rounds rounds in the same
process on the same GPU.  Reported per call: wall time, waits (cjs_dbg_bwtc_dec_batch_syncs), documents on the host path
(cjs_dbg_bwtc_dec_batch_fallbacks) and one sha256 over all decoded documents, which must be equal for both libraries and both forms
and equal to the inputs'.  The condition: this build's slowest round is faster than the parent's fastest round, at every shape,
level and form.  --only-batch: this build alone (no --parent-lib needed), for a kernel trace of the batch call.
    python tests/gpu_bwtc_batch_decode_defsum_probe.py --parent-lib PATH [--levels 1,5] [--shapes 1000x100000,10000x10000] [--rounds 3]"""
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
from compressjs_amd.bzip2 import Context

ap = argparse.ArgumentParser()
ap.add_argument("--parent-lib")
ap.add_argument("--only-batch", action="store_true")
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--shapes", default="1000x100000,10000x10000")
ap.add_argument("--levels", default="1,5")
ap.add_argument("--blocks", type=int, default=128)
args = ap.parse_args()
assert args.only_batch or args.parent_lib, "--parent-lib PATH, or --only-batch"

libs = [("this build", _lib.load(), True)]
if not args.only_batch:
    libs.append(("parent build", _lib.load(args.parent_lib), False))
ctxs = []
for name, L, ex in libs:
    h = L.cjs_create(0, args.blocks)
    assert h, name
    ctxs.append((name, L, h, ex))
maker = Context(0, args.blocks)
gate_ok = True
for level in (int(x) for x in args.levels.split(",")):
    for shape in args.shapes.split(","):
        count, size = (int(x) for x in shape.split("x"))
        data = np.ascontiguousarray(synth.enwik_like(count * size, 77))
        total = count * size
        want = hashlib.sha256(data.tobytes()).hexdigest()[:16]
        streams = maker.bwtc_compress_many([data[k * size:(k + 1) * size] for k in range(count)], level)
        flat = np.frombuffer(b"".join(streams), dtype=np.uint8)
        off = np.zeros(count + 1, np.uint64)
        off[1:] = np.cumsum([len(s) for s in streams], dtype=np.uint64)
        del streams
        tag = "%d x %d B, level %d" % (count, size, level)
        d_in = torch.from_numpy(flat.copy()).cuda()
        d_off = torch.from_numpy(off.astype(np.int64)).cuda()
        d_out = torch.empty(total, dtype=torch.uint8, device="cuda")
        d_oo = torch.empty(count + 1, dtype=torch.int64, device="cuda")
        d_st = torch.empty(count, dtype=torch.int32, device="cuda")
        out = np.zeros(total, np.uint8)
        out_off = np.zeros(count + 1, np.uint64)
        status = np.zeros(count, np.int32)

        def device(L, h, ex):
            """-> (seconds, waits, documents on the host path, sha256 of the documents back to back)"""
            d_out.zero_()
            torch.cuda.synchronize()
            a = (h, d_in.data_ptr(), d_off.data_ptr(), count, d_out.data_ptr(), total, d_oo.data_ptr(), d_st.data_ptr(), None)
            t0 = time.perf_counter()
            n = int(L.cjs_bwtc_decompress_batch_device_ex(*a, 1) if ex else L.cjs_bwtc_decompress_batch_device(*a))
            w = time.perf_counter() - t0
            assert n == total, n
            torch.cuda.synchronize()
            assert int(d_st.abs().max().item()) == 0
            return w, int(L.cjs_dbg_bwtc_dec_batch_syncs(h)), int(L.cjs_dbg_bwtc_dec_batch_fallbacks(h)), hashlib.sha256(d_out.cpu().numpy().tobytes()).hexdigest()[:16]

        def host(L, h, ex):
            out[:] = 0
            a = (h, flat.ctypes.data, off.ctypes.data, count, out.ctypes.data, total, out_off.ctypes.data, status.ctypes.data, None)
            t0 = time.perf_counter()
            n = int(L.cjs_bwtc_decompress_batch_ex(*a, 1) if ex else L.cjs_bwtc_decompress_batch(*a))
            w = time.perf_counter() - t0
            assert n == total and not status.any(), n
            return w, int(L.cjs_dbg_bwtc_dec_batch_syncs(h)), int(L.cjs_dbg_bwtc_dec_batch_fallbacks(h)), hashlib.sha256(out.tobytes()).hexdigest()[:16]

        forms = (("device-resident", device), ("host to host", host))
        for name, L, h, ex in ctxs:                        # warm-up of every path at this shape (workspaces grow, code objects load)
            for _, fn in forms:
                fn(L, h, ex)
        times = {(f, name): [] for f, _ in forms for name, _, _, _ in ctxs}
        waits, fbs, digests = {}, {}, set()
        for r in range(args.rounds):
            for f, fn in forms:
                for name, L, h, ex in ctxs:
                    w, s, fb, dg = fn(L, h, ex)
                    times[(f, name)].append(w)
                    waits[(f, name)], fbs[(f, name)] = s, fb
                    digests.add(dg)
            print("%s: round %d: " % (tag, r + 1) + "; ".join("%s %s %.2f ms" % (f, name, times[(f, name)][-1] * 1e3) for f, _ in forms for name, _, _, _ in ctxs), flush=True)
        assert digests == {want}, (digests, want)
        for f, _ in forms:
            mine = times[(f, "this build")]
            line = "%s: %s: this build %.2f .. %.2f ms (%.0f MB/s best, %d waits, %d documents on the host path)" % (
                tag, f, min(mine) * 1e3, max(mine) * 1e3, total / min(mine) / 1e6, waits[(f, "this build")], fbs[(f, "this build")])
            if not args.only_batch:
                theirs = times[(f, "parent build")]
                line += ", parent build %.2f .. %.2f ms (%.0f MB/s best, %d waits, %d documents on the host path); parent's fastest / this build's slowest = %.1fx" % (
                    min(theirs) * 1e3, max(theirs) * 1e3, total / min(theirs) / 1e6, waits[(f, "parent build")], fbs[(f, "parent build")], min(theirs) / max(mine))
                if max(mine) >= min(theirs):
                    line += "\n%s: %s: CONDITION NOT MET - this build's slowest round is not faster than the parent's fastest" % (tag, f)
                    gate_ok = False
            print(line, flush=True)
        print("%s: %d -> %d bytes; digest of all documents %s, equal for both builds, both forms and the inputs" % (tag, int(off[-1]), total, want), flush=True)
        del d_in, d_out
for name, L, h, ex in ctxs:
    L.cjs_destroy(h)
maker.close()
sys.exit(0 if gate_ok else 1)
