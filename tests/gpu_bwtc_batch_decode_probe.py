"""Throughput probe of the batched BWTC decode (not a test): the level-9 streams of N independent documents of synth.enwik_like,
made once by bwtc_compress_many, through cjs_bwtc_decompress_batch_device (device-resident) and cjs_bwtc_decompress_batch (host to
host), against the loop of single cjs_bwtc_decompress calls over the same streams on a library built from the parent commit
(--parent-lib; without it, on this build).  Every shape is warmed up first; then batch and loop alternate for --rounds rounds in
the same process on the same GPU (the loop over the first --loop-calls streams, scaled to the whole batch), and one full loop
gives the digest over all decoded documents, which must equal the batch's and the inputs'.  The condition: the batch is faster
than the loop at every shape by more than the spread of the rounds.  --only-batch runs the device-resident batch alone (for a
kernel trace).
    python tests/gpu_bwtc_batch_decode_probe.py [--parent-lib PATH] [--rounds 3] [--shapes 1000x100000,10000x10000] [--loop-calls 300]"""
import argparse
import ctypes as C
import hashlib
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
from compressjs_amd import synth
from compressjs_amd.bzip2 import Context

ap = argparse.ArgumentParser()
ap.add_argument("--parent-lib", default=None)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--shapes", default="1000x100000,10000x10000")
ap.add_argument("--level", type=int, default=9)
ap.add_argument("--loop-calls", type=int, default=300)
ap.add_argument("--blocks", type=int, default=128)
ap.add_argument("--only-batch", action="store_true")
args = ap.parse_args()


def loop_single(L, h, flat, off, count, room, digest=False):
    """-> (seconds, digest of all decoded documents in order)"""
    out = np.zeros(room, np.uint8)
    dg = hashlib.sha256()
    base = flat.ctypes.data
    t = 0.0
    for k in range(count):
        ln = int(off[k + 1] - off[k])
        a = time.perf_counter()
        n = int(L.cjs_bwtc_decompress(h, base + int(off[k]), ln, out.ctypes.data, room, None))
        t += time.perf_counter() - a
        assert n > 0, n
        if digest:
            dg.update(out[:n].tobytes())
    return t, dg.hexdigest()[:16]


ctx = Context(0, args.blocks)
L = ctx.L
if args.parent_lib:
    PL = C.CDLL(args.parent_lib)                     # (plain: the parent's library has no batched decode)
    PL.cjs_create.restype = C.c_void_p
    PL.cjs_create.argtypes = [C.c_int, C.c_uint32]
    PL.cjs_destroy.restype = None
    PL.cjs_destroy.argtypes = [C.c_void_p]
    PL.cjs_bwtc_decompress.restype = C.c_int64
    PL.cjs_bwtc_decompress.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.POINTER(C.c_int64)]
    ref, ref_name = (PL, PL.cjs_create(0, args.blocks)), "parent build"
    assert ref[1]
else:
    ref, ref_name = (L, ctx.h), "this build"
gate_ok = True
for shape in args.shapes.split(","):
    count, size = (int(x) for x in shape.split("x"))
    data = np.ascontiguousarray(synth.enwik_like(count * size, 77))
    total = count * size
    want = hashlib.sha256(data.tobytes()).hexdigest()[:16]
    streams = ctx.bwtc_compress_many([data[k * size:(k + 1) * size] for k in range(count)], args.level)
    off = np.zeros(count + 1, np.uint64)
    off[1:] = np.cumsum([len(s) for s in streams], dtype=np.uint64)
    flat = np.frombuffer(b"".join(streams), dtype=np.uint8).copy()
    del streams
    tag = "%d x %d B, level %d" % (count, size, args.level)
    d_in = torch.from_numpy(flat).cuda()
    d_off = torch.from_numpy(off.astype(np.int64)).cuda()
    d_out = torch.empty(total, dtype=torch.uint8, device="cuda")
    d_oo = torch.empty(count + 1, dtype=torch.int64, device="cuda")
    d_st = torch.empty(count, dtype=torch.int32, device="cuda")
    out = np.zeros(total, np.uint8)
    out_off = np.zeros(count + 1, np.uint64)
    status = np.zeros(count, np.int32)
    sub = min(count, args.loop_calls)

    def batch_device():
        torch.cuda.synchronize()
        a = time.perf_counter()
        n = ctx.bwtc_decompress_many_device(d_in, d_off, d_out, d_oo, d_st)
        return time.perf_counter() - a, n

    def batch_host():
        a = time.perf_counter()
        m = int(L.cjs_bwtc_decompress_batch(ctx.h, flat.ctypes.data, off.ctypes.data, count, out.ctypes.data, total, out_off.ctypes.data,
                                            status.ctypes.data, None))
        return time.perf_counter() - a, m

    # warm-up of every path at this shape (buffers grow, code objects load)
    _, n = batch_device()
    assert n == total, n
    if args.only_batch:
        w, n = batch_device()
        print("%s: batch device-resident %.2f ms wall (%d syncs, %d on the host path), %d -> %d bytes"
              % (tag, w * 1e3, int(L.cjs_dbg_bwtc_dec_batch_syncs(ctx.h)), int(L.cjs_dbg_bwtc_dec_batch_fallbacks(ctx.h)), flat.size, n), flush=True)
        continue
    _, m = batch_host()
    assert m == total, m
    loop_single(ref[0], ref[1], flat, off, min(count, 30), size)
    wd, wh, wl = [], [], []
    for r in range(args.rounds):
        w, n = batch_device()
        wd.append(w)
        syncs, fb = int(L.cjs_dbg_bwtc_dec_batch_syncs(ctx.h)), int(L.cjs_dbg_bwtc_dec_batch_fallbacks(ctx.h))
        w, m = batch_host()
        wh.append(w)
        assert m == n == total
        t, _ = loop_single(ref[0], ref[1], flat, off, sub, size)
        wl.append(t / sub * count)
        print("%s: round %d: batch device-resident %.2f ms wall, host to host %.2f ms, loop of single calls (%s, %d calls scaled to %d) %.1f ms = %.3f ms per call"
              % (tag, r + 1, wd[-1] * 1e3, wh[-1] * 1e3, ref_name, sub, count, wl[-1] * 1e3, t * 1e3 / sub), flush=True)
    assert int(d_st.abs().sum().item()) == 0 and not status.any()
    dg = hashlib.sha256(d_out.cpu().numpy().tobytes()).hexdigest()[:16]
    dgh = hashlib.sha256(out.tobytes()).hexdigest()[:16]
    tfull, dgl = loop_single(ref[0], ref[1], flat, off, count, size, digest=True)
    print("%s: full loop of single calls (%s) %.1f ms (%.3f ms per call), %.1f MB/s; digests inputs %s, batch device %s, batch host %s, loop %s"
          % (tag, ref_name, tfull * 1e3, tfull * 1e3 / count, total / tfull / 1e6, want, dg, dgh, dgl), flush=True)
    assert want == dg == dgh == dgl, (want, dg, dgh, dgl)
    print("%s: batch device-resident %.2f .. %.2f ms (%.0f MB/s best), host to host %.2f .. %.2f ms (%.0f MB/s best), loop %.1f .. %.1f ms; %d syncs per device call, %d documents on the host path; %d -> %d bytes"
          % (tag, min(wd) * 1e3, max(wd) * 1e3, total / min(wd) / 1e6, min(wh) * 1e3, max(wh) * 1e3, total / min(wh) / 1e6, min(wl) * 1e3, max(wl) * 1e3,
             syncs, fb, flat.size, total), flush=True)
    print("%s: speed-up over the loop, slowest batch round against fastest loop round: %.1fx device-resident, %.1fx host to host; digests equal"
          % (tag, min(wl) / max(wd), min(wl) / max(wh)), flush=True)
    if max(wd) >= min(wl) or max(wh) >= min(wl):
        print("%s: CONDITION NOT MET - a batch round is not faster than every loop round" % tag, flush=True)
        gate_ok = False
    del d_in, d_out
if args.parent_lib:
    ref[0].cjs_destroy(ref[1])
ctx.close()
sys.exit(0 if gate_ok else 1)
