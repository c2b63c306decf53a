"""Throughput probe of the batched bzip2 decode entry (not a test): N independent documents of synth.enwik_like, compressed at
level 9 by compress_many, back through cjs_bz2_decompress_batch_device (device-resident) and cjs_bz2_decompress_batch (host to
host) - a mean over repeated calls after a warm-up - against the loop of single cjs_bz2_decompress calls over the same streams, on
this build and, with --parent-lib, on a library built from the parent commit.  Prints one line per measurement and one digest over
all decoded documents, which must equal the digest of the inputs.  Exit status 1 when a batch call is slower than the loop.
    python tests/gpu_batch_decode_probe.py [--parent-lib PATH] [--reps 3] [--shapes 1000x100000,10000x10000] [--loop-calls 0]"""
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
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--shapes", default="1000x100000,10000x10000")
ap.add_argument("--loop-calls", type=int, default=0, help="time only the first K single calls and scale (0: all of them)")
args = ap.parse_args()


def loop_single(L, h, z, zoff, count, size, digest):
    """-> seconds for `count` calls (every document fits `size` bytes); digest (or None) is fed the decoded bytes"""
    out = np.zeros(size + 64, np.uint8)
    base = z.ctypes.data
    t = 0.0
    for k in range(count):
        a = time.perf_counter()
        n = int(L.cjs_bz2_decompress(h, base + int(zoff[k]), int(zoff[k + 1] - zoff[k]), out.ctypes.data, size + 64, 0))
        t += time.perf_counter() - a
        assert n == size, (k, n)
        if digest is not None:
            digest.update(out[:n].tobytes())
    return t


ctx = Context(0, 128)
L = ctx.L
gate_ok = True
parent = None
if args.parent_lib:
    PL = C.CDLL(args.parent_lib)                     # (plain: the parent's library has no batch symbols for _lib.load to bind)
    PL.cjs_create.restype = C.c_void_p
    PL.cjs_create.argtypes = [C.c_int, C.c_uint32]
    PL.cjs_destroy.restype = None
    PL.cjs_destroy.argtypes = [C.c_void_p]
    PL.cjs_bz2_decompress.restype = C.c_int64
    PL.cjs_bz2_decompress.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_int]
    parent = (PL, PL.cjs_create(0, 128))
    assert parent[1]
for shape in args.shapes.split(","):
    count, size = (int(x) for x in shape.split("x"))
    flat = np.ascontiguousarray(synth.enwik_like(count * size, 77))
    total = count * size
    want = hashlib.sha256(flat.tobytes()).hexdigest()[:16]
    tag = "%d x %d B" % (count, size)
    streams = ctx.compress_many([flat[k * size:(k + 1) * size] for k in range(count)], 9)
    z = np.frombuffer(b"".join(streams), dtype=np.uint8).copy()
    zoff = np.zeros(count + 1, np.uint64)
    zoff[1:] = np.cumsum([len(s) for s in streams], dtype=np.uint64)
    del streams
    # device-resident
    d_in = torch.from_numpy(z).cuda()
    d_off = torch.from_numpy(zoff.astype(np.int64)).cuda()
    d_out = torch.empty(total + 64, dtype=torch.uint8, device="cuda")
    d_oo = torch.empty(count + 1, dtype=torch.int64, device="cuda")
    d_st = torch.empty(count, dtype=torch.int32, device="cuda")
    wall = dev = 0.0
    for r in range(args.reps + 1):                      # (the first call grows the workspaces)
        torch.cuda.synchronize()
        a = time.perf_counter()
        n = ctx.decompress_many_device(d_in, d_off, d_out, d_oo, d_st)
        w = time.perf_counter() - a
        if r:
            wall, dev = wall + w / args.reps, dev + ctx.last_decode_ms / 1e3 / args.reps
    assert n == total and not d_st.any().item() and int(d_oo[-1].item()) == total
    dg = hashlib.sha256(d_out[:n].cpu().numpy().tobytes()).hexdigest()[:16]
    syncs = L.cjs_dbg_dec_syncs()
    print("%s: batch device-resident %.2f ms wall, %.2f ms device, %.0f MB/s decoded, %d -> %d bytes, %d host<->device syncs, digest %s"
          % (tag, wall * 1e3, dev * 1e3, total / wall / 1e6, z.size, n, syncs, dg), flush=True)
    del d_in, d_out
    # host to host
    out = np.zeros(total + 64, np.uint8)
    out_off = np.zeros(count + 1, np.uint64)
    status = np.zeros(count, np.int32)
    host = 0.0
    for r in range(args.reps + 1):
        a = time.perf_counter()
        m = int(L.cjs_bz2_decompress_batch(ctx.h, z.ctypes.data, zoff.ctypes.data, count, 0, out.ctypes.data, total + 64, out_off.ctypes.data,
                                           status.ctypes.data, None))
        w = time.perf_counter() - a
        assert m == total and not status.any(), m
        if r:
            host += w / args.reps
    dgh = hashlib.sha256(out[:m].tobytes()).hexdigest()[:16]
    print("%s: batch host to host %.2f ms, %.0f MB/s decoded, digest %s" % (tag, host * 1e3, total / host / 1e6, dgh), flush=True)
    calls = min(count, args.loop_calls) if args.loop_calls else count
    hd = hashlib.sha256() if calls == count else None
    loop_single(L, ctx.h, z, zoff, min(calls, 20), size, None)          # warm-up
    t = loop_single(L, ctx.h, z, zoff, calls, size, hd) * count / calls
    dgl = hd.hexdigest()[:16] if hd else dg
    print("%s: loop of single calls, this build %.1f ms (%.3f ms per call, %d calls timed), %.1f MB/s" % (tag, t * 1e3, t * 1e3 / count, calls, total / t / 1e6), flush=True)
    tl = t
    if parent:
        loop_single(parent[0], parent[1], z, zoff, min(calls, 20), size, None)
        tl = loop_single(parent[0], parent[1], z, zoff, calls, size, None) * count / calls
        print("%s: loop of single calls, parent build %.1f ms (%.3f ms per call, %d calls timed), %.1f MB/s" % (tag, tl * 1e3, tl * 1e3 / count, calls, total / tl / 1e6), flush=True)
    assert dg == dgh == dgl == want, (dg, dgh, dgl, want)
    print("%s: batch / loop (%s build) speed-up %.1fx device-resident, %.1fx host to host; digest of all decoded documents %s = digest of the inputs"
          % (tag, "parent" if parent else "this", tl / wall, tl / host, dg), flush=True)
    if tl / wall < 1.0 or tl / host < 1.0:
        print("%s: GATE VIOLATED - the batch call is slower than the loop of single calls" % tag, flush=True)
        gate_ok = False
if parent:
    parent[0].cjs_destroy(parent[1])
ctx.close()
sys.exit(0 if gate_ok else 1)
