"""Throughput probe of the batched block fetch (not a test): the bench's enwik stream (tests/workloads.py, 10^8 bytes) compressed
at level 9 and at level 1, all table positions shuffled, fetched by ONE cjs_bz2_decompress_blocks_device call (device-resident) and
ONE cjs_bz2_decompress_blocks call (host to host) of this build, against a loop of single cjs_bz2_decompress_block calls on a
library built from the parent commit (--parent-lib; without it the loop runs on this build) - three alternating rounds in one
process.  The digest over all decoded blocks must be equal for the three and equal to that of the input's slices in request order.
Writes the report to --out (profiles/block_batch_probe.txt).  Exit status 1 when the batch's slowest round is not faster than the
loop's fastest round by more than the spread of the rounds.
    python tests/gpu_block_batch_probe.py [--parent-lib PATH] [--size 100000000] [--rounds 3] [--levels 9,1] [--out PATH]"""
import argparse
import ctypes as C
import hashlib
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import numpy as np
import torch
import workloads
from compressjs_amd.bzip2 import Context

ap = argparse.ArgumentParser()
ap.add_argument("--parent-lib", default=None)
ap.add_argument("--size", type=int, default=100_000_000)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--levels", default="9,1")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "block_batch_probe.txt"))
args = ap.parse_args()

lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


ctx = Context(0, 128)
L = ctx.L
if args.parent_lib:
    PL = C.CDLL(args.parent_lib)                     # (plain: the parent's library lacks the symbols _lib.load binds)
    PL.cjs_create.restype = C.c_void_p
    PL.cjs_create.argtypes = [C.c_int, C.c_uint32]
    PL.cjs_destroy.restype = None
    PL.cjs_destroy.argtypes = [C.c_void_p]
    PL.cjs_bz2_decompress_block.restype = C.c_int64
    PL.cjs_bz2_decompress_block.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p, C.c_uint64]
    loop_lib, loop_h, loop_name = PL, PL.cjs_create(0, 128), "parent build"
    assert loop_h
else:
    loop_lib, loop_h, loop_name = L, ctx.h, "this build"


def loop_single(z, pos, cap, digest):
    """-> seconds for one cjs_bz2_decompress_block call per position"""
    out = np.zeros(cap, np.uint8)
    t = 0.0
    for p in pos:
        a = time.perf_counter()
        n = int(loop_lib.cjs_bz2_decompress_block(loop_h, z.ctypes.data, z.size, int(p), out.ctypes.data, cap))
        t += time.perf_counter() - a
        assert n > 0, (p, n)
        if digest is not None:
            digest.update(out[:n].tobytes())
    return t


gate_ok = True
data = np.ascontiguousarray(workloads.stream("enwik", args.size))
say("block fetch probe: enwik stream of %d bytes, %d alternating rounds, loop of single calls on the %s" % (data.size, args.rounds, loop_name))
for level in (int(x) for x in args.levels.split(",")):
    z = np.frombuffer(ctx.compress(data, level), dtype=np.uint8).copy()
    tab = ctx.table(z)
    nb = len(tab)
    cut = np.concatenate([[0], np.cumsum([s for _p, s in tab])])
    assert int(cut[-1]) == data.size
    order = np.random.RandomState(5).permutation(nb)
    pos = np.array([tab[k][0] for k in order], np.uint64)
    hd = hashlib.sha256()
    for k in order:
        hd.update(data[int(cut[k]):int(cut[k + 1])].tobytes())
    want = hd.hexdigest()[:16]
    total = data.size
    cap = max(s for _p, s in tab) + 64
    tag = "level %d, %d blocks, %d -> %d bytes" % (level, nb, z.size, total)

    d_in = torch.from_numpy(z).cuda()
    d_pos = torch.from_numpy(pos.view(np.int64)).cuda()
    d_out = torch.empty(total + 64, dtype=torch.uint8, device="cuda")
    d_oo = torch.empty(nb + 1, dtype=torch.int64, device="cuda")
    d_st = torch.empty(nb, dtype=torch.int32, device="cuda")
    out = np.zeros(total + 64, np.uint8)
    out_off = np.zeros(nb + 1, np.uint64)
    status = np.zeros(nb, np.int32)

    def batch_device():
        torch.cuda.synchronize()
        a = time.perf_counter()
        n = ctx.decompress_blocks_device(d_in, d_pos, d_out, d_oo, d_st)
        w = time.perf_counter() - a
        assert n == total and not d_st.any().item(), n
        return w, L.cjs_dbg_dec_syncs(), ctx.last_decode_ms

    def batch_host():
        a = time.perf_counter()
        n = int(L.cjs_bz2_decompress_blocks(ctx.h, z.ctypes.data, z.size, pos.ctypes.data, nb, out.ctypes.data, total + 64,
                                            out_off.ctypes.data, status.ctypes.data, None))
        w = time.perf_counter() - a
        assert n == total and not status.any(), n
        return w, L.cjs_dbg_dec_syncs()

    batch_device()                                      # warm-up: the first call grows the workspaces
    batch_host()
    loop_single(z, pos[:min(nb, 8)], cap, None)
    t_dev, t_host, t_loop = [], [], []
    for r in range(args.rounds):
        w, syncs_dev, dev_ms = batch_device()
        t_dev.append(w)
        w, syncs_host = batch_host()
        t_host.append(w)
        hl = hashlib.sha256() if r == 0 else None
        t_loop.append(loop_single(z, pos, cap, hl))
        if hl:
            dgl = hl.hexdigest()[:16]
        say("%s, round %d: batch device-resident %.2f ms (%.2f ms between the call's events), batch host to host %.2f ms, loop of %d single calls %.1f ms"
            % (tag, r, t_dev[-1] * 1e3, dev_ms, t_host[-1] * 1e3, nb, t_loop[-1] * 1e3))
    dg = hashlib.sha256(d_out[:total].cpu().numpy().tobytes()).hexdigest()[:16]
    dgh = hashlib.sha256(out[:total].tobytes()).hexdigest()[:16]
    assert dg == dgh == dgl == want, (dg, dgh, dgl, want)
    for name, t, syncs in (("batch device-resident", t_dev, syncs_dev), ("batch host to host", t_host, syncs_host), ("loop of single calls (%s)" % loop_name, t_loop, None)):
        say("%s: %s: median %.2f ms, min %.2f, max %.2f (spread %.1f %% of the median), %.0f MB/s of decoded bytes at the median%s"
            % (tag, name, np.median(t) * 1e3, min(t) * 1e3, max(t) * 1e3, (max(t) - min(t)) / np.median(t) * 100, total / np.median(t) / 1e6,
               ", %d host<->device waits per call" % syncs if syncs is not None else ""))
    spread = max((max(t) - min(t)) / np.median(t) for t in (t_dev, t_host, t_loop))
    for name, t in (("device-resident", t_dev), ("host to host", t_host)):
        ratio = min(t_loop) / max(t)
        ok = ratio > 1.0 + spread
        gate_ok = gate_ok and ok
        say("%s: %s: loop's fastest round / batch's slowest round = %.2fx, largest spread of the rounds %.1f %%: %s"
            % (tag, name, ratio, spread * 100, "faster by more than the spread" if ok else "GATE VIOLATED - not faster by more than the spread"))
    say("%s: digest of all decoded blocks %s = digest of the input's slices in request order, for the two batch forms and the loop" % (tag, dg))
    say("%s: the probe kernels' own time: not measured" % tag)
    del d_in, d_out
if args.parent_lib:
    loop_lib.cjs_destroy(loop_h)
ctx.close()
os.makedirs(os.path.dirname(args.out), exist_ok=True)
with open(args.out, "w") as f:
    f.write("\n".join(lines) + "\n")
sys.exit(0 if gate_ok else 1)
