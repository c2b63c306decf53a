"""Cases of the batched block fetch, cjs_bz2_decompress_blocks (tests/test_emu_block_batch.py on the CPU logic build,
tests/test_gpu_block_batch.py on the GPU): N chosen blocks of one stream in one call.  Every request must come out as
Bzip2.decompressBlock gives it for that position alone; the arbiter is oracle.bz2_decompress_block, pinned to the reference by the
suite, and for the catalogue of decode_cases the reference-made record in tests/golden/golden_decode.json.

A form of the call is a `Mem`: where the caller's arrays live.  HostMem is the host form; the GPU test passes a Mem of torch
tensors for the device form (on the CPU logic build the device form takes host pointers)."""
import hashlib

import numpy as np

import batch_decode_cases as bdc
import decode_chain_cases as dcc
import oracle

WHOLEPI = 0x314159265359


class HostMem:
    device = False

    def up(self, a):
        """-> (pointer, owner)"""
        return a.ctypes.data, a

    def down(self, owner):
        return owner


class HostAsDevice(HostMem):
    """the device entry on host pointers: the CPU logic build only"""
    device = True


class Result:
    def __init__(self, ret, out_off, status, detail, out, syncs):
        self.ret, self.out_off, self.status, self.detail, self.out, self.syncs = ret, out_off, status, detail, out, syncs

    def doc(self, k):
        return self.out[int(self.out_off[k]):int(self.out_off[k + 1])].tobytes()


def run_blocks(L, h, stream, positions, mem=None, cap=0, with_detail=True, tail=0):
    """One call with an output buffer of cap + tail bytes, of which the call is told cap; every array is pre-filled with stale
    values.  -> Result (out: the whole buffer, the tail included)"""
    mem = mem or HostMem()
    n = len(positions)
    s = np.frombuffer(bytes(stream), dtype=np.uint8).copy() if len(stream) else np.zeros(1, np.uint8)
    p_in, _k0 = mem.up(s)
    p_pos, _k1 = mem.up(np.array([int(p) for p in positions], dtype=np.uint64))
    p_oo, k_oo = mem.up(np.full(n + 1, 0xEEEE, np.uint64))
    p_st, k_st = mem.up(np.full(n, 77, np.int32))
    p_det, k_det = mem.up(np.full(3 * n, 0xDDDD, np.uint32)) if with_detail else (None, None)
    p_out, k_out = mem.up(np.full(max(cap + tail, 1), 0xAA, np.uint8))
    fn = L.cjs_bz2_decompress_blocks_device if mem.device else L.cjs_bz2_decompress_blocks
    ret = int(fn(h, p_in if len(stream) else None, len(stream), p_pos, n, p_out, cap, p_oo, p_st, p_det))
    syncs = L.cjs_dbg_dec_syncs()
    return Result(ret, mem.down(k_oo), mem.down(k_st), mem.down(k_det) if with_detail else None, mem.down(k_out), syncs)


_oracle = {}


def want_of(key, stream, pos):
    """oracle.bz2_decompress_block(stream, pos), computed once per (key, pos): key names the stream"""
    if (key, pos) not in _oracle:
        _oracle[(key, pos)] = oracle.bz2_decompress_block(stream, pos, 1 << 20)
    return _oracle[(key, pos)]


def check_vs_oracle(L, h, mem, key, stream, positions, crc_pairs=None):
    """One call on `positions`: status, detail triple, bytes and out_off of every request are the oracle's for that position
    alone (crc_pairs: {position: (got, expected)} of the blocks whose CRC is bad), nothing is written behind the last byte.
    -> Result"""
    want = [want_of(key, stream, p) for p in positions]
    total = sum(w[0] for w in want if w[0] > 0)
    r = run_blocks(L, h, stream, positions, mem, cap=total, tail=64)
    assert r.ret == total, (key, r.ret, total)
    off = 0
    for k, (p, w) in enumerate(zip(positions, want)):
        assert int(r.out_off[k]) == off, (key, k, p, int(r.out_off[k]), off)
        trip = tuple(int(x) for x in r.detail[3 * k:3 * k + 3])
        if w[0] < 0:
            assert int(r.status[k]) == w[0] and trip[0] == w[1], (key, k, p, int(r.status[k]), trip, w[:2])
            assert trip[1:] == (crc_pairs[p] if w[1] == 4 else (0, 0)), (key, k, p, [hex(x) for x in trip[1:]])
        else:
            assert int(r.status[k]) == 0 and trip == (0, 0, 0), (key, k, p, int(r.status[k]), trip)
            assert r.out[off:off + w[0]].tobytes() == w[2], (key, k, p)
            off += w[0]
    assert int(r.out_off[len(positions)]) == off == total
    assert bytes(r.out[total:]) == b"\xaa" * 64, key                      # the canary
    return r


# ---- case 1: the reference-made outcomes ------------------------------------------------------------------------------------------

def check_golden(L, h, mem, max_len=None):
    """BLOCK_CASES of decode_cases against golden_decode.json: one call per stream with all its positions."""
    import decode_cases
    g = bdc.golden_decode()
    by = {sid: s for sid, s, _ms in decode_cases.streams()}
    groups = {}
    for sid, pos in decode_cases.BLOCK_CASES:
        groups.setdefault(sid, []).append(pos)
    ran = 0
    for sid, positions in groups.items():
        s = by.get(sid)
        if s is None or (max_len is not None and len(s) > max_len):
            continue
        r = run_blocks(L, h, s, positions, mem)
        if r.ret == -21:
            r = run_blocks(L, h, s, positions, mem, cap=int(r.out_off[-1]))
        assert r.ret >= 0 and int(r.out_off[0]) == 0 and int(r.out_off[-1]) == r.ret, (sid, r.ret)
        for k, pos in enumerate(positions):
            v = g["block:%s@%d" % (sid, pos)]
            st, doc = int(r.status[k]), r.doc(k)
            if v["ok"]:
                assert st == 0 and len(doc) == v["out_len"] and hashlib.sha256(doc).hexdigest() == v["out_sha256"], (sid, pos, st, len(doc))
            else:
                assert st == v["error_code"] and doc == b"", (sid, pos, st, v)
                exp = bdc.DETAIL.get(int(r.detail[3 * k]))
                assert v["message"].endswith(": " + exp) if exp else ": " not in v["message"], (sid, pos, v["message"])
        ran += len(positions)
    return ran


# ---- case 2: order, kinds, slot batches -------------------------------------------------------------------------------------------

def mixed_positions():
    """The 40 blocks of the 40-stream file, its 40 end-of-stream magics, every one of them + 1, ten duplicates and five positions
    at and behind the file's end, shuffled: 50 block requests - four slot batches of 16 - with failures mixed in."""
    f = dcc.the_file()
    blocks = [p for p, _z in f.tab]
    ends = [dcc.end_magic(f, k) for k in range(dcc.NSTREAM)]
    n = len(f.data)
    pos = blocks + ends + [p + 1 for p in blocks + ends] + blocks[3:33:3] + [8 * n - 47, 8 * n - 1, 8 * n, 2 ** 63, 2 ** 64 - 1]
    assert len(pos) == 175
    rng = np.random.RandomState(20240)
    return [pos[i] for i in rng.permutation(len(pos))]


def check_mixed(L, h, mem):
    f = dcc.the_file()
    pos = mixed_positions()
    r = check_vs_oracle(L, h, mem, "file", f.data, pos)
    assert sum(1 for k in range(len(pos)) if int(r.out_off[k + 1]) > int(r.out_off[k])) == 50
    return r


def check_mixed_vs_single_calls(L, h, mem):
    """the same positions through a loop of cjs_bz2_decompress_block"""
    f = dcc.the_file()
    pos = mixed_positions()
    r = check_mixed(L, h, mem)
    d = np.frombuffer(f.data, dtype=np.uint8)
    for k, p in enumerate(pos):
        n = L.cjs_bz2_decompress_block(h, d.ctypes.data, d.size, p, None, 0)
        det = L.cjs_bz2_last_detail(h, None, None)
        if n == -21:
            n = int(L.cjs_bz2_last_size(h))
            one = np.full(n, 0xAA, np.uint8)
            assert L.cjs_bz2_fetch(h, one.ctypes.data, n) == n
            assert int(r.status[k]) == 0 and r.doc(k) == one.tobytes(), (k, p)
        else:
            assert (int(r.status[k]), int(r.detail[3 * k])) == (n, det) and r.doc(k) == b"", (k, p, n, det)


# ---- case 3: waits ----------------------------------------------------------------------------------------------------------------

def check_waits(L, h, mem):
    """cjs_dbg_dec_syncs() of a call does not depend on the number of requests inside a slot batch of 16, and every further slot
    batch adds the same number."""
    f = dcc.the_file()
    syncs = {}
    for n in (1, 16, 17, 32, 33):
        positions = [p for p, _z in f.tab[:n]]
        r = run_blocks(L, h, f.data, positions, mem)
        assert r.ret == -21 and int(r.out_off[-1]) == sum(z for _p, z in f.tab[:n]), (n, r.ret)
        syncs[n] = r.syncs
    print("syncs of a block-list call, device form %d: %s" % (mem.device, syncs))
    assert syncs[1] == syncs[16] and syncs[17] == syncs[32], syncs
    assert syncs[17] - syncs[16] == syncs[33] - syncs[32] > 0, syncs
    return syncs


# ---- case 4: broken blocks --------------------------------------------------------------------------------------------------------

def check_broken(L, h, mem, name):
    f = dcc.the_file()
    tab = [p for p, _z in f.tab]
    if name in ("blockcrc16", "trunc33"):
        s, blk, pair = dcc.broken_files()[name]
        if name == "blockcrc16":
            r = check_vs_oracle(L, h, mem, name, s, [tab[17], tab[16], tab[15]], {tab[16]: pair})
            assert [int(x) for x in r.status] == [0, -5, 0] and int(r.detail[3]) == 4
            assert r.doc(0) == want_of("file", f.data, tab[17])[2] and r.doc(2) == want_of("file", f.data, tab[15])[2]
        else:
            r = check_vs_oracle(L, h, mem, name, s, [tab[33], tab[32]])
            assert int(r.status[0]) < 0 and int(r.status[1]) == 0 and r.doc(1) == want_of("file", f.data, tab[32])[2]
    elif name == "origptr5":
        s = bdc.flip(f.data, tab[5] + 48 + 32 + 1)                      # magic, CRC, the randomised bit, then 24 bits of origPtr
        r = check_vs_oracle(L, h, mem, name, s, [tab[4], tab[5], tab[6]])
        assert (int(r.status[1]), int(r.detail[3])) == (-5, 3)
    elif name == "fakemagic":
        s = f.data + WHOLEPI.to_bytes(6, "big") + np.random.RandomState(77).randint(0, 256, 200).astype(np.uint8).tobytes()
        r = check_vs_oracle(L, h, mem, name, s, [tab[39], 8 * len(f.data), tab[0]])
        assert int(r.status[1]) < 0
    elif name == "level":
        s = bdc.flip(f.data, 3 * 8 + 1)                                  # '1'..'9' ^ 0x40: no level
        pos = [tab[0], dcc.end_magic(f, 0), tab[0] + 1, 2 ** 64 - 1]
        r = run_blocks(L, h, s, pos, mem, cap=64)
        assert r.ret == 0 and [int(x) for x in r.out_off] == [0] * 5
        assert [int(x) for x in r.status] == [-2] * 4 and [int(x) for x in r.detail] == [2, 0, 0] * 4
        assert all(want_of(name, s, p)[:2] == (-2, 2) for p in pos)
    elif name == "short":
        for n in (0, 3):
            r = run_blocks(L, h, f.data[:n], [32, 0, 2 ** 63], mem, cap=64)
            assert r.ret == 0 and [int(x) for x in r.out_off] == [0] * 4, (n, r.ret)
            assert [int(x) for x in r.status] == [-2] * 3 and [int(x) for x in r.detail] == [1, 0, 0] * 3, n
            assert want_of("short%d" % n, f.data[:n], 32)[:2] == (-2, 1)
    else:
        raise KeyError(name)


BROKEN = ["blockcrc16", "trunc33", "origptr5", "fakemagic", "level", "short"]


# ---- case 6: call level -----------------------------------------------------------------------------------------------------------

def check_call_level(L, h):
    f = dcc.the_file()
    d = np.frombuffer(f.data, dtype=np.uint8)
    pos = np.array([f.tab[7][0], f.tab[2][0]], np.uint64)
    want = want_of("file", f.data, f.tab[7][0])[2] + want_of("file", f.data, f.tab[2][0])[2]
    oo, st, det = np.zeros(3, np.uint64), np.zeros(2, np.int32), np.zeros(6, np.uint32)
    out = np.full(len(want) + 8, 0xAA, np.uint8)
    args = lambda: [h, d.ctypes.data, d.size, pos.ctypes.data, 2, out.ctypes.data, out.size, oo.ctypes.data, st.ctypes.data, det.ctypes.data]  # noqa: E731
    for fn in (L.cjs_bz2_decompress_blocks, L.cjs_bz2_decompress_blocks_device):
        a = args()
        a[4] = 0
        assert fn(*a) == 0                                               # count == 0
        assert fn(h, None, 0, None, 0, None, 0, None, None, None) == 0
        for k in (0, 1, 3, 7, 8):                                        # ctx, in (with in_len > 0), bitpos, out_off, status
            a = args()
            a[k] = None
            assert fn(*a) == -22, k
    a = args()
    a[6] = len(want) - 1                                                 # one byte short
    assert L.cjs_bz2_decompress_blocks(*a) == -21 and bytes(out) == b"\xaa" * out.size
    assert [int(x) for x in oo] == [0, f.tab[7][1], len(want)] and [int(x) for x in st] == [0, 0]
    assert L.cjs_bz2_last_size(h) == len(want)
    assert L.cjs_bz2_fetch(h, out.ctypes.data, out.size) == len(want) and out[:len(want)].tobytes() == want
    a = args()
    a[9] = None                                                          # detail == NULL
    off_by_one = np.array([f.tab[7][0] + 1, f.tab[2][0]], np.uint64)
    a[3] = off_by_one.ctypes.data
    out[:] = 0xAA
    n = L.cjs_bz2_decompress_blocks(*a)
    assert n == f.tab[2][1] and [int(x) for x in st] == [-2, 0] and [int(x) for x in oo] == [0, 0, n]
    assert out[:n].tobytes() == want[f.tab[7][1]:]
    assert L.cjs_bz2_last_detail(h, None, None) == 0


# ---- case 8: neighbours undisturbed -----------------------------------------------------------------------------------------------

def neighbour_calls(L, h, which):
    """One call of kind `which` -> what it gave, in a comparable form"""
    f = dcc.the_file()
    if which == "blocks":
        r = run_blocks(L, h, f.data, [f.tab[20][0], f.tab[1][0] + 1, f.tab[1][0], dcc.end_magic(f, 3)], cap=4096)
        return r.ret, [int(x) for x in r.out_off], [int(x) for x in r.status], [int(x) for x in r.detail], r.out[:max(r.ret, 0)].tobytes()
    if which == "many":
        docs = [f.streams[0], f.streams[1][:-9], f.streams[2]]          # (one document truncated)
        r = bdc.run_batch(L, h, docs, False)
        return r.ret, [int(x) for x in r.out_off], [int(x) for x in r.status], [int(x) for x in r.detail], r.docs
    if which == "single":
        return dcc.run_single(L, h, b"".join(f.streams[:4]), True)
    if which == "block":
        d = np.frombuffer(f.data, dtype=np.uint8)
        n = L.cjs_bz2_decompress_block(h, d.ctypes.data, d.size, f.tab[9][0], None, 0)
        size = int(L.cjs_bz2_last_size(h))
        out = np.zeros(size, np.uint8)
        assert n == -21 and L.cjs_bz2_fetch(h, out.ctypes.data, size) == size
        return size, out.tobytes()
    raise KeyError(which)


def check_neighbours(L, h, fresh):
    """fresh(): a context manager giving the handle of a new context.  The four entries alternate on one context; each gives what
    it gives on a context of its own."""
    alone = {}
    for which in ("blocks", "many", "single", "block"):
        with fresh() as h2:
            alone[which] = neighbour_calls(L, h2, which)
    f = dcc.the_file()
    assert alone["block"] == (f.tab[9][1], want_of("file", f.data, f.tab[9][0])[2])
    assert alone["many"][2][1] < 0 and alone["blocks"][2] == [0, -2, 0, 0]
    for which in ("blocks", "many", "blocks", "single", "blocks", "block", "blocks"):
        assert neighbour_calls(L, h, which) == alone[which], which


def ctx_factory(L, batch_blocks):
    import contextlib

    @contextlib.contextmanager
    def fresh():
        h = L.cjs_create(0, batch_blocks)
        assert h
        try:
            yield h
        finally:
            L.cjs_destroy(h)
    return fresh


def sha(b):
    return hashlib.sha256(b).hexdigest()

