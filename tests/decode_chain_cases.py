"""Cases of the single-call decoder's chain walk across slot batches (tests/test_emu_decode_chain.py on the CPU logic build,
tests/test_gpu_decode_chain.py on the GPU): 40 one-block streams concatenated into one .bz2 file, decoded with multistream=1 on
16 slots (CJS_DEC_MAX_SLOTS=16 around the calls, in a fresh context: the variable is read per call and the slab never shrinks) -
three slot batches with a follow-on header read at every block.  The arbiter is oracle.bz2_decompress, pinned to the reference by
the suite; what the reference does not define - the partial size left after a failed call, the number of host<->device
synchronisations - is pinned to values recorded from the build in front of the one that merged the stream's and the batch's chain
walk."""
import contextlib
import ctypes as C
import os

import numpy as np

import batch_decode_cases as bdc
import oracle

NSTREAM = 40
SLOTS = 16

# cjs_bz2_last_size after the failed call, recorded from the parent build.  This is the parent's behaviour where the reference has
# written a block before it compares its CRC (lib/Bzip2.js:437-445): the failing block's bytes are counted, and an error of the
# walk leaves the bytes of every block in front of it.
PARENT_PARTIAL = {"blockcrc5": 1455, "blockcrc16": 6082, "blockcrc39": 15860, "streamcrc20": 7420, "level17": 6082, "trunc33": 12486}
# cjs_dbg_dec_syncs() after the clean 40-stream file, recorded from the parent on the CPU build (the fake runtime counts the same
# calls): scan, candidates, then 3 slot batches of one k7 and two K8/K9 waits; the device form adds one read per header and per
# stream CRC on the chain.
PARENT_SYNCS = {False: 11, True: 91}


@contextlib.contextmanager
def sixteen_slots():
    old = os.environ.get("CJS_DEC_MAX_SLOTS")
    os.environ["CJS_DEC_MAX_SLOTS"] = str(SLOTS)
    try:
        yield
    finally:
        if old is None:
            del os.environ["CJS_DEC_MAX_SLOTS"]
        else:
            os.environ["CJS_DEC_MAX_SLOTS"] = old


class File:
    """The clean file, the oracle's outcome on it and where its parts are."""
    def __init__(self):
        self.streams = [bdc.one_block(4000 + k, 150 + (k * 37) % 500, 1 + k % 9) for k in range(NSTREAM)]
        self.data = b"".join(self.streams)
        self.soff = np.concatenate([[0], np.cumsum([len(s) for s in self.streams])]).tolist()
        n, det, self.out, self.tab = oracle.bz2_decompress(self.data, True)
        assert n == len(self.out) and det == 0 and len(self.tab) == NSTREAM and len(self.data) < 100000
        self.first = oracle.bz2_decompress(self.streams[0], False)[2]
        assert oracle.bz2_decompress(self.data, False)[2] == self.first


_file = None


def the_file():
    global _file
    if _file is None:
        _file = File()
    return _file


def bits(s, bit, n=32):
    """the n bits at bit position `bit`"""
    return (int.from_bytes(s[bit >> 3:(bit >> 3) + 8], "big") >> (64 - n - (bit & 7))) & ((1 << n) - 1)


def end_magic(f, k):
    """bit position of the end-of-stream magic of stream k: 48 + 32 bits and at most 7 padding bits in front of the stream's end"""
    e = f.soff[k + 1] * 8
    at = [b for b in range(e - 87, e - 79) if bits(f.data, b, 48) == 0x177245385090]
    assert len(at) == 1
    return at[0]


def broken_files():
    """-> {name: (bytes, block whose CRC is bad or None, (got, expected) or None)}"""
    f = the_file()
    out = {}
    for k in (5, 16, 39):                  # inside the first slot batch, first of the second, the last
        at = f.tab[k][0] + 48
        s = bdc.flip(f.data, at + 7)
        out["blockcrc%d" % k] = (s, k, (bits(f.data, at), bits(s, at)))
    at = f.soff[21] * 8 - 9                # (at most 7 padding bits behind the stream CRC)
    s = bdc.flip(f.data, at)
    crc_at = end_magic(f, 20) + 48
    assert crc_at <= at < crc_at + 32
    out["streamcrc20"] = (s, None, (bits(f.data, crc_at), bits(s, crc_at)))
    out["level17"] = (bdc.flip(f.data, (f.soff[17] + 3) * 8 + 1), None, None)      # '1'..'9' ^ 0x40: no level
    out["trunc33"] = (f.data[:(f.tab[33][0] >> 3) + 40], None, None)
    return out


def host_ptr(a):
    return a.ctypes.data, a


def run_single(L, h, s, ms, to_dev=None):
    """One cjs_bz2_decompress (to_dev: cjs_bz2_decompress_device on to_dev(array) -> (pointer, owner)) with no room ->
    (ret or size, detail, got, expected, syncs of the call, bytes or None, cjs_bz2_last_size)"""
    d = np.frombuffer(s, dtype=np.uint8).copy()
    if to_dev:
        p, _keep = to_dev(d)
        n = L.cjs_bz2_decompress_device(h, p, d.size, None, 0, int(ms))
    else:
        n = L.cjs_bz2_decompress(h, d.ctypes.data, d.size, None, 0, int(ms))
    syncs = L.cjs_dbg_dec_syncs()
    got, want = C.c_uint32(0), C.c_uint32(0)
    det = L.cjs_bz2_last_detail(h, C.byref(got), C.byref(want))
    last = int(L.cjs_bz2_last_size(h))
    data = None
    if n == -21:
        n = last
        out = np.full(n, 0xAA, np.uint8)
        assert L.cjs_bz2_fetch(h, out.ctypes.data, n) == n
        data = out.tobytes()
    return int(n), int(det), got.value, want.value, syncs, data, last


def table(L, h, s, ms):
    d = np.frombuffer(s, dtype=np.uint8)
    cap = NSTREAM + 8
    pos, size = np.zeros(cap, np.uint64), np.zeros(cap, np.uint64)
    n = L.cjs_bz2_table(h, d.ctypes.data, d.size, int(ms), pos.ctypes.data, size.ctypes.data, cap)
    return [(int(pos[i]), int(size[i])) for i in range(n)] if n >= 0 else n


def check_clean(L, h, to_dev):
    """Case 1 and case 4: bytes, table, the first stream alone; the parent's sync count, the same on a second call."""
    f = the_file()
    for dev in (None, to_dev):
        for _rep in range(2):
            n, det, _g, _w, syncs, data, last = run_single(L, h, f.data, True, dev)
            assert (n, det, last) == (len(f.out), 0, len(f.out)) and data == f.out, (bool(dev), n, det)
            print("syncs of the clean file, device form %d: %d" % (bool(dev), syncs))
            assert syncs == PARENT_SYNCS[bool(dev)], (bool(dev), syncs)
        n, det, _g, _w, _s, data, _last = run_single(L, h, f.data, False, dev)
        assert (n, det) == (len(f.first), 0) and data == f.first, (bool(dev), n, det)
    assert table(L, h, f.data, True) == f.tab
    assert table(L, h, f.data, False) == f.tab[:1]


def check_broken(L, h, to_dev, name):
    """Cases 2 and 3: code, detail and CRC pair are the oracle's; the partial size is the parent's."""
    f = the_file()
    s, blk, pair = broken_files()[name]
    want = oracle.bz2_decompress(s, True)
    assert want[0] < 0
    for dev in (None, to_dev):
        n, det, g, w, _syncs, _data, last = run_single(L, h, s, True, dev)
        print("%s, device form %d: ret %d detail %d got %08x expected %08x last_size %d" % (name, bool(dev), n, det, g, w, last))
        assert (n, det) == want[:2], (name, bool(dev), n, det, want[:2])
        if pair:
            assert det == (4 if blk is not None else 5) and (g, w) == pair, (name, det, hex(g), hex(w), pair)
        if blk is not None:
            assert last == sum(z for _p, z in f.tab[:blk + 1]), (name, last)
        assert last == PARENT_PARTIAL[name], (name, bool(dev), last)
        got = np.full(last, 0xAA, np.uint8)
        assert L.cjs_bz2_fetch(h, got.ctypes.data, last) == last and got.tobytes() == f.out[:last], name


def check_block_entry(L, h):
    """Case 5: cjs_bz2_decompress_block at block 16, at an end-of-stream magic and one bit off."""
    f = the_file()
    d = np.frombuffer(f.data, dtype=np.uint8)
    pos = f.tab[16][0]
    end = end_magic(f, 16)
    for bit in (pos, end, pos + 1):
        want = oracle.bz2_decompress_block(f.data, bit)
        n = L.cjs_bz2_decompress_block(h, d.ctypes.data, d.size, bit, None, 0)
        det = L.cjs_bz2_last_detail(h, None, None)
        if n == -21:
            n = int(L.cjs_bz2_last_size(h))
            out = np.full(n, 0xAA, np.uint8)
            assert L.cjs_bz2_fetch(h, out.ctypes.data, n) == n
            assert want[0] == n and out.tobytes() == want[2], bit
        else:
            assert (n, det) == want[:2], (bit, n, det, want[:2])
    start = sum(z for _p, z in f.tab[:16])
    assert oracle.bz2_decompress_block(f.data, pos)[2] == f.out[start:start + f.tab[16][1]]
    assert oracle.bz2_decompress_block(f.data, end)[:2] == (0, 0) and oracle.bz2_decompress_block(f.data, pos + 1)[:2] == (-2, 0)
