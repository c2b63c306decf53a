"""Host-side mirror of the reference's module API for the bzip2 path.

    compressjs.Bzip2.compressFile(input, [output], [level])      lib/Bzip2.js:879-929
    compressjs.BWT.bwtransform2(T, U, n, [k]) -> pidx            lib/BWT.js:372-417

with the input/output coercions of lib/Util.js:9-103 translated to Python objects.  The primary
host binding for the reference's own language is js/ (N-API); this module is the same thin layer
for Python callers, bench.py and the tests.  Every call goes through the C ABI
(include/compressjs_amd.h) into the HIP kernels; nothing here computes on the CPU.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib

EOF_BYTE = -1          # Stream.EOF (lib/Stream.js)


class Context:
    """One GPU context (cjs_ctx): HIP stream + HBM workspace for `batch_blocks` blocks."""

    def __init__(self, device: int = 0, batch_blocks: int = 128):
        self.L = _lib.load()
        self.h = self.L.cjs_create(device, batch_blocks)
        if not self.h:
            raise _lib.CompressjsAmdError(
                "cjs_create failed: no MI355X visible or out of HBM (the product has no CPU path)")
        self.device = device

    def close(self):
        if getattr(self, "h", None):
            self.L.cjs_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # host buffers -------------------------------------------------------------------------
    def _staging(self, cap: int) -> np.ndarray:
        """A host buffer kept across calls: a fresh np.empty() would fault in every page the D2H copy touches."""
        buf = getattr(self, "_obuf", None)
        if buf is None or buf.size < cap:
            buf = np.zeros(cap, dtype=np.uint8)
            self._obuf = buf
        return buf

    def compress(self, data: np.ndarray, level: int = 9) -> bytes:
        d = np.ascontiguousarray(data, dtype=np.uint8)
        cap = int(self.L.cjs_bz2_compress_bound(d.size))
        out = self._staging(cap)
        n = self.L.cjs_bz2_compress(self.h, d.ctypes.data, d.size, int(level), out.ctypes.data, cap)
        _lib.check(n, "cjs_bz2_compress")
        return out[:n].tobytes()

    def compress_many(self, docs, level: int = 9) -> list:
        """Many independent inputs in one call (cjs_bz2_compress_batch): one .bz2 stream per document, each equal to
        compress(doc, level)."""
        arrs = [np.ascontiguousarray(d, dtype=np.uint8).reshape(-1) for d in docs]
        if not arrs:
            level = int(level)
            if level < 1 or level > 9:
                _lib.check(-20, "cjs_bz2_compress_batch")
            return []
        off = np.zeros(len(arrs) + 1, dtype=np.uint64)
        off[1:] = np.cumsum([a.size for a in arrs], dtype=np.uint64)
        flat = np.concatenate(arrs) if int(off[-1]) else np.zeros(1, np.uint8)
        cap = int(self.L.cjs_bz2_compress_batch_bound(int(off[-1]), len(arrs)))
        out = self._staging(cap)
        out_off = np.zeros(len(arrs) + 1, dtype=np.uint64)
        n = self.L.cjs_bz2_compress_batch(self.h, flat.ctypes.data, off.ctypes.data, len(arrs), int(level), out.ctypes.data, cap,
                                          out_off.ctypes.data)
        _lib.check(n, "cjs_bz2_compress_batch")
        return [out[int(out_off[k]):int(out_off[k + 1])].tobytes() for k in range(len(arrs))]

    def compress_many_device(self, d_in, d_off, d_out, d_out_off, level: int = 9) -> int:
        """The same with everything resident in HBM: d_in / d_out torch uint8 CUDA tensors, d_off / d_out_off 64-bit integer
        CUDA tensors of count + 1 elements (document d = d_in[d_off[d]:d_off[d+1]]; stream d = d_out[d_out_off[d]:d_out_off[d+1]]).
        Returns the total number of bytes written."""
        import torch
        count = int(d_off.numel()) - 1
        for name, t, dt in (("d_in", d_in, (torch.uint8,)), ("d_out", d_out, (torch.uint8,)),
                            ("d_off", d_off, (torch.int64, getattr(torch, "uint64", torch.int64))),
                            ("d_out_off", d_out_off, (torch.int64, getattr(torch, "uint64", torch.int64)))):
            if t.dtype not in dt or not t.is_contiguous():
                raise ValueError("%s: a contiguous tensor of dtype %s" % (name, dt[0]))
            if t.device != d_in.device:
                raise ValueError("%s: on another device than d_in" % name)
        if count < 0 or d_out_off.numel() < count + 1:
            raise ValueError("d_off / d_out_off: count + 1 elements")
        n = self.L.cjs_bz2_compress_batch_device(self.h, d_in.data_ptr(), d_off.data_ptr(), count, int(level),
                                                 d_out.data_ptr(), d_out.numel(), d_out_off.data_ptr())
        return _lib.check(n, "cjs_bz2_compress_batch_device")

    def bwtc_compress(self, data: np.ndarray, level: int = 9, declared_size=None) -> bytes:
        d = np.ascontiguousarray(data, dtype=np.uint8)
        cap = int(self.L.cjs_bwtc_compress_bound(d.size))
        out = np.empty(cap, dtype=np.uint8)
        n = self.L.cjs_bwtc_compress(self.h, d.ctypes.data, d.size, int(level), out.ctypes.data, cap,
                                     d.size if declared_size is None else declared_size)
        _lib.check(n, "cjs_bwtc_compress")
        return out[:n].tobytes()

    def bwtc_compress_many(self, docs, level: int = 9) -> list:
        """Many independent inputs in one call (cjs_bwtc_compress_batch): one BWTC stream per document, each equal to
        bwtc_compress(doc, level).  At every level the model of every block (FenwickModel for 6-9, DefSumModel for 1-5) and the
        range coder, one coder per document, run on the GPU too."""
        arrs = [np.ascontiguousarray(d, dtype=np.uint8).reshape(-1) for d in docs]
        if not arrs:
            return []
        off = np.zeros(len(arrs) + 1, dtype=np.uint64)
        off[1:] = np.cumsum([a.size for a in arrs], dtype=np.uint64)
        flat = np.concatenate(arrs) if int(off[-1]) else np.zeros(1, np.uint8)
        cap = int(self.L.cjs_bwtc_compress_batch_bound(int(off[-1]), len(arrs)))
        out = self._staging(cap)
        out_off = np.zeros(len(arrs) + 1, dtype=np.uint64)
        n = self.L.cjs_bwtc_compress_batch(self.h, flat.ctypes.data, off.ctypes.data, len(arrs), int(level), out.ctypes.data, cap,
                                           out_off.ctypes.data)
        _lib.check(n, "cjs_bwtc_compress_batch")
        return [out[int(out_off[k]):int(out_off[k + 1])].tobytes() for k in range(len(arrs))]

    def bwtc_compress_many_device(self, d_in, d_off, d_out, d_out_off, level: int = 9) -> int:
        """The same with everything resident in HBM: tensors as for compress_many_device.  Returns the total number of bytes
        written."""
        import torch
        count = int(d_off.numel()) - 1
        for name, t, dt in (("d_in", d_in, (torch.uint8,)), ("d_out", d_out, (torch.uint8,)),
                            ("d_off", d_off, (torch.int64, getattr(torch, "uint64", torch.int64))),
                            ("d_out_off", d_out_off, (torch.int64, getattr(torch, "uint64", torch.int64)))):
            if t.dtype not in dt or not t.is_contiguous():
                raise ValueError("%s: a contiguous tensor of dtype %s" % (name, dt[0]))
            if t.device != d_in.device:
                raise ValueError("%s: on another device than d_in" % name)
        if count < 0 or d_out_off.numel() < count + 1:
            raise ValueError("d_off / d_out_off: count + 1 elements")
        n = self.L.cjs_bwtc_compress_batch_device(self.h, d_in.data_ptr(), d_off.data_ptr(), count, int(level),
                                                  d_out.data_ptr(), d_out.numel(), d_out_off.data_ptr())
        return _lib.check(n, "cjs_bwtc_compress_batch_device")

    def decompress(self, stream, multistream: bool = False) -> bytes:
        """Bzip2.decompressFile on host buffers; raises the reference's TypeError(.errorCode) on bad input."""
        d = np.ascontiguousarray(stream, dtype=np.uint8)
        n = self.L.cjs_bz2_decompress(self.h, d.ctypes.data, d.size, None, 0, int(bool(multistream)))
        if n == -21:                                   # size now known: fetch the retained result
            n = int(self.L.cjs_bz2_last_size(self.h))
            out = self._staging(max(n, 1))
            _lib.check(self.L.cjs_bz2_fetch(self.h, out.ctypes.data, n), "cjs_bz2_fetch")
            return out[:n].tobytes()
        if n < 0:
            _lib.raise_decode_error(self.L, self.h, int(n))
        return b""

    def decompress_many(self, streams, multistream: bool = False, return_errors: bool = False) -> list:
        """Many independent .bz2 documents in one call (cjs_bz2_decompress_batch): entry d is decompress(streams[d], multistream).
        A document that fails raises what decompress would raise for it, with .index = d (the first failing one) - or, with
        return_errors, that exception instance takes its place in the list and the other documents are still delivered."""
        arrs = [_coerce_input(s).reshape(-1) for s in streams]
        if not arrs:
            return []
        count = len(arrs)
        off = np.zeros(count + 1, dtype=np.uint64)
        off[1:] = np.cumsum([a.size for a in arrs], dtype=np.uint64)
        flat = np.concatenate(arrs) if int(off[-1]) else np.zeros(1, np.uint8)
        out_off = np.zeros(count + 1, dtype=np.uint64)
        status = np.zeros(count, dtype=np.int32)
        detail = np.zeros(3 * count, dtype=np.uint32)
        out = self._staging(1)
        n = self.L.cjs_bz2_decompress_batch(self.h, flat.ctypes.data, off.ctypes.data, count, int(bool(multistream)), out.ctypes.data,
                                            0, out_off.ctypes.data, status.ctypes.data, detail.ctypes.data)
        if n == -21:                                   # sizes now known: fetch the retained result
            n = int(self.L.cjs_bz2_last_size(self.h))
            out = self._staging(max(n, 1))
            n = self.L.cjs_bz2_fetch(self.h, out.ctypes.data, n)
        _lib.check(n, "cjs_bz2_decompress_batch")
        res = []
        for k in range(count):
            if status[k]:
                err = _lib.decode_error(int(status[k]), int(detail[3 * k]), int(detail[3 * k + 1]), int(detail[3 * k + 2]))
                err.index = k
                if not return_errors:
                    raise err
                res.append(err)
            else:
                res.append(out[int(out_off[k]):int(out_off[k + 1])].tobytes())
        return res

    def decompress_many_device(self, d_in, d_off, d_out, d_out_off, d_status, multistream: bool = False, d_detail=None) -> int:
        """The same with everything resident in HBM: d_in / d_out torch uint8 CUDA tensors, d_off / d_out_off 64-bit integer CUDA
        tensors of count + 1 elements, d_status an int32 CUDA tensor of count elements (0 or the reference's Err code of document
        d; a failed document contributes no bytes), d_detail an optional 32-bit CUDA tensor of 3 * count elements.  Returns the
        total number of decoded bytes."""
        import torch
        count = int(d_off.numel()) - 1
        i64 = (torch.int64, getattr(torch, "uint64", torch.int64))
        i32 = (torch.int32, getattr(torch, "uint32", torch.int32))
        for name, t, dt in (("d_in", d_in, (torch.uint8,)), ("d_out", d_out, (torch.uint8,)), ("d_off", d_off, i64),
                            ("d_out_off", d_out_off, i64), ("d_status", d_status, (torch.int32,)), ("d_detail", d_detail, i32)):
            if t is None and name == "d_detail":
                continue
            if t.dtype not in dt or not t.is_contiguous():
                raise ValueError("%s: a contiguous tensor of dtype %s" % (name, dt[0]))
            if t.device != d_in.device:
                raise ValueError("%s: on another device than d_in" % name)
        if count < 0 or d_out_off.numel() < count + 1 or d_status.numel() < count or (d_detail is not None and d_detail.numel() < 3 * count):
            raise ValueError("d_off / d_out_off: count + 1 elements, d_status: count, d_detail: 3 * count")
        n = self.L.cjs_bz2_decompress_batch_device(self.h, d_in.data_ptr(), d_off.data_ptr(), count, int(bool(multistream)),
                                                   d_out.data_ptr(), d_out.numel(), d_out_off.data_ptr(), d_status.data_ptr(),
                                                   d_detail.data_ptr() if d_detail is not None else None)
        return _lib.check(n, "cjs_bz2_decompress_batch_device")

    def decompress_block(self, stream, bitpos: int) -> bytes:
        """Bzip2.decompressBlock (lib/Bzip2.js:482-503)."""
        d = np.ascontiguousarray(stream, dtype=np.uint8)
        n = self.L.cjs_bz2_decompress_block(self.h, d.ctypes.data, d.size, int(bitpos), None, 0)
        if n == -21:
            n = int(self.L.cjs_bz2_last_size(self.h))
            out = self._staging(max(n, 1))
            _lib.check(self.L.cjs_bz2_fetch(self.h, out.ctypes.data, n), "cjs_bz2_fetch")
            return out[:n].tobytes()
        if n < 0:
            _lib.raise_decode_error(self.L, self.h, int(n))
        return b""

    def decompress_blocks(self, stream, positions, return_errors: bool = False) -> list:
        """Many blocks of one stream in one call (cjs_bz2_decompress_blocks): index once with table, fetch many.  Entry k is
        decompress_block(stream, positions[k]); positions are bit positions below 2**64, in any order, duplicates allowed.  A
        request that fails raises what decompress_block would raise for it, with .index = k (the first failing one) - or, with
        return_errors, that exception instance takes its place in the list and the other blocks are still delivered."""
        d = _coerce_input(stream).reshape(-1)
        pos = np.array([int(p) for p in positions], dtype=np.uint64)
        count = int(pos.size)
        if not count:
            return []
        out_off = np.zeros(count + 1, dtype=np.uint64)
        status = np.zeros(count, dtype=np.int32)
        detail = np.zeros(3 * count, dtype=np.uint32)
        out = self._staging(1)
        n = self.L.cjs_bz2_decompress_blocks(self.h, d.ctypes.data if d.size else None, d.size, pos.ctypes.data, count,
                                             out.ctypes.data, 0, out_off.ctypes.data, status.ctypes.data, detail.ctypes.data)
        if n == -21:                                   # sizes now known: fetch the retained result
            n = int(self.L.cjs_bz2_last_size(self.h))
            out = self._staging(max(n, 1))
            n = self.L.cjs_bz2_fetch(self.h, out.ctypes.data, n)
        _lib.check(n, "cjs_bz2_decompress_blocks")
        res = []
        for k in range(count):
            if status[k]:
                err = _lib.decode_error(int(status[k]), int(detail[3 * k]), int(detail[3 * k + 1]), int(detail[3 * k + 2]))
                err.index = k
                if not return_errors:
                    raise err
                res.append(err)
            else:
                res.append(out[int(out_off[k]):int(out_off[k + 1])].tobytes())
        return res

    def decompress_blocks_device(self, d_in, d_pos, d_out, d_out_off, d_status, d_detail=None) -> int:
        """The same with everything resident in HBM: d_in (the stream) / d_out torch uint8 CUDA tensors, d_pos a 64-bit integer CUDA
        tensor of count bit positions, d_out_off one of count + 1 elements, d_status an int32 CUDA tensor of count elements (0 or
        the reference's Err code of request k; a failed request contributes no bytes), d_detail an optional 32-bit CUDA tensor of
        3 * count elements.  Returns the total number of decoded bytes."""
        import torch
        count = int(d_pos.numel())
        i64 = (torch.int64, getattr(torch, "uint64", torch.int64))
        i32 = (torch.int32, getattr(torch, "uint32", torch.int32))
        for name, t, dt in (("d_in", d_in, (torch.uint8,)), ("d_out", d_out, (torch.uint8,)), ("d_pos", d_pos, i64),
                            ("d_out_off", d_out_off, i64), ("d_status", d_status, (torch.int32,)), ("d_detail", d_detail, i32)):
            if t is None and name == "d_detail":
                continue
            if t.dtype not in dt or not t.is_contiguous():
                raise ValueError("%s: a contiguous tensor of dtype %s" % (name, dt[0]))
            if t.device != d_in.device:
                raise ValueError("%s: on another device than d_in" % name)
        if d_out_off.numel() < count + 1 or d_status.numel() < count or (d_detail is not None and d_detail.numel() < 3 * count):
            raise ValueError("d_out_off: count + 1 elements, d_status: count, d_detail: 3 * count")
        n = self.L.cjs_bz2_decompress_blocks_device(self.h, d_in.data_ptr(), d_in.numel(), d_pos.data_ptr(), count,
                                                    d_out.data_ptr(), d_out.numel(), d_out_off.data_ptr(), d_status.data_ptr(),
                                                    d_detail.data_ptr() if d_detail is not None else None)
        return _lib.check(n, "cjs_bz2_decompress_blocks_device")

    def table(self, stream, multistream: bool = False):
        """Bzip2.table (lib/Bzip2.js:508-548) -> [(bit position, decoded bytes)]."""
        d = np.ascontiguousarray(stream, dtype=np.uint8)
        cap = d.size // 8 + 16
        pos = np.zeros(cap, dtype=np.uint64)
        size = np.zeros(cap, dtype=np.uint64)
        n = self.L.cjs_bz2_table(self.h, d.ctypes.data, d.size, int(bool(multistream)), pos.ctypes.data, size.ctypes.data, cap)
        if n < 0:
            _lib.raise_decode_error(self.L, self.h, int(n))
        return [(int(pos[i]), int(size[i])) for i in range(int(n))]

    def bwtc_decompress(self, stream) -> bytes:
        """BWTC.decompressFile (lib/BWTC.js:141-233): host range decoder, inverse BWT on the GPU (K6)."""
        d = np.ascontiguousarray(stream, dtype=np.uint8)
        declared = C.c_int64(-1)
        n = self.L.cjs_bwtc_decompress(self.h, d.ctypes.data, d.size, None, 0, C.byref(declared))
        if n == -21:
            n = int(self.L.cjs_bwtc_last_size(self.h))
            out = self._staging(max(n, 1))
            _lib.check(self.L.cjs_bwtc_fetch(self.h, out.ctypes.data, n), "cjs_bwtc_fetch")
            return out[:n].tobytes()
        _lib.check(n, "cjs_bwtc_decompress")
        return b""

    def bwtc_decompress_many(self, streams, return_errors: bool = False) -> list:
        """Many independent BWTC streams in one call (cjs_bwtc_decompress_batch_ex): entry d is bwtc_decompress(streams[d]).  Every
        level runs one range decoder per document on the GPU (levels 1-5 through CJS_BWTC_DEC_DEFSUM_DEVICE).  A document that fails raises what bwtc_decompress raises for it, with
        .index = d (the first failing one) - or, with return_errors, that exception takes its place in the list and the other
        documents are still delivered."""
        arrs = [_coerce_input(s).reshape(-1) for s in streams]
        if not arrs:
            return []
        count = len(arrs)
        off = np.zeros(count + 1, dtype=np.uint64)
        off[1:] = np.cumsum([a.size for a in arrs], dtype=np.uint64)
        flat = np.concatenate(arrs) if int(off[-1]) else np.zeros(1, np.uint8)
        out_off = np.zeros(count + 1, dtype=np.uint64)
        status = np.zeros(count, dtype=np.int32)
        out = self._staging(1)
        n = self.L.cjs_bwtc_decompress_batch_ex(self.h, flat.ctypes.data, off.ctypes.data, count, out.ctypes.data, 0, out_off.ctypes.data,
                                                status.ctypes.data, None, _lib.BWTC_DEC_DEFSUM_DEVICE)
        if n == -21:                                   # sizes now known: fetch the retained result
            n = int(self.L.cjs_bwtc_last_size(self.h))
            out = self._staging(max(n, 1))
            n = self.L.cjs_bwtc_fetch(self.h, out.ctypes.data, n)
        _lib.check(n, "cjs_bwtc_decompress_batch_ex")
        res = []
        for k in range(count):
            if status[k]:
                try:
                    _lib.check(int(status[k]), "cjs_bwtc_decompress")
                except Exception as err:               # noqa: BLE001 - the single call's exception for this code
                    err.index = k
                    if not return_errors:
                        raise
                    res.append(err)
            else:
                res.append(out[int(out_off[k]):int(out_off[k + 1])].tobytes())
        return res

    def bwtc_decompress_many_device(self, d_in, d_off, d_out, d_out_off, d_status, d_declared=None) -> int:
        """The same (cjs_bwtc_decompress_batch_device_ex) with everything resident in HBM: d_in / d_out torch uint8 CUDA tensors,
        d_off / d_out_off 64-bit integer CUDA tensors of count + 1 elements, d_status an int32 CUDA tensor of count elements (0, -30 or -31; a failed document contributes
        no bytes), d_declared an optional int64 CUDA tensor of count elements (the size every header records, -1: unknown).
        Returns the total number of decoded bytes."""
        import torch
        count = int(d_off.numel()) - 1
        i64 = (torch.int64, getattr(torch, "uint64", torch.int64))
        for name, t, dt in (("d_in", d_in, (torch.uint8,)), ("d_out", d_out, (torch.uint8,)), ("d_off", d_off, i64),
                            ("d_out_off", d_out_off, i64), ("d_status", d_status, (torch.int32,)), ("d_declared", d_declared, (torch.int64,))):
            if t is None and name == "d_declared":
                continue
            if t.dtype not in dt or not t.is_contiguous():
                raise ValueError("%s: a contiguous tensor of dtype %s" % (name, dt[0]))
            if t.device != d_in.device:
                raise ValueError("%s: on another device than d_in" % name)
        if count < 0 or d_out_off.numel() < count + 1 or d_status.numel() < count or (d_declared is not None and d_declared.numel() < count):
            raise ValueError("d_off / d_out_off: count + 1 elements, d_status / d_declared: count")
        n = self.L.cjs_bwtc_decompress_batch_device_ex(self.h, d_in.data_ptr(), d_off.data_ptr(), count, d_out.data_ptr(), d_out.numel(),
                                                       d_out_off.data_ptr(), d_status.data_ptr(),
                                                       d_declared.data_ptr() if d_declared is not None else None, _lib.BWTC_DEC_DEFSUM_DEVICE)
        return _lib.check(n, "cjs_bwtc_decompress_batch_device_ex")

    def decompress_device(self, d_in, d_out, multistream: bool = False) -> int:
        """Stream and output are torch uint8 CUDA tensors; returns the decoded size."""
        n = self.L.cjs_bz2_decompress_device(self.h, d_in.data_ptr(), d_in.numel(), d_out.data_ptr(), d_out.numel(),
                                             int(bool(multistream)))
        if n < 0 and n != -21:
            _lib.raise_decode_error(self.L, self.h, int(n))
        return _lib.check(n, "cjs_bz2_decompress_device")

    @property
    def last_decode_ms(self) -> float:
        return float(self.L.cjs_bz2_last_decode_ms(self.h))

    # device-resident (torch tensors on this context's GPU) ----------------------------------
    def compress_device(self, d_in, d_out, level: int = 9) -> int:
        """d_in / d_out: torch uint8 CUDA tensors.  Returns the number of bytes written."""
        n = self.L.cjs_bz2_compress_device(self.h, d_in.data_ptr(), d_in.numel(), int(level),
                                           d_out.data_ptr(), d_out.numel())
        return _lib.check(n, "cjs_bz2_compress_device")

    def plan(self, d_in, level: int = 9) -> int:
        """RLE1/block-split pre-pass over the whole input; returns the number of blocks."""
        return _lib.check(self.L.cjs_bz2_plan(self.h, d_in.data_ptr(), d_in.numel(), int(level)),
                          "cjs_bz2_plan")

    def lcg_ascii_device(self, d_out, seed: int, first: int = 0):
        """Fill the torch uint8 CUDA tensor d_out with bytes [first, first + len) of LCG(N, seed), on the device."""
        return _lib.check(self.L.cjs_lcg_ascii_device(self.h, d_out.data_ptr(), d_out.numel(), int(seed) & 0xFFFFFFFF, int(first)),
                          "cjs_lcg_ascii_device")

    # parallel plan of a slice (compressjs_amd/dist.py: sharded_compress_parallel; include/compressjs_amd.h)
    def plan_scan(self, d_in, level: int = 9) -> int:
        """K0's scans over d_in (slice + following margin); returns the input's own RLE1 cost total."""
        return _lib.check(self.L.cjs_bz2_plan_scan(self.h, d_in.data_ptr(), d_in.numel(), int(level)), "cjs_bz2_plan_scan")

    def plan_cost(self, pos: int) -> int:
        return _lib.check(self.L.cjs_bz2_plan_cost(self.h, int(pos)), "cjs_bz2_plan_cost")

    def plan_phase(self, own_len: int, phase: int, last: bool) -> int:
        """Blocks that start in [0, own_len): their number, or -1 when the slice cannot be planned on its own (CJS_E_SPEC)."""
        n = self.L.cjs_bz2_plan_phase(self.h, int(own_len), int(phase), 1 if last else 0)
        if n == -25:
            return -1
        return _lib.check(n, "cjs_bz2_plan_phase")

    def plan_chain(self, own_len: int, t0: int, last: bool):
        """The slice's plan as a link of a chain (round 6): (blocks that start in [0, own_len), target of the first boundary at or
        beyond own_len in this input's own cost prefix), or (-1, t0) when the slice cannot be planned on its own (CJS_E_SPEC)."""
        tn = C.c_uint64(0)
        n = self.L.cjs_bz2_plan_chain(self.h, int(own_len), int(t0), 1 if last else 0, C.byref(tn))
        if n == -25:
            return -1, int(t0)
        return _lib.check(n, "cjs_bz2_plan_chain"), int(tn.value)

    def plan_block_start(self, k: int) -> int:
        """First input byte (relative to the planned input) of block k of the current plan."""
        return _lib.check(self.L.cjs_bz2_plan_block_start(self.h, int(k)), "cjs_bz2_plan_block_start")

    def encode_blocks(self, first: int, count: int, d_seg):
        """Encode blocks [first, first+count) of the planned input into d_seg (bit 0 aligned).
        Returns (bits, crc_fold, n_blocks)."""
        fold, cnt = C.c_uint32(0), C.c_uint32(0)
        bits = self.L.cjs_bz2_encode_blocks(self.h, first, count, d_seg.data_ptr(), d_seg.numel(),
                                            C.byref(fold), C.byref(cnt))
        _lib.check(bits, "cjs_bz2_encode_blocks")
        return int(bits), int(fold.value), int(cnt.value)

    def shift_bits(self, d_seg, nbytes: int, s: int, d_out):
        """d_out[:nbytes+1] = d_seg[:nbytes] shifted right by s bits (torch uint8 tensors on this context's device)."""
        return _lib.check(self.L.cjs_shift_bits(self.h, d_seg.data_ptr(), int(nbytes), int(s), d_out.data_ptr()), "cjs_shift_bits")

    @property
    def last_device_ms(self) -> float:
        return float(self.L.cjs_last_device_ms(self.h))

    @property
    def last_block_count(self) -> int:
        return int(self.L.cjs_last_block_count(self.h))


def compress_multi(contexts, data, level: int = 9) -> bytes:
    """Bzip2.compressFile over several GPUs from one process (cjs_bz2_compress_multi): `contexts` = Context objects on
    different devices; segments of about one batch of blocks go round-robin to them.  Same bytes as one context."""
    d = np.ascontiguousarray(data, dtype=np.uint8)
    L = contexts[0].L
    cap = int(L.cjs_bz2_compress_bound(d.size))
    out = contexts[0]._staging(cap)
    hs = (C.c_void_p * len(contexts))(*[c.h for c in contexts])
    n = L.cjs_bz2_compress_multi(hs, len(contexts), d.ctypes.data, d.size, int(level), out.ctypes.data, cap)
    _lib.check(n, "cjs_bz2_compress_multi")
    return out[:n].tobytes()


_default_ctx = None


def default_context() -> Context:
    global _default_ctx
    if _default_ctx is None:
        _default_ctx = Context(0, 32)
    return _default_ctx


def _coerce_input(inp) -> np.ndarray:
    """Util.coerceInputStream (lib/Util.js:9-29): buffers are used as they are, stream objects
    are drained through readByte() until it returns -1."""
    if hasattr(inp, "readByte"):
        buf = bytearray()
        while True:
            b = inp.readByte()
            if b == EOF_BYTE:
                break
            buf.append(b & 0xFF)
        return np.frombuffer(bytes(buf), dtype=np.uint8)
    if isinstance(inp, np.ndarray):
        return np.ascontiguousarray(inp, dtype=np.uint8)
    if isinstance(inp, (bytes, bytearray, memoryview)):
        return np.frombuffer(bytes(inp), dtype=np.uint8)
    return np.asarray(list(inp), dtype=np.uint8)


def _deliver(data: bytes, output):
    """Util.coerceOutputStream (lib/Util.js:85-103): None -> exact-length bytes; object with
    writeByte -> bytes pushed one at a time and the object returned; int -> expected size;
    writable buffer -> filled, size must match."""
    if output is None or output is False:
        return data
    if hasattr(output, "writeByte"):
        for b in data:
            output.writeByte(b)
        if hasattr(output, "flush"):
            output.flush()
        return output
    if isinstance(output, int):
        if output != len(data):
            raise TypeError("outputsize does not match decoded input")    # lib/Util.js:69-71
        return data
    mv = memoryview(output)
    if len(mv) != len(data):
        raise TypeError("outputsize does not match decoded input")
    mv[:] = data
    return output


class Bzip2:
    """compressjs.Bzip2 (lib/Bzip2.js:878-933), compress side on MI355X."""

    @staticmethod
    def compressFile(inStream, outStream=None, props=None):
        level = 9
        if isinstance(props, (int, float)) and not isinstance(props, bool):   # lib/Bzip2.js:884-887
            level = props
        if level < 1 or level > 9 or level != int(level):
            raise ValueError("Invalid block size multiplier")                  # :888-890
        data = _coerce_input(inStream)
        return _deliver(default_context().compress(data, int(level)), outStream)

    @staticmethod
    def compressFiles(inputs, props=None):
        """Many independent inputs, one .bz2 stream each, in one trip through the GPU (the reference has no batched entry):
        [Bzip2.compressFile(x, None, props) for x in inputs], bit for bit."""
        level = 9
        if isinstance(props, (int, float)) and not isinstance(props, bool):   # lib/Bzip2.js:884-887
            level = props
        if level < 1 or level > 9 or level != int(level):
            raise ValueError("Invalid block size multiplier")                  # :888-890
        return default_context().compress_many([_coerce_input(x) for x in inputs], int(level))

    @staticmethod
    def decompressFile(inStream, outStream=None, multistream=False):
        """Bzip2.decompressFile = Bunzip.decode (lib/Bzip2.js:454-481) on the GPU decoder (K7-K9)."""
        data = _coerce_input(inStream)
        return _deliver(default_context().decompress(data, multistream), outStream)

    @staticmethod
    def decompressFiles(inputs, multistream=False, return_errors=False):
        """Many independent .bz2 inputs in one trip through the GPU (the reference has no batched entry):
        [Bzip2.decompressFile(x, None, multistream) for x in inputs]; a document that fails raises its error with .index set."""
        return default_context().decompress_many([_coerce_input(x) for x in inputs], multistream, return_errors)

    @staticmethod
    def decompressBlock(inStream, bitPos, outStream=None):
        """Bzip2.decompressBlock = Bunzip.decodeBlock (lib/Bzip2.js:482-503)."""
        data = _coerce_input(inStream)
        return _deliver(default_context().decompress_block(data, bitPos), outStream)

    @staticmethod
    def decompressBlocks(inStream, bitPositions, return_errors=False):
        """Many blocks of one stream in one trip through the GPU (the reference has no batched entry): index once with table, then
        [Bzip2.decompressBlock(inStream, p) for p in bitPositions]; a request that fails raises its error with .index set."""
        return default_context().decompress_blocks(_coerce_input(inStream), bitPositions, return_errors)

    @staticmethod
    def table(inStream, callback, multistream=False):
        """Bzip2.table (lib/Bzip2.js:508-548): callback(position in bits, decoded bytes) per block."""
        for pos, size in default_context().table(_coerce_input(inStream), multistream):
            callback(pos, size)


class HuffmanAllocator:
    """require('compressjs/lib/HuffmanAllocator') (lib/HuffmanAllocator.js:199-226)."""

    @staticmethod
    def allocateHuffmanCodeLengths(array, maximumLength):
        """In place, like the reference: ascending weights in, code lengths out."""
        a = np.ascontiguousarray(np.asarray(array, dtype=np.int64))
        _lib.check(_lib.load().cjs_huff_lengths(a.ctypes.data, a.size, int(maximumLength)), "cjs_huff_lengths")
        for i in range(a.size):
            array[i] = int(a[i])

    @staticmethod
    def allocate_many(arrays, maximumLength):
        """`count` independent arrays in one launch; returns a list of lists."""
        off = np.zeros(len(arrays) + 1, dtype=np.uint32)
        off[1:] = np.cumsum([len(a) for a in arrays])
        flat = np.ascontiguousarray(np.concatenate([np.asarray(a, dtype=np.int64) for a in arrays]) if arrays else np.zeros(0, np.int64))
        _lib.check(_lib.load().cjs_huff_lengths_batch(flat.ctypes.data, off.ctypes.data, len(arrays), int(maximumLength)),
                   "cjs_huff_lengths_batch")
        return [flat[off[k]:off[k + 1]].tolist() for k in range(len(arrays))]


class BWTC:
    """compressjs.BWTC (lib/BWTC.js), compress side, levels 6-9: BWT + MTF/RLE2 on MI355X, the
    adaptive range coder on the host."""

    @staticmethod
    def compressFile(inStream, outStream=None, props=None):
        level = 9
        if isinstance(props, (int, float)) and not isinstance(props, bool) and 1 <= props <= 9:
            level = int(props)                                                   # lib/BWTC.js:16-19
        known = not hasattr(inStream, "readByte") or hasattr(inStream, "size")
        data = _coerce_input(inStream)
        size = data.size if known else -1                                        # lib/Util.js:119-124
        return _deliver(default_context().bwtc_compress(data, level, size), outStream)

    @staticmethod
    def compressFiles(inputs, props=None):
        """Many independent inputs, one BWTC stream each, in one call (the reference has no batched entry):
        [BWTC.compressFile(x, None, props) for x in inputs], bit for bit, each with its size declared."""
        level = 9
        if isinstance(props, (int, float)) and not isinstance(props, bool) and 1 <= props <= 9:
            level = int(props)                                                   # lib/BWTC.js:16-19
        return default_context().bwtc_compress_many([_coerce_input(x) for x in inputs], level)

    @staticmethod
    def decompressFile(inStream, outStream=None):
        """BWTC.decompressFile (lib/BWTC.js:141-233), levels 6-9."""
        return _deliver(default_context().bwtc_decompress(_coerce_input(inStream)), outStream)

    @staticmethod
    def decompressFiles(inputs, return_errors=False):
        """Many independent BWTC streams of any level in one call (the reference has no batched entry; cjs_bwtc_decompress_batch_ex
        with levels 1-5 on the GPU too): [BWTC.decompressFile(x) for x in inputs]; a document that fails raises its error with .index set, or takes its place in the list with return_errors."""
        return default_context().bwtc_decompress_many([_coerce_input(x) for x in inputs], return_errors)


class BWT:
    """compressjs.BWT (lib/BWT.js:302-419): the cyclic transform used by bzip2."""

    @staticmethod
    def bwtransform(T, U, A, n, alphabetSize=256):
        """BWT.bwtransform (lib/BWT.js:328-350); A is the reference's scratch array, unused here."""
        t = np.ascontiguousarray(np.asarray(T)[:n], dtype=np.uint8)
        u = np.zeros(max(n, 1), dtype=np.uint8)
        p = C.c_uint32(0)
        _lib.check(_lib.load().cjs_bwt_linear(t.ctypes.data, u.ctypes.data, n, C.byref(p)), "cjs_bwt_linear")
        U[:n] = u[:n] if isinstance(U, np.ndarray) else bytes(u[:n])
        return int(p.value)

    @staticmethod
    def unbwtransform(T, U, LF, n, pidx):
        """BWT.unbwtransform (lib/BWT.js:352-363); LF is the reference's scratch array, unused."""
        t = np.ascontiguousarray(np.asarray(T)[:n], dtype=np.uint8)
        u = np.zeros(max(n, 1), dtype=np.uint8)
        _lib.check(_lib.load().cjs_unbwt_linear(t.ctypes.data, u.ctypes.data, n, int(pidx)), "cjs_unbwt_linear")
        U[:n] = u[:n] if isinstance(U, np.ndarray) else bytes(u[:n])

    @staticmethod
    def unbwtransform_many(blocks, pidxs):
        """BWT.unbwtransform of many blocks in one call (cjs_unbwt_linear_batch): -> [bytes], entry k the text of (blocks[k], pidxs[k])."""
        arrs = [np.ascontiguousarray(np.asarray(b), dtype=np.uint8).reshape(-1) for b in blocks]
        if not arrs:
            return []
        off = np.zeros(len(arrs) + 1, dtype=np.uint64)
        off[1:] = np.cumsum([a.size for a in arrs], dtype=np.uint64)
        flat = np.concatenate(arrs) if int(off[-1]) else np.zeros(1, np.uint8)
        pidx = np.ascontiguousarray(np.asarray(pidxs, dtype=np.uint32))
        if pidx.size != len(arrs):
            raise ValueError("one primary index per block")
        u = np.zeros(max(int(off[-1]), 1), dtype=np.uint8)
        _lib.check(_lib.load().cjs_unbwt_linear_batch(flat.ctypes.data, off.ctypes.data, pidx.ctypes.data, len(arrs), u.ctypes.data),
                   "cjs_unbwt_linear_batch")
        return [u[int(off[k]):int(off[k + 1])].tobytes() for k in range(len(arrs))]

    @staticmethod
    def suffixsort(T, SA, n, alphabetSize=256):
        """BWT.suffixsort (lib/BWT.js:305-321)."""
        t = np.ascontiguousarray(np.asarray(T)[:n], dtype=np.uint8)
        sa = np.zeros(max(n, 1), dtype=np.int32)
        _lib.check(_lib.load().cjs_suffixsort(t.ctypes.data, sa.ctypes.data, n), "cjs_suffixsort")
        SA[:n] = sa[:n]
        return 0

    @staticmethod
    def bwtransform2(T, U, n, alphabetSize=256):
        t = np.ascontiguousarray(np.asarray(T)[:n], dtype=np.uint8)
        u = np.zeros(max(n, 1), dtype=np.uint8)
        p = C.c_uint32(0)
        _lib.check(_lib.load().cjs_bwt_cyclic(t.ctypes.data, u.ctypes.data, n, C.byref(p)),
                   "cjs_bwt_cyclic")
        U[:n] = u[:n] if isinstance(U, np.ndarray) else bytes(u[:n])
        return int(p.value)
