"""Host-resident encode / rebuild through the pinned-buffer pipeline
(include/redset_hip.h, "streaming pipeline"): cells live in host memory or in
files with redset's logical-file layout and stream through HBM."""
from __future__ import annotations

import ctypes
from ctypes import c_char_p, c_int, c_ulonglong, c_void_p
from typing import List, Optional, Sequence, Tuple

from . import _lib


class HostIO:
    """Cells in host memory, laid out like the device set layout."""

    def __init__(self, ranks: int, lofi_ptrs: Sequence[int], parity_ptrs: Sequence[int], cell_stride: int,
                 keepalive=(), pinned: bool = False):
        self.io = _lib.StreamIO()
        h = c_void_p()
        _lib.check(_lib.load().redset_hip_hostio_create(
            ranks, _lib.ptr_array(lofi_ptrs), _lib.ptr_array(parity_ptrs), cell_stride, int(pinned),
            ctypes.byref(self.io), ctypes.byref(h)), "hostio_create")
        self._h = h
        self._keep = keepalive

    def close(self):
        if self._h:
            _lib.load().redset_hip_hostio_destroy(self._h)
            self._h = None

    def __del__(self):  # pragma: no cover
        self.close()


class FileIO:
    """Member r's logical file = concatenation of files[r] = [(path, size), ...];
    parity at redundancy[r] + header[r] + slot * chunk (redset's layout)."""

    def __init__(self, files: Sequence[Sequence[Tuple[str, int]]], redundancy: Sequence[str],
                 headers: Optional[Sequence[int]], chunk: int, writable: Optional[Sequence[bool]] = None):
        p = len(files)
        nfiles = (c_int * p)(*[len(f) for f in files])
        flat = [x for f in files for x in f]
        paths = (c_char_p * max(1, len(flat)))(*[x[0].encode() for x in flat])
        sizes = (c_ulonglong * max(1, len(flat)))(*[int(x[1]) for x in flat])
        reds = (c_char_p * p)(*[x.encode() for x in redundancy])
        hdr = (c_ulonglong * p)(*([int(h) for h in headers] if headers else [0] * p))
        wr = (c_int * p)(*([1 if w else 0 for w in writable] if writable else [0] * p))
        self.io = _lib.StreamIO()
        h = c_void_p()
        _lib.check(_lib.load().redset_hip_fileio_create(
            p, nfiles, paths, sizes, reds, hdr, chunk, wr, ctypes.byref(self.io), ctypes.byref(h)),
            "fileio_create")
        self._h = h

    def close(self):
        if self._h:
            _lib.load().redset_hip_fileio_destroy(self._h)
            self._h = None

    def __del__(self):  # pragma: no cover
        self.close()


def _run(fn, *args) -> dict:
    st = _lib.StreamStats()
    _lib.check(fn(*args, ctypes.byref(st)), fn.__name__)
    return st.as_dict()


def rs_encode_stream(codec, chunk: int, io, first: int = 0, nstripes: int = 0, slice_bytes: int = 0,
                     io_threads: int = 0) -> dict:
    return _run(_lib.load().redset_hip_rs_encode_stream, codec._h, chunk, first, nstripes, slice_bytes,
                io_threads, ctypes.byref(io.io))


def rs_rebuild_stream(codec, lost: Sequence[int], chunk: int, io, first: int = 0, nstripes: int = 0,
                      slice_bytes: int = 0, io_threads: int = 0) -> dict:
    r = sorted(lost)
    arr = (c_int * len(r))(*r)
    return _run(_lib.load().redset_hip_rs_rebuild_stream, codec._h, len(r), arr, chunk, first, nstripes,
                slice_bytes, io_threads, ctypes.byref(io.io))


def xor_encode_stream(ranks: int, chunk: int, io, first: int = 0, nstripes: int = 0, slice_bytes: int = 0,
                      io_threads: int = 0) -> dict:
    return _run(_lib.load().redset_hip_xor_encode_stream, ranks, chunk, first, nstripes, slice_bytes,
                io_threads, ctypes.byref(io.io))


def xor_rebuild_stream(ranks: int, root: int, chunk: int, io, first: int = 0, nstripes: int = 0,
                       slice_bytes: int = 0, io_threads: int = 0) -> dict:
    return _run(_lib.load().redset_hip_xor_rebuild_stream, ranks, root, chunk, first, nstripes, slice_bytes,
                io_threads, ctypes.byref(io.io))


def _verify(fn, stripes: int, e: int, *args) -> dict:
    from .codec import rows_to_arrays

    st = _lib.StreamStats()
    rows = (_lib.VerifyRow * max(1, stripes * e))()
    _lib.check(fn(*args, ctypes.byref(st), rows, stripes * e), fn.__name__)
    mism, first = rows_to_arrays(rows[:stripes * e], stripes, e)
    return {"mismatch": mism, "first": first, "clean": not mism.any(), "stats": st.as_dict()}


def rs_verify_stream(codec, chunk: int, io, first: int = 0, nstripes: int = 0, slice_bytes: int = 0,
                     io_threads: int = 0) -> dict:
    """Verify a host-resident RS set: ``mismatch`` / ``first`` arrays
    [stripes of the call, e] (see codec.VerifyPlan.report), ``clean`` and the
    pipeline statistics. Reads only; io's write is never called."""
    n = nstripes if nstripes > 0 else codec.ranks
    return _verify(_lib.load().redset_hip_rs_verify_stream, n, codec.encoding, codec._h, chunk, first, nstripes,
                   slice_bytes, io_threads, ctypes.byref(io.io))


def xor_verify_stream(ranks: int, chunk: int, io, first: int = 0, nstripes: int = 0, slice_bytes: int = 0,
                      io_threads: int = 0) -> dict:
    n = nstripes if nstripes > 0 else ranks
    return _verify(_lib.load().redset_hip_xor_verify_stream, n, 1, ranks, chunk, first, nstripes, slice_bytes,
                   io_threads, ctypes.byref(io.io))


def rs_repair_stream(codec, chunk: int, io, first: int = 0, nstripes: int = 0, slice_bytes: int = 0,
                     io_threads: int = 0, apply: bool = True) -> dict:
    """Scrub a host-resident RS set (2 <= e <= 4) and correct every byte
    column with one wrong byte (include/redset_hip.h
    redset_hip_rs_repair_stream): the verify stream first -- a clean set ends
    there -- then the damaged stripes slice by slice through the repair
    kernel, writing back (``apply``) only the corrected cells' slices, then
    the check again. Returns the summary's fields, ``corrected`` / ``first``
    [stripes of the call, p], ``unlocated`` / ``first_unlocated`` [stripes of
    the call] (see codec.RepairPlan.report) and the statistics."""
    from .codec import repair_arrays

    n, p = (nstripes if nstripes > 0 else codec.ranks), codec.ranks
    st, summ = _lib.StreamStats(), _lib.RepairSummary()
    cells = (_lib.RepairCell * max(1, n * p))()
    stripes = (_lib.RepairStripe * max(1, n))()
    _lib.check(_lib.load().redset_hip_rs_repair_stream(
        codec._h, chunk, first, nstripes, slice_bytes, io_threads, ctypes.byref(io.io), int(bool(apply)),
        ctypes.byref(st), cells, n * p, stripes, n, ctypes.byref(summ)), "rs_repair_stream")
    corrected, first_off, unloc, first_unloc = repair_arrays(cells, stripes, n, p)
    out = summ.as_dict()
    out.update({"corrected": corrected, "first": first_off, "unlocated": unloc, "first_unlocated": first_unloc,
                "stats": st.as_dict()})
    return out


def rs_rebuild_checked_stream(codec, lost: Sequence[int], chunk: int, io, first: int = 0, nstripes: int = 0,
                              slice_bytes: int = 0, io_threads: int = 0, fix_survivors: bool = False) -> dict:
    """Rebuild the lost members of a host-resident RS set (0 < lost < e <= 4)
    and check the survivors against the spare parity rows
    (include/redset_hip.h redset_hip_rs_rebuild_checked_stream): one wrong
    survivor byte per column is located and kept out of the rebuilt bytes
    (e - k >= 2) and, with ``fix_survivors``, written back corrected. Returns
    the summary's fields (``corrected_bytes``, ``unlocated_columns``,
    ``stripes_with_findings``, ``cells_written``), ``corrected`` / ``first``
    [stripes of the call, p], ``unlocated`` / ``first_unlocated`` [stripes of
    the call] (see codec.RebuildCheckedPlan.report) and the statistics."""
    from .codec import repair_arrays

    r = sorted(lost)
    arr = (c_int * max(1, len(r)))(*r)
    n, p = (nstripes if nstripes > 0 else codec.ranks), codec.ranks
    st, summ = _lib.StreamStats(), _lib.RebuildCheckedSummary()
    cells = (_lib.RepairCell * max(1, n * p))()
    stripes = (_lib.RepairStripe * max(1, n))()
    _lib.check(_lib.load().redset_hip_rs_rebuild_checked_stream(
        codec._h, len(r), arr, chunk, first, nstripes, slice_bytes, io_threads, ctypes.byref(io.io),
        int(bool(fix_survivors)), ctypes.byref(st), cells, n * p, stripes, n, ctypes.byref(summ)),
        "rs_rebuild_checked_stream")
    corrected, first_off, unloc, first_unloc = repair_arrays(cells, stripes, n, p)
    out = summ.as_dict()
    out.update({"corrected": corrected, "first": first_off, "unlocated": unloc, "first_unlocated": first_unloc,
                "stats": st.as_dict()})
    return out


def crc32_stream(chunk: int, io, spans: Sequence[Tuple[int, int, int, int]], slice_bytes: int = 0,
                 io_threads: int = 0) -> dict:
    """zlib CRC-32 of every span ``(rank, kind, offset, length)`` of a
    host-resident set -- kind 0: bytes of the member's logical file, 1: bytes
    of its redundancy payload -- computed on the GPU (include/redset_hip.h
    redset_hip_crc32_stream). Reads only. Returns ``crcs`` and the pipeline
    statistics."""
    from ctypes import c_uint

    arr = (_lib.CrcSpan * max(1, len(spans)))()
    for i, (rank, kind, off, n) in enumerate(spans):
        arr[i] = _lib.CrcSpan(int(rank), int(kind), int(off), int(n))
    out = (c_uint * max(1, len(spans)))()
    st = _lib.StreamStats()
    _lib.check(_lib.load().redset_hip_crc32_stream(chunk, arr, len(spans), slice_bytes, io_threads,
                                                   ctypes.byref(io.io), ctypes.byref(st), out), "crc32_stream")
    return {"crcs": [int(x) for x in out[:len(spans)]], "stats": st.as_dict()}


def chunk_size_for(max_bytes: int, data_cells: int) -> int:
    """redset_apply_rs / redset_apply_xor chunk size: ceil(max / data cells),
    at least 1 (src/redset_reedsolomon.c:485-493, src/redset_xor.c:362-370)."""
    c = max_bytes // data_cells
    if c * data_cells < max_bytes:
        c += 1
    return max(1, c)
