"""Python face of the HIP codec, for tests, bench and the multi-GPU driver.

The codec itself is the C ABI in ``include/redset_hip.h`` (host C++ planner +
gfx950 kernels). This module only passes device pointers through ctypes;
PyTorch provides device memory and streams. Names follow redset's domain:
a *set* of ``ranks`` members, each with a logical file of data *cells* and a
redundancy region of parity cells; a *stripe* is the row of cells, one per
member, that one parity computation covers.
"""
from __future__ import annotations

import ctypes
from ctypes import c_int, c_ubyte, c_void_p
from dataclasses import dataclass
from typing import Optional, Sequence

import numpy as np

from . import _lib

CELL_ALIGN = 256  # cell_stride rounding in SetLayout (16 B is the kernel's minimum)


def _stream_handle(stream) -> Optional[int]:
    if stream is None:
        try:
            import torch

            if torch.cuda.is_available():
                return torch.cuda.current_stream().cuda_stream
        except Exception:  # pragma: no cover
            pass
        return None
    if isinstance(stream, int):
        return stream
    return stream.cuda_stream


def _ptr(x) -> int:
    return x if isinstance(x, int) else x.data_ptr()


class Plan:
    """Prepared kernel launches for one whole-set operation."""

    def __init__(self, handle: c_void_p, keepalive=()):
        self._h = handle
        self._keep = keepalive
        info = _lib.PlanInfo()
        _lib.check(_lib.load().redset_hip_plan_get_info(self._h, ctypes.byref(info)), "plan_get_info")
        self.info = info

    def execute(self, stream=None) -> None:
        _lib.check(_lib.load().redset_hip_plan_execute(self._h, _stream_handle(stream)), "plan_execute")

    @property
    def bytes_read(self) -> int:
        return int(self.info.bytes_read)

    @property
    def bytes_written(self) -> int:
        return int(self.info.bytes_written)

    @property
    def launches(self) -> int:
        """Kernel launches one execute() issues (one per stripe when the
        plan runs its jobs one after another)."""
        return int(self.info.launches)

    def close(self) -> None:
        if self._h:
            _lib.load().redset_hip_plan_destroy(self._h)
            self._h = None

    def __del__(self):  # pragma: no cover - finaliser
        try:
            self.close()
        except Exception:
            pass


NO_OFFSET = (1 << 64) - 1  # first_offset of a report row where nothing differs


def rows_to_arrays(rows, stripes: int, e: int):
    """(mismatch[stripes, e], first[stripes, e]) of a redset_hip_verify_row array."""
    mism = np.array([int(r.mismatch_bytes) for r in rows], dtype=np.uint64).reshape(stripes, e)
    first = np.array([int(r.first_offset) for r in rows], dtype=np.uint64).reshape(stripes, e)
    return mism, first


class VerifyPlan(Plan):
    """A verify (scrub) plan: execute() reads every cell of the set once and
    writes none; report() says which stored parity rows no longer match the
    stored data (include/redset_hip.h, "set verification")."""

    def report(self, stream=None):
        """``(mismatch, first)``: numpy uint64 arrays [p, e] -- differing bytes
        of stripe c's parity row i and the first differing cell offset
        (NO_OFFSET where nothing differs) -- of the last execute. Waits for
        the work on ``stream``."""
        p, e = int(self.info.ranks), int(self.info.encoding)
        rows = (_lib.VerifyRow * (p * e))()
        _lib.check(_lib.load().redset_hip_plan_verify_report(self._h, _stream_handle(stream), rows, p * e, None),
                   "plan_verify_report")
        return rows_to_arrays(rows, p, e)

    @property
    def clean(self) -> bool:
        """No byte of the last execute's report differs."""
        from ctypes import c_ulonglong

        total = c_ulonglong(0)
        _lib.check(_lib.load().redset_hip_plan_verify_report(self._h, _stream_handle(None), None, 0,
                                                             ctypes.byref(total)), "plan_verify_report")
        return total.value == 0

    def locate(self, stripe: int, stream=None):
        """``(member, offset)`` for ``stripe`` after an execute: the member
        whose single wrong byte explains the stripe's first differing column
        (-1: clean, or no single member explains it, or an XOR set) and that
        column's cell offset (None if the stripe is clean)."""
        from ctypes import c_ulonglong

        m, off = c_int(-1), c_ulonglong(0)
        _lib.check(_lib.load().redset_hip_plan_verify_locate(self._h, _stream_handle(stream), stripe,
                                                             ctypes.byref(m), ctypes.byref(off)),
                   "plan_verify_locate")
        return int(m.value), (None if off.value == NO_OFFSET else int(off.value))


def repair_arrays(cells, stripes, n: int, p: int):
    """(corrected[n, p], first[n, p], unlocated[n], first_unlocated[n]) of
    redset_hip_repair_cell / redset_hip_repair_stripe arrays."""
    corrected = np.array([int(c.corrected_bytes) for c in cells[:n * p]], dtype=np.uint64).reshape(n, p)
    first = np.array([int(c.first_offset) for c in cells[:n * p]], dtype=np.uint64).reshape(n, p)
    unloc = np.array([int(s.unlocated_columns) for s in stripes[:n]], dtype=np.uint64)
    first_unloc = np.array([int(s.first_unlocated) for s in stripes[:n]], dtype=np.uint64)
    return corrected, first, unloc, first_unloc


class RepairPlan(Plan):
    """A repair plan: execute() locates, for every byte column of the planned
    stripes, the one member whose wrong byte explains the syndrome and (made
    with apply=True) XORs that byte right; nothing else is written
    (include/redset_hip.h, "repair")."""

    def report(self, stream=None):
        """``(corrected, first, unlocated, first_unlocated)`` of the last
        execute: numpy uint64 arrays [n, p] -- corrected bytes of member m's
        cell of the k-th planned stripe and the smallest corrected cell offset
        (NO_OFFSET if none) -- and [n] -- byte columns no single member
        explains, and the first of them. n = the stripes planned (p when none
        were listed). Waits for the work on ``stream``."""
        n, p = int(self.info.jobs), int(self.info.ranks)
        cells = (_lib.RepairCell * max(1, n * p))()
        stripes = (_lib.RepairStripe * max(1, n))()
        _lib.check(_lib.load().redset_hip_plan_repair_report(self._h, _stream_handle(stream), cells, n * p,
                                                             stripes, n), "plan_repair_report")
        return repair_arrays(cells, stripes, n, p)


class RebuildCheckedPlan(Plan):
    """A checked rebuild plan: execute() rebuilds the lost members' cells
    and, per byte column, locates one wrong survivor byte from the parity
    rows the rebuild does not need and takes its error out of the rebuilt
    bytes (include/redset_hip.h, "checked rebuild")."""

    def report(self, stream=None):
        """``(corrected, first, unlocated, first_unlocated)`` of the last
        execute, shaped as RepairPlan.report with n = p: survivor bytes
        located as wrong per (stripe, member) and the smallest such cell
        offset, and per stripe the columns no single survivor explains.
        Waits for the work on ``stream``."""
        p = int(self.info.ranks)
        cells = (_lib.RepairCell * (p * p))()
        stripes = (_lib.RepairStripe * p)()
        _lib.check(_lib.load().redset_hip_plan_rebuild_checked_report(self._h, _stream_handle(stream), cells, p * p,
                                                                      stripes, p), "plan_rebuild_checked_report")
        return repair_arrays(cells, stripes, p, p)


class RSCodec:
    """GF(2^8) tables + encoding matrix for a set of ``ranks`` members with
    ``encoding`` parity cells per stripe (redset_construct_rs,
    src/redset_reedsolomon.c:80-188)."""

    def __init__(self, ranks: int, encoding: int):
        lib = _lib.load()
        h = c_void_p()
        _lib.check(lib.redset_hip_rs_create(ranks, encoding, ctypes.byref(h)), "rs_create")
        self._h = h
        self.ranks = ranks
        self.encoding = encoding

    @property
    def data_cells(self) -> int:
        return self.ranks - self.encoding

    def matrix(self) -> np.ndarray:
        p, e = self.ranks, self.encoding
        buf = (c_ubyte * ((p + e) * p))()
        _lib.check(_lib.load().redset_hip_rs_matrix(self._h, buf), "rs_matrix")
        return np.frombuffer(bytes(buf), dtype=np.uint8).reshape(p + e, p).copy()

    def decode_matrix(self, rebuild_ranks: Sequence[int], chunk_id: int) -> np.ndarray:
        m = len(rebuild_ranks)
        ranks = (c_int * m)(*sorted(rebuild_ranks))
        buf = (c_ubyte * (m * self.ranks))()
        _lib.check(
            _lib.load().redset_hip_rs_decode_matrix(self._h, m, ranks, chunk_id, buf), "rs_decode_matrix"
        )
        return np.frombuffer(bytes(buf), dtype=np.uint8).reshape(m, self.ranks).copy()

    def encoding_id(self, rank: int, chunk_id: int) -> int:
        return _lib.load().redset_hip_rs_get_encoding_id(self.ranks, self.encoding, rank, chunk_id)

    def data_id(self, rank: int, chunk_id: int) -> int:
        return _lib.load().redset_hip_rs_get_data_id(self.ranks, self.encoding, rank, chunk_id)

    def plan_encode(self, lofi, parity, chunk_size: int, cell_stride: Optional[int] = None) -> Plan:
        stride = chunk_size if cell_stride is None else cell_stride
        a, b = _lib.ptr_array([_ptr(x) for x in lofi]), _lib.ptr_array([_ptr(x) for x in parity])
        h = c_void_p()
        _lib.check(
            _lib.load().redset_hip_rs_plan_encode(self._h, a, b, chunk_size, stride, ctypes.byref(h)),
            "rs_plan_encode",
        )
        return Plan(h, (self, lofi, parity))

    def plan_rebuild(self, rebuild_ranks: Sequence[int], lofi, parity, chunk_size: int,
                     cell_stride: Optional[int] = None) -> Plan:
        stride = chunk_size if cell_stride is None else cell_stride
        ranks = sorted(rebuild_ranks)
        r = (c_int * max(1, len(ranks)))(*ranks)
        a, b = _lib.ptr_array([_ptr(x) for x in lofi]), _lib.ptr_array([_ptr(x) for x in parity])
        h = c_void_p()
        _lib.check(
            _lib.load().redset_hip_rs_plan_rebuild(
                self._h, len(ranks), r, a, b, chunk_size, stride, ctypes.byref(h)
            ),
            "rs_plan_rebuild",
        )
        return Plan(h, (self, lofi, parity))

    def plan_verify(self, lofi, parity, chunk_size: int, cell_stride: Optional[int] = None) -> "VerifyPlan":
        """Check every stripe's stored parity against its stored data."""
        stride = chunk_size if cell_stride is None else cell_stride
        a, b = _lib.ptr_array([_ptr(x) for x in lofi]), _lib.ptr_array([_ptr(x) for x in parity])
        h = c_void_p()
        _lib.check(
            _lib.load().redset_hip_rs_plan_verify(self._h, a, b, chunk_size, stride, ctypes.byref(h)),
            "rs_plan_verify",
        )
        return VerifyPlan(h, (self, lofi, parity))

    def plan_repair(self, lofi, parity, chunk_size: int, cell_stride: Optional[int] = None,
                    stripes: Optional[Sequence[int]] = None, apply: bool = True) -> "RepairPlan":
        """Correct, in the listed stripes (default: all), every byte column
        with one wrong byte; ``apply=False`` only reports. 2 <= e <= 4."""
        stride = chunk_size if cell_stride is None else cell_stride
        a, b = _lib.ptr_array([_ptr(x) for x in lofi]), _lib.ptr_array([_ptr(x) for x in parity])
        n = 0 if stripes is None else len(stripes)
        arr = None if stripes is None else (c_int * max(1, n))(*[int(c) for c in stripes])
        h = c_void_p()
        _lib.check(
            _lib.load().redset_hip_rs_plan_repair(self._h, a, b, chunk_size, stride, n, arr, int(bool(apply)),
                                                  ctypes.byref(h)),
            "rs_plan_repair",
        )
        return RepairPlan(h, (self, lofi, parity))

    def plan_rebuild_checked(self, rebuild_ranks: Sequence[int], lofi, parity, chunk_size: int,
                             cell_stride: Optional[int] = None, fix_survivors: bool = False) -> "RebuildCheckedPlan":
        """Rebuild the lost members and check the survivors against the spare
        parity rows: 0 < len(rebuild_ranks) < e <= 4. ``fix_survivors`` also
        corrects the located survivor bytes in place."""
        stride = chunk_size if cell_stride is None else cell_stride
        ranks = sorted(rebuild_ranks)
        r = (c_int * max(1, len(ranks)))(*ranks)
        a, b = _lib.ptr_array([_ptr(x) for x in lofi]), _lib.ptr_array([_ptr(x) for x in parity])
        h = c_void_p()
        _lib.check(
            _lib.load().redset_hip_rs_plan_rebuild_checked(self._h, len(ranks), r, a, b, chunk_size, stride,
                                                           int(bool(fix_survivors)), ctypes.byref(h)),
            "rs_plan_rebuild_checked",
        )
        return RebuildCheckedPlan(h, (self, lofi, parity))

    def check_matrix(self, rebuild_ranks: Sequence[int], chunk_id: int):
        """``(M, lost_cols)`` of stripe chunk_id with these members lost: M is
        [e, d + e] uint8 -- e - k check rows (zero on the lost columns), then
        k rebuild rows (identity on them) -- over the stripe's cells (column
        i < d: data input i, column d + j: parity row j); lost_cols[i] is the
        column of sorted(rebuild_ranks)[i] (include/redset_hip.h
        redset_hip_rs_check_matrix)."""
        ranks = sorted(rebuild_ranks)
        k, e, n = len(ranks), self.encoding, self.ranks
        r = (c_int * max(1, k))(*ranks)
        buf = (c_ubyte * (e * n))()
        cols = (c_int * max(1, k))()
        _lib.check(_lib.load().redset_hip_rs_check_matrix(self._h, k, r, chunk_id, buf, cols), "rs_check_matrix")
        return np.frombuffer(bytes(buf), dtype=np.uint8).reshape(e, n).copy(), [int(c) for c in cols[:k]]

    def locate_reduced(self, rebuild_ranks: Sequence[int], chunk_id: int, reduced_syndrome):
        """``(member, value)``: the one surviving member whose single wrong
        byte gives this reduced syndrome (e - k bytes: the check rows of
        check_matrix applied to the survivors' bytes of one column) and that
        byte's error, or (-1, 0) (include/redset_hip.h
        redset_hip_rs_locate_reduced)."""
        ranks = sorted(rebuild_ranks)
        r = (c_int * max(1, len(ranks)))(*ranks)
        syn = (c_ubyte * max(1, len(reduced_syndrome)))(*[int(x) for x in reduced_syndrome])
        m, x = c_int(-1), c_ubyte(0)
        _lib.check(_lib.load().redset_hip_rs_locate_reduced(self._h, len(ranks), r, chunk_id, syn, ctypes.byref(m),
                                                            ctypes.byref(x)), "rs_locate_reduced")
        return int(m.value), int(x.value)

    def locate_syndrome(self, chunk_id: int, syndrome) -> int:
        """The member whose single wrong byte gives this syndrome column (e
        bytes: stored parity ^ parity of stored data) in stripe chunk_id, or
        -1 (include/redset_hip.h redset_hip_rs_locate_syndrome)."""
        syn = (c_ubyte * self.encoding)(*[int(x) for x in syndrome])
        m = c_int(-1)
        _lib.check(_lib.load().redset_hip_rs_locate_syndrome(self._h, chunk_id, syn, ctypes.byref(m)),
                   "rs_locate_syndrome")
        return int(m.value)

    def close(self) -> None:
        if self._h:
            _lib.load().redset_hip_rs_destroy(self._h)
            self._h = None

    def __del__(self):  # pragma: no cover
        try:
            self.close()
        except Exception:
            pass


def xor_plan_encode(ranks: int, lofi, xorc, chunk_size: int, cell_stride: Optional[int] = None) -> Plan:
    stride = chunk_size if cell_stride is None else cell_stride
    a, b = _lib.ptr_array([_ptr(x) for x in lofi]), _lib.ptr_array([_ptr(x) for x in xorc])
    h = c_void_p()
    _lib.check(
        _lib.load().redset_hip_xor_plan_encode(ranks, a, b, chunk_size, stride, ctypes.byref(h)),
        "xor_plan_encode",
    )
    return Plan(h, (lofi, xorc))


def xor_plan_rebuild(ranks: int, root: int, lofi, xorc, chunk_size: int,
                     cell_stride: Optional[int] = None) -> Plan:
    stride = chunk_size if cell_stride is None else cell_stride
    a, b = _lib.ptr_array([_ptr(x) for x in lofi]), _lib.ptr_array([_ptr(x) for x in xorc])
    h = c_void_p()
    _lib.check(
        _lib.load().redset_hip_xor_plan_rebuild(ranks, root, a, b, chunk_size, stride, ctypes.byref(h)),
        "xor_plan_rebuild",
    )
    return Plan(h, (lofi, xorc))


def xor_plan_verify(ranks: int, lofi, xorc, chunk_size: int, cell_stride: Optional[int] = None) -> VerifyPlan:
    """Check that the XOR of every stripe's p cells is zero."""
    stride = chunk_size if cell_stride is None else cell_stride
    a, b = _lib.ptr_array([_ptr(x) for x in lofi]), _lib.ptr_array([_ptr(x) for x in xorc])
    h = c_void_p()
    _lib.check(
        _lib.load().redset_hip_xor_plan_verify(ranks, a, b, chunk_size, stride, ctypes.byref(h)),
        "xor_plan_verify",
    )
    return VerifyPlan(h, (lofi, xorc))


def xor_plan_repair(ranks: int, lofi, xorc, chunk_size: int, cell_stride: Optional[int] = None, stripes=None,
                    apply: bool = True):
    """There is none: an XOR stripe has one parity row, which says that a
    column is wrong and not which cell. Always raises; the tool for an XOR
    set is a rebuild of the member its checksum sidecar names."""
    raise _lib.RedsetHipError("xor_plan_repair: one parity row locates nothing; rebuild the member that the "
                              "checksum sidecar names (verify_set(checksums=True), rebuild_set)")


def gf_combine(inputs, outputs, coeffs: np.ndarray, nbytes: int, accumulate: bool = False, stream=None) -> None:
    """outputs[j] (^)= sum_i coeffs[j, i] * inputs[i] over GF(2^8) (device buffers)."""
    coeffs = np.ascontiguousarray(coeffs, dtype=np.uint8)
    nout, nin = coeffs.shape
    assert len(inputs) == nin and len(outputs) == nout
    c = (c_ubyte * coeffs.size).from_buffer_copy(coeffs.tobytes())
    _lib.check(
        _lib.load().redset_hip_gf_combine(
            _lib.ptr_array([_ptr(x) for x in inputs]), nin,
            _lib.ptr_array([_ptr(x) for x in outputs]), nout,
            c, nbytes, int(accumulate), _stream_handle(stream),
        ),
        "gf_combine",
    )


def xor_combine(inputs, output, nbytes: int, accumulate: bool = False, stream=None) -> None:
    _lib.check(
        _lib.load().redset_hip_xor_combine(
            _lib.ptr_array([_ptr(x) for x in inputs]), len(inputs), _ptr(output), nbytes,
            int(accumulate), _stream_handle(stream),
        ),
        "xor_combine",
    )


@dataclass
class SetLayout:
    """Device-resident layout of one redundancy set (see include/redset_hip.h).

    Member r's logical file = ``data_cells`` cells and its redundancy region =
    ``parity_cells`` cells, every cell ``cell_stride`` bytes apart (chunk_size
    rounded up to CELL_ALIGN). One allocation holds the whole set.
    """

    ranks: int
    data_cells: int
    parity_cells: int
    chunk_size: int
    cell_stride: int
    storage: object  # torch.uint8 tensor

    @classmethod
    def allocate(cls, ranks: int, data_cells: int, parity_cells: int, chunk_size: int, device="cuda",
                 pad: int = 0):
        """``pad`` extra bytes after every cell (rounded to CELL_ALIGN): moves
        the cells of a stripe relative to each other in HBM."""
        import torch

        stride = max(CELL_ALIGN, -(-chunk_size // CELL_ALIGN) * CELL_ALIGN)
        stride += -(-pad // CELL_ALIGN) * CELL_ALIGN
        per = (data_cells + parity_cells) * stride
        storage = torch.empty(ranks * per, dtype=torch.uint8, device=device)
        return cls(ranks, data_cells, parity_cells, chunk_size, stride, storage)

    @property
    def member_bytes(self) -> int:
        return (self.data_cells + self.parity_cells) * self.cell_stride

    def lofi(self, r: int):
        base = r * self.member_bytes
        return self.storage[base: base + self.data_cells * self.cell_stride]

    def parity(self, r: int):
        base = r * self.member_bytes + self.data_cells * self.cell_stride
        return self.storage[base: base + self.parity_cells * self.cell_stride]

    def data_cell(self, r: int, s: int):
        return self.lofi(r)[s * self.cell_stride: s * self.cell_stride + self.chunk_size]

    def parity_cell(self, r: int, i: int):
        return self.parity(r)[i * self.cell_stride: i * self.cell_stride + self.chunk_size]

    def lofi_ptrs(self):
        return [self.lofi(r).data_ptr() for r in range(self.ranks)]

    def parity_ptrs(self):
        return [self.parity(r).data_ptr() for r in range(self.ranks)]


def cell_stride(chunk_size: int) -> int:
    """The library's recommended cell stride for a set held in one
    allocation (include/redset_hip.h redset_hip_cell_stride)."""
    return int(_lib.load().redset_hip_cell_stride(chunk_size))


def ring_faults(clear: bool = True) -> int:
    """Capped loader-ring handshake spins on the current device since the
    last clearing read (include/redset_hip.h redset_hip_ring_faults). Outputs
    are correct either way -- a capped spin falls back to direct HBM loads --
    so this is a stall counter: 0 means every launch's ring handshake
    completed in time. Synchronises the device."""
    from ctypes import c_uint

    n = c_uint(0)
    _lib.check(_lib.load().redset_hip_ring_faults(ctypes.byref(n), int(clear)), "ring_faults")
    return int(n.value)


def hang_faults(clear: bool = True, stream=None) -> int:
    """Capped HANG waits on the current device since the last clearing read
    (include/redset_hip.h redset_hip_hang_faults): waits with no fallback
    that gave up, so some launch's outputs are wrong. 0 on every healthy
    run. Read in order on `stream` (default: the library's own stream, after
    nothing -- synchronise the work to be counted first)."""
    from ctypes import c_uint

    n = c_uint(0)
    h = None if stream is None else _stream_handle(stream)
    _lib.check(_lib.load().redset_hip_hang_faults(h, ctypes.byref(n), int(clear)), "hang_faults")
    return int(n.value)
