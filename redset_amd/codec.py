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


class VerifyCrcPlan(VerifyPlan):
    """A verify plan that checksums what it scrubs: execute() reads every
    cell of the set once, writes none, leaves VerifyPlan's report and the
    zlib CRC-32 of every cell as stored (include/redset_hip.h, "scrub and
    checksum in one read")."""

    def crcs(self, stream=None) -> np.ndarray:
        """The CRCs of the last execute: a ``(p, p)`` uint32 array indexed
        ``[member, cell]`` -- the member's data cells in logical-file order,
        then its parity slots. Waits for the work on ``stream``."""
        p = int(self.info.ranks)
        crcs = (ctypes.c_uint * (p * p))()
        _lib.check(_lib.load().redset_hip_plan_verify_crc32_report(self._h, _stream_handle(stream), crcs, p * p),
                   "plan_verify_crc32_report")
        return np.array(crcs[:], dtype=np.uint32).reshape(p, p)


def check_max_errors(max_errors: int, encoding: int) -> None:
    """The correction levels of repair: 1, or 2 on sets with four parity rows."""
    if max_errors not in (1, 2):
        raise ValueError(f"max_errors={max_errors}: repair corrects 1 or 2 wrong bytes per column")
    if max_errors == 2 and encoding != 4:
        raise ValueError(f"max_errors=2 on a set with {encoding} parity rows: two wrong bytes per column need "
                         "distance 5, that is e = 4")


def wide_max_errors(max_errors: Optional[int], encoding: int) -> int:
    """The correction levels of the wide repair (5 <= e <= 8): 1 .. e // 2,
    None meaning e // 2."""
    if not 5 <= encoding <= 8:
        raise ValueError(f"wide repair on a set with {encoding} parity rows: it is built for 5..8")
    t = encoding // 2
    if max_errors is None:
        return t
    if not 1 <= max_errors <= t:
        raise ValueError(f"max_errors={max_errors}: {encoding} parity rows correct 1..{t} wrong bytes per column")
    return int(max_errors)


def checked_wide_max_errors(max_errors: Optional[int], encoding: int, lost: int) -> int:
    """The correction levels of the wide checked rebuild (5 <= e <= 8, s =
    e - lost spare rows): 1 .. s // 2 (0 where s == 1), None meaning s // 2."""
    if not 5 <= encoding <= 8:
        raise ValueError(f"wide checked rebuild on a set with {encoding} parity rows: it is built for 5..8")
    if not 0 < lost < encoding:
        raise ValueError(f"wide checked rebuild of {lost} lost members: {encoding} parity rows take 1..{encoding - 1}")
    t = (encoding - lost) // 2
    if max_errors is None:
        return t
    if not min(1, t) <= max_errors <= t:
        raise ValueError(f"max_errors={max_errors}: {encoding - lost} spare rows locate {min(1, t)}..{t} wrong bytes "
                         "per column")
    return int(max_errors)


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


class Repair2Plan(Plan):
    """A repair plan made with ``max_errors=2`` (RS sets with e = 4): columns
    with two wrong bytes are corrected as well (include/redset_hip.h,
    "repair2")."""

    def report(self, stream=None):
        """RepairPlan.report's four arrays -- both members of a pair are
        counted -- and ``pair_columns`` [n]: the columns of each planned
        stripe corrected as a pair. Waits for the work on ``stream``."""
        n, p = int(self.info.jobs), int(self.info.ranks)
        cells = (_lib.RepairCell * max(1, n * p))()
        stripes = (_lib.RepairStripe * max(1, n))()
        pairs = (ctypes.c_ulonglong * max(1, n))()
        _lib.check(_lib.load().redset_hip_plan_repair2_report(self._h, _stream_handle(stream), cells, n * p,
                                                              stripes, n, pairs), "plan_repair2_report")
        return repair_arrays(cells, stripes, n, p) + (np.array(pairs[:n], dtype=np.uint64),)


class RepairWidePlan(Plan):
    """A wide repair plan (RS sets with 5 <= e <= 8): columns with up to
    ``max_errors`` <= e // 2 wrong bytes are corrected (include/redset_hip.h,
    "repair_wide")."""

    def report(self, stream=None):
        """RepairPlan.report's four arrays -- every byte of a correction is
        counted -- and ``multi_columns`` [n, 3]: the columns of each planned
        stripe corrected with 2, 3 and 4 wrong bytes. Waits for the work on
        ``stream``."""
        n, p = int(self.info.jobs), int(self.info.ranks)
        cells = (_lib.RepairCell * max(1, n * p))()
        stripes = (_lib.RepairStripe * max(1, n))()
        multi = (ctypes.c_ulonglong * max(1, 3 * n))()
        _lib.check(_lib.load().redset_hip_plan_repair_wide_report(self._h, _stream_handle(stream), cells, n * p,
                                                                  stripes, n, multi), "plan_repair_wide_report")
        return repair_arrays(cells, stripes, n, p) + (np.array(multi[:3 * n], dtype=np.uint64).reshape(n, 3),)


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


class RebuildCheckedWidePlan(Plan):
    """A wide checked rebuild plan (RS sets with 5 <= e <= 8): per byte
    column up to ``max_errors`` <= (e - k) // 2 wrong survivor bytes are
    located and taken out of the rebuilt bytes (include/redset_hip.h,
    "checked rebuild, wide")."""

    def report(self, stream=None):
        """RebuildCheckedPlan.report's four arrays -- every byte of a
        correction is counted -- and ``multi_columns`` [p, 2]: the columns of
        each stripe corrected with 2 and 3 wrong survivor bytes. Waits for the
        work on ``stream``."""
        p = int(self.info.ranks)
        cells = (_lib.RepairCell * (p * p))()
        stripes = (_lib.RepairStripe * p)()
        multi = (ctypes.c_ulonglong * (2 * p))()
        _lib.check(_lib.load().redset_hip_plan_rebuild_checked_wide_report(
            self._h, _stream_handle(stream), cells, p * p, stripes, p, multi), "plan_rebuild_checked_wide_report")
        return repair_arrays(cells, stripes, p, p) + (np.array(multi[:2 * p], dtype=np.uint64).reshape(p, 2),)


class EncodeCrcPlan(Plan):
    """An encode plan that checksums what it encodes: execute() reads every
    data cell once, stores the parity cells of the plain encode plan and
    leaves the zlib CRC-32 of every cell of the set (include/redset_hip.h,
    "encode and checksum in one read")."""

    def report(self, stream=None) -> np.ndarray:
        """The CRCs of the last execute: a ``(p, p)`` uint32 array indexed
        ``[member, cell]`` -- the member's data cells in logical-file order,
        then its parity slots. Waits for the work on ``stream``."""
        p = int(self.info.ranks)
        crcs = (ctypes.c_uint * (p * p))()
        _lib.check(_lib.load().redset_hip_plan_encode_crc32_report(self._h, _stream_handle(stream), crcs, p * p),
                   "plan_encode_crc32_report")
        return np.array(crcs[:], dtype=np.uint32).reshape(p, p)


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

    def plan_encode_crc32(self, lofi, parity, chunk_size: int,
                          cell_stride: Optional[int] = None) -> "EncodeCrcPlan":
        """plan_encode that also checksums every cell in the same read:
        p - e <= 16 data cells and e <= 4 parity cells a stripe, pointers and
        stride 16-B aligned (anything else is refused, never run another way)."""
        stride = chunk_size if cell_stride is None else cell_stride
        a, b = _lib.ptr_array([_ptr(x) for x in lofi]), _lib.ptr_array([_ptr(x) for x in parity])
        h = c_void_p()
        _lib.check(
            _lib.load().redset_hip_rs_plan_encode_crc32(self._h, a, b, chunk_size, stride, ctypes.byref(h)),
            "rs_plan_encode_crc32",
        )
        return EncodeCrcPlan(h, (self, lofi, parity))

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

    def plan_verify_crc32(self, lofi, parity, chunk_size: int,
                          cell_stride: Optional[int] = None) -> "VerifyCrcPlan":
        """plan_verify that also checksums every cell in the same read:
        p - e <= 16 data cells and e <= 4 parity cells a stripe, pointers and
        stride 16-B aligned (anything else is refused, never run another way)."""
        stride = chunk_size if cell_stride is None else cell_stride
        a, b = _lib.ptr_array([_ptr(x) for x in lofi]), _lib.ptr_array([_ptr(x) for x in parity])
        h = c_void_p()
        _lib.check(
            _lib.load().redset_hip_rs_plan_verify_crc32(self._h, a, b, chunk_size, stride, ctypes.byref(h)),
            "rs_plan_verify_crc32",
        )
        return VerifyCrcPlan(h, (self, lofi, parity))

    def plan_repair(self, lofi, parity, chunk_size: int, cell_stride: Optional[int] = None,
                    stripes: Optional[Sequence[int]] = None, apply: bool = True, max_errors: int = 1):
        """Correct, in the listed stripes (default: all), every byte column
        with one wrong byte; ``apply=False`` only reports. 2 <= e <= 4.
        ``max_errors=2`` (e = 4 only, else ValueError) also corrects columns
        with two wrong bytes and returns a Repair2Plan."""
        check_max_errors(max_errors, self.encoding)
        stride = chunk_size if cell_stride is None else cell_stride
        a, b = _lib.ptr_array([_ptr(x) for x in lofi]), _lib.ptr_array([_ptr(x) for x in parity])
        n = 0 if stripes is None else len(stripes)
        arr = None if stripes is None else (c_int * max(1, n))(*[int(c) for c in stripes])
        h = c_void_p()
        if max_errors == 2:
            _lib.check(
                _lib.load().redset_hip_rs_plan_repair2(self._h, a, b, chunk_size, stride, n, arr, int(bool(apply)),
                                                       ctypes.byref(h)),
                "rs_plan_repair2",
            )
            return Repair2Plan(h, (self, lofi, parity))
        _lib.check(
            _lib.load().redset_hip_rs_plan_repair(self._h, a, b, chunk_size, stride, n, arr, int(bool(apply)),
                                                  ctypes.byref(h)),
            "rs_plan_repair",
        )
        return RepairPlan(h, (self, lofi, parity))

    def plan_repair_wide(self, lofi, parity, chunk_size: int, cell_stride: Optional[int] = None,
                         stripes: Optional[Sequence[int]] = None, apply: bool = True,
                         max_errors: Optional[int] = None) -> "RepairWidePlan":
        """plan_repair for sets with 5 <= e <= 8: every byte column with up
        to ``max_errors`` wrong bytes (1 .. e // 2; None: e // 2) is
        corrected. Other e, or max_errors out of range: ValueError."""
        max_errors = wide_max_errors(max_errors, self.encoding)
        stride = chunk_size if cell_stride is None else cell_stride
        a, b = _lib.ptr_array([_ptr(x) for x in lofi]), _lib.ptr_array([_ptr(x) for x in parity])
        n = 0 if stripes is None else len(stripes)
        arr = None if stripes is None else (c_int * max(1, n))(*[int(c) for c in stripes])
        h = c_void_p()
        _lib.check(
            _lib.load().redset_hip_rs_plan_repair_wide(self._h, a, b, chunk_size, stride, n, arr, int(bool(apply)),
                                                       max_errors, ctypes.byref(h)),
            "rs_plan_repair_wide",
        )
        return RepairWidePlan(h, (self, lofi, parity))

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

    def plan_rebuild_checked_wide(self, rebuild_ranks: Sequence[int], lofi, parity, chunk_size: int,
                                  cell_stride: Optional[int] = None, fix_survivors: bool = False,
                                  max_errors: Optional[int] = None) -> "RebuildCheckedWidePlan":
        """plan_rebuild_checked for sets with 5 <= e <= 8 and 0 <
        len(rebuild_ranks) < e: per byte column up to ``max_errors`` wrong
        survivor bytes (1 .. (e - k) // 2; None: (e - k) // 2) are located,
        taken out of the rebuilt bytes and, with ``fix_survivors``, corrected
        in place. Other e, or max_errors out of range: ValueError."""
        ranks = sorted(rebuild_ranks)
        max_errors = checked_wide_max_errors(max_errors, self.encoding, len(ranks))
        stride = chunk_size if cell_stride is None else cell_stride
        r = (c_int * max(1, len(ranks)))(*ranks)
        a, b = _lib.ptr_array([_ptr(x) for x in lofi]), _lib.ptr_array([_ptr(x) for x in parity])
        h = c_void_p()
        _lib.check(
            _lib.load().redset_hip_rs_plan_rebuild_checked_wide(self._h, len(ranks), r, a, b, chunk_size, stride,
                                                                int(bool(fix_survivors)), max_errors,
                                                                ctypes.byref(h)),
            "rs_plan_rebuild_checked_wide",
        )
        return RebuildCheckedWidePlan(h, (self, lofi, parity))

    def check_basis_wide(self, rebuild_ranks: Sequence[int], chunk_id: int):
        """``(alpha, uprime, M, lost_cols)`` of stripe chunk_id with these
        members lost (ranks as given: the library refuses unsorted ones): M
        is [e, d + e] -- e - k check rows u'_i * alpha_i^j, zero on the lost
        columns, then the k rebuild rows (include/redset_hip.h
        redset_hip_rs_check_basis_wide)."""
        k, e, n = len(rebuild_ranks), self.encoding, self.ranks
        r = (c_int * max(1, k))(*[int(x) for x in rebuild_ranks])
        alpha, up, buf, cols = (c_ubyte * n)(), (c_ubyte * n)(), (c_ubyte * (e * n))(), (c_int * max(1, k))()
        _lib.check(_lib.load().redset_hip_rs_check_basis_wide(self._h, k, r, chunk_id, alpha, up, buf, cols),
                   "rs_check_basis_wide")
        as_np = lambda b: np.frombuffer(bytes(b), dtype=np.uint8).copy()  # noqa: E731
        return as_np(alpha), as_np(up), as_np(buf).reshape(e, n), [int(cols[i]) for i in range(k)]

    def locate_reduced_wide(self, rebuild_ranks: Sequence[int], chunk_id: int, reduced,
                            max_errors: Optional[int] = None):
        """``[(member, value), ...]``: the up to ``max_errors`` (None:
        (e - k) // 2) surviving members, ascending, whose wrong bytes give
        these e - k modified sums, with the error values; empty when clean or
        unlocated (include/redset_hip.h redset_hip_rs_locate_reduced_wide)."""
        ranks = sorted(rebuild_ranks)
        r = (c_int * max(1, len(ranks)))(*ranks)
        t = (self.encoding - len(ranks)) // 2
        syn = (c_ubyte * 8)(*[int(x) for x in reduced])
        mem, val, n = (c_int * 3)(), (c_ubyte * 3)(), c_int(0)
        _lib.check(_lib.load().redset_hip_rs_locate_reduced_wide(
            self._h, len(ranks), r, chunk_id, syn, t if max_errors is None else int(max_errors), mem, val,
            ctypes.byref(n)), "rs_locate_reduced_wide")
        return [(int(mem[i]), int(val[i])) for i in range(n.value)]

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

    def power_basis(self, chunk_id: int):
        """``(alpha, u, winv)`` of stripe chunk_id (e = 4): the evaluation
        point and dual multiplier of its d + e cells (data inputs, then parity
        rows) and the [e, e] transform with winv @ H[:, i] = u[i] * alpha[i]^t
        (include/redset_hip.h redset_hip_rs_power_basis)."""
        n, e = self.ranks, self.encoding
        alpha, u, winv = (c_ubyte * n)(), (c_ubyte * n)(), (c_ubyte * (e * e))()
        _lib.check(_lib.load().redset_hip_rs_power_basis(self._h, chunk_id, alpha, u, winv), "rs_power_basis")
        as_np = lambda b: np.frombuffer(bytes(b), dtype=np.uint8).copy()  # noqa: E731
        return as_np(alpha), as_np(u), as_np(winv).reshape(e, e)

    def locate_syndrome2(self, chunk_id: int, syndrome):
        """``[(member, value), ...]``: the one or two members, ascending,
        whose wrong bytes give this syndrome column in stripe chunk_id, with
        the error values; empty when clean or unlocated (e = 4;
        include/redset_hip.h redset_hip_rs_locate_syndrome2)."""
        syn = (c_ubyte * max(4, self.encoding))(*[int(x) for x in syndrome])
        mem, val, n = (c_int * 2)(), (c_ubyte * 2)(), c_int(0)
        _lib.check(_lib.load().redset_hip_rs_locate_syndrome2(self._h, chunk_id, syn, mem, val, ctypes.byref(n)),
                   "rs_locate_syndrome2")
        return [(int(mem[i]), int(val[i])) for i in range(n.value)]

    def power_basis_wide(self, chunk_id: int):
        """power_basis for 5 <= e <= 8: ``(alpha, u, winv)`` with
        winv @ H[:, i] = u[i] * alpha[i]^k, k = 0 .. e - 1
        (include/redset_hip.h redset_hip_rs_power_basis_wide)."""
        n, e = self.ranks, self.encoding
        alpha, u, winv = (c_ubyte * n)(), (c_ubyte * n)(), (c_ubyte * (e * e))()
        _lib.check(_lib.load().redset_hip_rs_power_basis_wide(self._h, chunk_id, alpha, u, winv), "rs_power_basis_wide")
        as_np = lambda b: np.frombuffer(bytes(b), dtype=np.uint8).copy()  # noqa: E731
        return as_np(alpha), as_np(u), as_np(winv).reshape(e, e)

    def locate_syndrome_wide(self, chunk_id: int, syndrome, max_errors: Optional[int] = None):
        """``[(member, value), ...]``: the up to ``max_errors`` (None: e // 2)
        members, ascending, whose wrong bytes give this syndrome column in
        stripe chunk_id, with the error values; empty when clean or unlocated
        (5 <= e <= 8; include/redset_hip.h redset_hip_rs_locate_syndrome_wide)."""
        e = self.encoding
        t = max(1, e // 2)
        syn = (c_ubyte * max(8, e))(*[int(x) for x in syndrome])
        mem, val, n = (c_int * t)(), (c_ubyte * t)(), c_int(0)
        _lib.check(_lib.load().redset_hip_rs_locate_syndrome_wide(
            self._h, chunk_id, syn, t if max_errors is None else int(max_errors), mem, val, ctypes.byref(n)),
            "rs_locate_syndrome_wide")
        return [(int(mem[i]), int(val[i])) for i in range(n.value)]

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


def xor_plan_encode_crc32(ranks: int, lofi, xorc, chunk_size: int,
                          cell_stride: Optional[int] = None) -> EncodeCrcPlan:
    """xor_plan_encode that also checksums every cell in the same read
    (ranks - 1 <= 16; pointers and stride 16-B aligned)."""
    stride = chunk_size if cell_stride is None else cell_stride
    a, b = _lib.ptr_array([_ptr(x) for x in lofi]), _lib.ptr_array([_ptr(x) for x in xorc])
    h = c_void_p()
    _lib.check(
        _lib.load().redset_hip_xor_plan_encode_crc32(ranks, a, b, chunk_size, stride, ctypes.byref(h)),
        "xor_plan_encode_crc32",
    )
    return EncodeCrcPlan(h, (lofi, xorc))


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


def xor_plan_verify_crc32(ranks: int, lofi, xorc, chunk_size: int,
                          cell_stride: Optional[int] = None) -> VerifyCrcPlan:
    """xor_plan_verify that also checksums every cell in the same read
    (ranks - 1 <= 16; pointers and stride 16-B aligned)."""
    stride = chunk_size if cell_stride is None else cell_stride
    a, b = _lib.ptr_array([_ptr(x) for x in lofi]), _lib.ptr_array([_ptr(x) for x in xorc])
    h = c_void_p()
    _lib.check(
        _lib.load().redset_hip_xor_plan_verify_crc32(ranks, a, b, chunk_size, stride, ctypes.byref(h)),
        "xor_plan_verify_crc32",
    )
    return VerifyCrcPlan(h, (lofi, xorc))


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
