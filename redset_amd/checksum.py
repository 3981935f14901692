"""Member checksums: zlib's CRC-32 of byte ranges in device memory, computed by
the HIP CRC kernels (include/redset_hip.h, "member checksums")."""
from __future__ import annotations

import ctypes
from ctypes import c_uint, c_void_p
from typing import List, Sequence, Tuple

from . import _lib
from .codec import _ptr, _stream_handle


def crc32_combine(crc_a: int, crc_b: int, len_b: int) -> int:
    """CRC-32 of A || B from crc(A), crc(B) and len(B) (zlib's crc32_combine)."""
    return int(_lib.load().redset_hip_crc32_combine(crc_a & 0xFFFFFFFF, crc_b & 0xFFFFFFFF, len_b))


class Crc32Plan:
    """One CRC-32 per range ``(pointer or tensor, length)`` of device memory.
    execute() only enqueues kernels and recomputes from the bytes then in
    memory; report() waits and returns the CRCs of the last execute."""

    def __init__(self, ranges: Sequence[Tuple[object, int]], keepalive=()):
        ranges = list(ranges)
        arr = (_lib.CrcRange * max(1, len(ranges)))()
        for i, (p, n) in enumerate(ranges):
            arr[i].ptr = None if p is None else _ptr(p)
            arr[i].len = int(n)
        h = c_void_p()
        _lib.check(_lib.load().redset_hip_plan_crc32(arr, len(ranges), ctypes.byref(h)), "plan_crc32")
        self._h = h
        self._keep = (ranges, keepalive)
        self.nranges = len(ranges)

    def execute(self, stream=None) -> None:
        _lib.check(_lib.load().redset_hip_plan_execute(self._h, _stream_handle(stream)), "plan_execute")

    def report(self, stream=None) -> List[int]:
        out = (c_uint * self.nranges)()
        _lib.check(_lib.load().redset_hip_plan_crc32_report(self._h, _stream_handle(stream), out, self.nranges),
                   "plan_crc32_report")
        return [int(x) for x in out]

    def info(self) -> dict:
        """Plan info (include/redset_hip.h redset_hip_plan_info) as a dict."""
        info = _lib.PlanInfo()
        _lib.check(_lib.load().redset_hip_plan_get_info(self._h, ctypes.byref(info)), "plan_get_info")
        return {k: int(getattr(info, k)) for k, _ in info._fields_}

    def close(self) -> None:
        if self._h:
            _lib.load().redset_hip_plan_destroy(self._h)
            self._h = None

    def __del__(self):  # pragma: no cover - finaliser
        try:
            self.close()
        except Exception:
            pass
