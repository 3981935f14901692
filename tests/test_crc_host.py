"""CPU tests of the member checksums' host side (include/redset_hip.h, "member
checksums"): redset_hip_crc32_combine against zlib.crc32, and the argument
checks of the CRC plan, its report and the streaming call. No kernel runs."""
import zlib
from ctypes import byref, c_uint, c_void_p

import numpy as np
import pytest


@pytest.fixture(scope="module")
def hiplib():
    import os

    import redset_amd
    from redset_amd import _lib

    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__

        __graft_entry__.build_library()
    return redset_amd


def zeros_crc(hiplib, n, memo=None):
    """zlib's CRC of n zero bytes without holding them: halves combined
    (the two halves differ by at most one byte, so few lengths recur)."""
    memo = {} if memo is None else memo
    if n <= 4096:
        return zlib.crc32(bytes(n))
    if n not in memo:
        h = n // 2
        memo[n] = hiplib.crc32_combine(zeros_crc(hiplib, h, memo), zeros_crc(hiplib, n - h, memo), n - h)
    return memo[n]


def test_known_vector(hiplib):
    assert zlib.crc32(b"123456789") == 0xCBF43926
    assert hiplib.crc32_combine(zlib.crc32(b"1234"), zlib.crc32(b"56789"), 5) == 0xCBF43926
    assert hiplib.crc32_combine(0, 0xCBF43926, 9) == 0xCBF43926  # nothing before it


def test_zeros_helper_agrees_with_zlib(hiplib):
    for n in (4097, 70000, (1 << 20) + 3):
        assert zeros_crc(hiplib, n) == zlib.crc32(bytes(n))


@pytest.mark.parametrize("len_b", [0, 1, 7, 4096, (1 << 20) + 3])
def test_combine_random_pieces(hiplib, len_b):
    rng = np.random.default_rng(len_b)
    for len_a in (0, 1, 13, 5000):
        a = rng.integers(0, 256, len_a, dtype=np.uint8).tobytes()
        b = rng.integers(0, 256, len_b, dtype=np.uint8).tobytes()
        assert hiplib.crc32_combine(zlib.crc32(a), zlib.crc32(b), len_b) == zlib.crc32(a + b), (len_a, len_b)


def matrix_advance(crc, nzeros):
    """The CRC register after nzeros more zero bytes, by squaring the 32 x 32
    bit matrix of one zero BIT (a method apart from the library's polynomial
    products): columns as integers, product = XOR of the selected columns."""
    def times(mat, vec):
        out, i = 0, 0
        while vec:
            if vec & 1:
                out ^= mat[i]
            vec >>= 1
            i += 1
        return out

    mat = [0xEDB88320] + [1 << (i - 1) for i in range(1, 32)]  # one zero bit: shift right, feed the polynomial
    n = nzeros * 8
    while n:
        if n & 1:
            crc = times(mat, crc)
        mat = [times(mat, col) for col in mat]
        n >>= 1
    return crc


def zero_run_crc(a, nzeros):
    """zlib.crc32(a + nzeros zero bytes) without the zeros: the register is
    the CRC with the final XOR undone."""
    return matrix_advance(zlib.crc32(a) ^ 0xFFFFFFFF, nzeros) ^ 0xFFFFFFFF


@pytest.mark.parametrize("len_b", [(1 << 20) + 3, (1 << 32) + 5])
def test_combine_long_zero_piece(hiplib, len_b):
    """B = len_b zero bytes, never allocated: its CRC comes from combining
    halves, the expected crc(A || B) from the bit-matrix method, itself
    checked against zlib on the length zlib can be given directly."""
    a = np.random.default_rng(3).integers(0, 256, 777, dtype=np.uint8).tobytes()
    assert zero_run_crc(a, (1 << 20) + 3) == zlib.crc32(a + bytes((1 << 20) + 3))
    assert zero_run_crc(b"", 4097) == zlib.crc32(bytes(4097))
    assert hiplib.crc32_combine(zlib.crc32(a), zeros_crc(hiplib, len_b), len_b) == zero_run_crc(a, len_b)
    assert zeros_crc(hiplib, len_b) == zero_run_crc(b"", len_b)


def test_combine_is_associative(hiplib):
    rng = np.random.default_rng(5)
    a, b, c = (rng.integers(0, 256, n, dtype=np.uint8).tobytes() for n in (1001, 17, 65537))
    ca, cb, cc = zlib.crc32(a), zlib.crc32(b), zlib.crc32(c)
    comb = hiplib.crc32_combine
    left = comb(comb(ca, cb, len(b)), cc, len(c))
    right = comb(ca, comb(cb, cc, len(c)), len(b) + len(c))
    assert left == right == zlib.crc32(a + b + c)


def test_argument_errors(hiplib):
    from redset_amd import _lib

    L = _lib.load()
    plan = c_void_p()
    one = (_lib.CrcRange * 2)()
    one[0].ptr, one[0].len = 256, 64
    one[1].ptr, one[1].len = None, 5
    assert L.redset_hip_plan_crc32(None, 1, byref(plan)) == _lib.REDSET_FAILURE
    assert b"null range array" in L.redset_hip_last_error()
    assert L.redset_hip_plan_crc32(one, 0, byref(plan)) == _lib.REDSET_FAILURE
    assert b"0 ranges" in L.redset_hip_last_error()
    assert L.redset_hip_plan_crc32(one, -3, byref(plan)) == _lib.REDSET_FAILURE
    assert L.redset_hip_plan_crc32(one, 2, byref(plan)) == _lib.REDSET_FAILURE
    assert b"range 1: null pointer with 5 bytes" in L.redset_hip_last_error()
    assert L.redset_hip_plan_crc32(one, 1, None) == _lib.REDSET_FAILURE
    assert b"null plan out-pointer" in L.redset_hip_last_error()
    assert not plan.value
    # the report on no plan, and on a plan of another kind (an empty combine plan: no device work)
    out = (c_uint * 4)()
    assert L.redset_hip_plan_crc32_report(None, None, out, 4) == _lib.REDSET_FAILURE
    other = c_void_p()
    assert L.redset_hip_plan_combine(None, 0, 64, byref(other)) == 0
    assert L.redset_hip_plan_crc32_report(other, None, out, 4) == _lib.REDSET_FAILURE
    assert b"not a CRC plan" in L.redset_hip_last_error()
    assert L.redset_hip_plan_crc32_report(other, None, None, 4) == _lib.REDSET_FAILURE
    L.redset_hip_plan_destroy(other)
    # the streaming call
    io, st = _lib.StreamIO(), _lib.StreamStats()
    spans = (_lib.CrcSpan * 1)(_lib.CrcSpan(0, 0, 0, 10))
    assert L.redset_hip_crc32_stream(64, spans, 1, 0, 0, None, byref(st), out) == _lib.REDSET_FAILURE
    assert b"null redset_hip_io" in L.redset_hip_last_error()
    assert L.redset_hip_crc32_stream(64, spans, 1, 0, 0, byref(io), byref(st), out) == _lib.REDSET_FAILURE  # no read
    assert L.redset_hip_crc32_stream(64, None, 1, 0, 0, byref(io), byref(st), out) == _lib.REDSET_FAILURE
    assert b"bad span list" in L.redset_hip_last_error()
    assert L.redset_hip_crc32_stream(64, spans, 1, 0, 0, byref(io), byref(st), None) == _lib.REDSET_FAILURE
    assert L.redset_hip_crc32_stream(64, spans, -1, 0, 0, byref(io), byref(st), out) == _lib.REDSET_FAILURE
    io.read = 1  # never called: the checks below fail first
    assert L.redset_hip_crc32_stream(0, spans, 1, 0, 0, byref(io), byref(st), out) == _lib.REDSET_FAILURE
    assert b"chunk_size 0" in L.redset_hip_last_error()
    spans[0].kind = 2
    assert L.redset_hip_crc32_stream(64, spans, 1, 0, 0, byref(io), byref(st), out) == _lib.REDSET_FAILURE
    assert b"kind 2" in L.redset_hip_last_error()
    spans[0] = _lib.CrcSpan(-1, 0, 0, 10)
    assert L.redset_hip_crc32_stream(64, spans, 1, 0, 0, byref(io), byref(st), out) == _lib.REDSET_FAILURE
    assert b"rank -1" in L.redset_hip_last_error()


def test_python_names_exported(hiplib):
    from redset_amd import stream

    for name in ("Crc32Plan", "crc32_combine"):
        assert hasattr(hiplib, name), name
    assert hasattr(stream, "crc32_stream")
    for name in ("execute", "report", "info"):
        assert hasattr(hiplib.Crc32Plan, name)
