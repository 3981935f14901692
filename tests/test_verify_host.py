"""CPU tests of set verification's host side (include/redset_hip.h, "set
verification"): the locate rule against a numpy restatement, and the argument
checks of the verify entry points. No kernel runs here."""
from ctypes import byref, c_int, c_ubyte, c_ulonglong, c_void_p

import numpy as np
import pytest

import np_ref

SHAPES = [(4, 2), (6, 3), (11, 3), (20, 4)]


@pytest.fixture(scope="module")
def hiplib():
    import os

    import redset_amd
    from redset_amd import _lib

    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__

        __graft_entry__.build_library()
    return redset_amd


def syndrome_of(M, p, e, c, errors):
    """Syndrome column of stripe c when member m's byte is off by eps, for
    every (m, eps) of `errors`: a data cell's error spreads through its
    column of the parity rows, a parity cell's stays in its own row."""
    syn = np.zeros(e, np.uint8)
    for m, eps in errors:
        enc = np_ref.encoding_id(p, e, m, c)
        if enc < p:
            syn ^= np_ref.MUL[M[p:, m], eps]
        else:
            syn[enc - p] ^= eps
    return syn


def rule(M, p, e, c, syn):
    """The locate rule, restated: exactly one nonzero row i names the holder
    of parity row i; otherwise the unique data member m with one x such that
    syn[j] = A[j][m] * x for every j; else -1."""
    nz = np.flatnonzero(syn)
    if e < 2 or len(nz) == 0:
        return -1
    if len(nz) == 1:
        return (c - int(nz[0])) % p
    found = []
    for m in range(p):
        if np_ref.encoding_id(p, e, m, c) >= p:
            continue
        col = M[p:, m]
        if any(np.array_equal(np_ref.MUL[col, x], syn) for x in range(1, 256)):
            found.append(m)
    return found[0] if len(found) == 1 else -1


@pytest.mark.parametrize("p,e", SHAPES)
def test_locate_every_single_error(hiplib, p, e):
    """Every stripe, every member, every error value: the member comes back."""
    codec = hiplib.RSCodec(p, e)
    M = np_ref.encoding_matrix(p, e)
    for c in range(p):
        assert (c - 0) % p == [r for r in range(p) if np_ref.encoding_id(p, e, r, c) == p][0]
        for m in range(p):
            for eps in range(1, 256):
                syn = syndrome_of(M, p, e, c, [(m, eps)])
                assert codec.locate_syndrome(c, syn) == m, (c, m, eps)
        assert codec.locate_syndrome(c, np.zeros(e, np.uint8)) == -1


def test_locate_needs_two_parity_rows(hiplib):
    codec = hiplib.RSCodec(8, 1)
    for c in range(8):
        for eps in (1, 77, 255):
            assert codec.locate_syndrome(c, [eps]) == -1


@pytest.mark.parametrize("p,e", SHAPES)
def test_locate_two_member_errors_follow_the_rule(hiplib, p, e):
    """Two wrong members in one column: the answer is -1 or a member for which
    the rule truly holds -- exactly what the numpy rule gives."""
    codec = hiplib.RSCodec(p, e)
    M = np_ref.encoding_matrix(p, e)
    rng = np.random.default_rng(100 * p + e)
    for _ in range(300):
        c = int(rng.integers(p))
        m1, m2 = (int(x) for x in rng.choice(p, 2, replace=False))
        e1, e2 = (int(x) for x in rng.integers(1, 256, 2))
        syn = syndrome_of(M, p, e, c, [(m1, e1), (m2, e2)])
        want = rule(M, p, e, c, syn)
        got = codec.locate_syndrome(c, syn)
        assert got == want, (c, m1, e1, m2, e2, syn)
        if got >= 0 and len(np.flatnonzero(syn)) > 1:
            col = M[p:, got]
            assert any(np.array_equal(np_ref.MUL[col, x], syn) for x in range(1, 256))


def test_argument_errors(hiplib):
    from redset_amd import _lib

    L = _lib.load()
    h = c_void_p()
    assert L.redset_hip_rs_create(11, 3, byref(h)) == 0
    ptrs = _lib.ptr_array([256] * 11)
    # a NULL out pointer
    assert L.redset_hip_rs_plan_verify(h, ptrs, ptrs, 64, 64, None) == _lib.REDSET_FAILURE
    assert b"null plan out-pointer" in L.redset_hip_last_error()
    assert L.redset_hip_xor_plan_verify(4, ptrs, ptrs, 64, 64, None) == _lib.REDSET_FAILURE
    assert b"null plan out-pointer" in L.redset_hip_last_error()
    syn = (c_ubyte * 3)(1, 2, 3)
    assert L.redset_hip_rs_locate_syndrome(h, 0, syn, None) == _lib.REDSET_FAILURE
    assert b"null argument" in L.redset_hip_last_error()
    m = c_int()
    assert L.redset_hip_rs_locate_syndrome(h, 11, syn, byref(m)) == _lib.REDSET_FAILURE
    assert b"out of range" in L.redset_hip_last_error()
    # nrows too small: 11 stripes x 3 rows, room for 32
    rows = (_lib.VerifyRow * 33)()
    io = _lib.StreamIO()
    st = _lib.StreamStats()
    assert L.redset_hip_rs_verify_stream(h, 64, 0, 0, 0, 0, byref(io), byref(st), rows, 32) == _lib.REDSET_FAILURE
    assert b"32 report rows, the call reports 33" in L.redset_hip_last_error()
    assert L.redset_hip_xor_verify_stream(4, 64, 0, 0, 0, 0, byref(io), byref(st), rows, 3) == _lib.REDSET_FAILURE
    assert b"3 report rows, the call reports 4" in L.redset_hip_last_error()
    assert L.redset_hip_rs_verify_stream(h, 64, 0, 0, 0, 0, byref(io), byref(st), None, 33) == _lib.REDSET_FAILURE
    # a non-verify plan (an empty combine plan: no device work) passed to the report calls
    plan = c_void_p()
    assert L.redset_hip_plan_combine(None, 0, 64, byref(plan)) == 0
    total = c_ulonglong()
    assert L.redset_hip_plan_verify_report(plan, None, rows, 33, byref(total)) == _lib.REDSET_FAILURE
    assert b"not a verify plan" in L.redset_hip_last_error()
    off = c_ulonglong()
    assert L.redset_hip_plan_verify_locate(plan, None, 0, byref(m), byref(off)) == _lib.REDSET_FAILURE
    assert b"not a verify plan" in L.redset_hip_last_error()
    assert L.redset_hip_plan_verify_locate(plan, None, 0, None, byref(off)) == _lib.REDSET_FAILURE
    assert L.redset_hip_plan_verify_report(None, None, rows, 33, byref(total)) == _lib.REDSET_FAILURE
    L.redset_hip_plan_destroy(plan)
    L.redset_hip_rs_destroy(h)


def test_python_names_exported(hiplib):
    for name in ("VerifyPlan", "xor_plan_verify", "rs_verify_stream", "xor_verify_stream", "verify_set"):
        assert hasattr(hiplib, name), name
    assert hasattr(hiplib.RSCodec, "plan_verify") and hasattr(hiplib.RSCodec, "locate_syndrome")
