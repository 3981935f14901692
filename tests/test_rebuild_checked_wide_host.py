"""CPU tests of the wide checked rebuild's host contract (include/redset_hip.h,
"checked rebuild, wide"): check_basis_wide against numpy GF(256) arithmetic on
the encode matrix and redset_hip_rs_decode_matrix, and locate_reduced_wide
against the errors the sums were built from."""
import numpy as np
import pytest

import repair_ref
import repair_wide_ref as wref
from rebuild_checked_ref import inv_table

# (p, e, lost): s = 4, 4, 7, 1, 7
SHAPES = [(8, 5, [1]), (10, 6, [0, 9]), (12, 8, [4]), (12, 7, [1, 5, 6, 9, 10, 11]), (248, 8, [5])]


@pytest.fixture(scope="module")
def rd():
    import redset_amd

    redset_amd.load()
    return redset_amd


def closed_form(st, lost):
    """(column members, alpha, u', C) of the stripe from the definitions:
    u_i = 1 / prod_{b != a} (a ^ b) over the p + e points, u'_i = u_i *
    prod_{l lost} (alpha_i ^ alpha_l), C[j, i] = u'_i * alpha_i^j."""
    p, e, mul = st.p, st.e, st.mul
    inv = inv_table(mul)
    data, _ = wref.members_of(st)
    colm = data + [st.row.index(j) for j in range(e)]
    alpha = np.array(data + list(range(p, p + e)), np.uint8)
    up = np.zeros(p, np.uint8)
    lost_alpha = [int(alpha[colm.index(r)]) for r in lost]
    for i, a in enumerate(alpha.tolist()):
        v = 1
        for b in range(p + e):
            if b != a:
                v = int(mul[v, a ^ b])
        v = int(inv[v])
        for la in lost_alpha:
            v = int(mul[v, a ^ la])
        up[i] = v
    C = np.zeros((e - len(lost), p), np.uint8)
    row = up.copy()
    for j in range(C.shape[0]):
        C[j] = row
        row = mul[row, alpha]
    return colm, alpha, up, C


def matmul(mul, A, B):
    out = np.zeros((A.shape[0], B.shape[1]), np.uint8)
    for k in range(A.shape[1]):
        out ^= mul[A[:, k][:, None], B[k][None, :]]
    return out


@pytest.mark.parametrize("p,e,lost", SHAPES)
def test_check_basis_wide(rd, oracle, p, e, lost):
    codec = rd.RSCodec(p, e)
    d, s = p - e, e - len(lost)
    for c in (0, e, p - 1):
        st = repair_ref.Stripe(oracle, codec, c)
        colm, alpha, up, C = closed_form(st, lost)
        got_alpha, got_up, M, lost_cols = codec.check_basis_wide(lost, c)
        assert lost_cols == [colm.index(r) for r in lost]
        assert np.array_equal(got_alpha, alpha) and np.array_equal(got_up, up)
        assert not M[:s, lost_cols].any() and not up[lost_cols].any()
        assert np.count_nonzero(up) == p - len(lost)
        assert np.array_equal(M[:s], C)
        # every row is a combination of the rows of H = [A | I]: the one its parity columns name
        H = np.concatenate([st.A[:, colm[:d]], np.eye(e, dtype=np.uint8)], axis=1)
        assert np.array_equal(matmul(st.mul, M[:, d:], H), M)
        D = codec.decode_matrix(lost, c)
        want = D[:, colm]
        want[np.arange(len(lost)), lost_cols] = 1
        assert np.array_equal(M[s:], want)


@pytest.mark.parametrize("p,e,lost", SHAPES)
def test_locate_reduced_wide(rd, oracle, p, e, lost):
    codec = rd.RSCodec(p, e)
    s = e - len(lost)
    t = s // 2
    rng = np.random.default_rng(p * e + s)
    for c in (0, e):
        st = repair_ref.Stripe(oracle, codec, c)
        colm, _, _, C = closed_form(st, lost)
        surv = [i for i in range(p) if colm[i] not in lost]
        assert codec.locate_reduced_wide(lost, c, [0] * s) == []
        for nu in range(1, t + 2):
            if nu == t + 1 and s % 2 == 0:
                continue  # even s: t + 1 wrong bytes may miscorrect
            for _ in range(6):
                cols = rng.choice(surv, nu, replace=False)
                xs = rng.integers(1, 256, nu)
                errs = sorted((colm[i], int(x)) for i, x in zip(cols, xs))
                T = np.bitwise_xor.reduce(st.mul[C[:, cols], xs[None, :]], axis=1).tolist()
                # odd s, t + 1 wrong bytes: distance 2 t + 2 leaves no codeword within t
                assert codec.locate_reduced_wide(lost, c, T) == (errs if nu <= t else []), (c, errs)
                if nu <= t:
                    assert codec.locate_reduced_wide(lost, c, T, max_errors=nu) == errs


def test_refusals(rd):
    for e in (4, 9):
        with pytest.raises(rd.RedsetHipError, match="5..8"):
            rd.RSCodec(20, e).check_basis_wide([1], 0)
        with pytest.raises(rd.RedsetHipError, match="5..8"):
            rd.RSCodec(20, e).locate_reduced_wide([1], 0, [1] * 8, max_errors=1)
    codec = rd.RSCodec(12, 6)
    for ranks, word in [([], "1..5"), ([0, 1, 2, 3, 4, 5], "1..5"), ([3, 1], "ascending"), ([2, 2], "listed twice"),
                        ([12], "out of range"), ([-1], "out of range")]:
        with pytest.raises(rd.RedsetHipError, match=word):
            codec.check_basis_wide(ranks, 0)
    with pytest.raises(rd.RedsetHipError, match="258"):  # p + e > 256: the points run out, at rs_create already
        rd.RSCodec(250, 8).check_basis_wide([1], 0)
    with pytest.raises(rd.RedsetHipError, match="1..2"):  # s = 5
        codec.locate_reduced_wide([2], 0, [1] * 5, max_errors=3)
    with pytest.raises(rd.RedsetHipError, match="0..0"):  # s = 1: detect only
        codec.locate_reduced_wide([0, 1, 2, 3, 4], 0, [1], max_errors=1)
    assert codec.locate_reduced_wide([0, 1, 2, 3, 4], 0, [1], max_errors=0) == []
