"""CPU tests of the two-error repair's host side (include/redset_hip.h,
"repair2"): the power basis against its closed form and its identity, and
redset_hip_rs_locate_syndrome2 against the brute-force verdict of
tests/repair2_ref.py. (252, 4) has p + e = 256: every byte value is a point."""
import numpy as np
import pytest

import repair2_ref
import repair_ref

SHAPES = [(6, 4), (20, 4), (252, 4)]


@pytest.fixture(scope="module")
def rd():
    import redset_amd

    redset_amd.load()
    return redset_amd


_stripes = {}


def stripe(rd, oracle, p, c):
    if (p, c) not in _stripes:
        _stripes[p, c] = repair_ref.Stripe(oracle, rd.RSCodec(p, 4), c)
    return _stripes[p, c]


def cells_of(st):
    """The members in power_basis order: data inputs ascending, then parity rows."""
    data = [m for m in range(st.p) if st.row[m] < 0]
    return data + sorted((m for m in range(st.p) if st.row[m] >= 0), key=lambda m: st.row[m])


@pytest.mark.parametrize("p,e", SHAPES)
def test_power_basis_closed_form_and_identity(rd, oracle, p, e):
    mul = repair_ref.mul_table(oracle).astype(np.int64)
    inv = np.array([0] + [int(np.nonzero(mul[a] == 1)[0][0]) for a in range(1, 256)])
    codec = rd.RSCodec(p, e)
    for c in sorted({0, 1, p // 2, p - 1}):
        st = stripe(rd, oracle, p, c)
        alpha, u, winv = codec.power_basis(c)
        members = cells_of(st)
        want_alpha = [m if st.row[m] < 0 else p + st.row[m] for m in members]
        assert alpha.tolist() == want_alpha
        for i, a in enumerate(want_alpha):
            prod = 1
            for b in range(p + e):
                if b != a:
                    prod = mul[prod, a ^ b]
            assert u[i] == inv[prod], (c, i)
        for i, m in enumerate(members):
            h = st.A[:, m] if st.row[m] < 0 else np.eye(e, dtype=np.uint8)[:, st.row[m]]
            power = int(u[i])  # u * alpha^t, 0^0 = 1
            for t in range(e):
                assert np.bitwise_xor.reduce(mul[winv[t], h]) == power, (c, i, t)
                power = mul[power, alpha[i]]


def test_every_single_error(rd, oracle):
    p, e = 6, 4
    codec = rd.RSCodec(p, e)
    for c in range(p):
        st = stripe(rd, oracle, p, c)
        for m in range(p):
            for x, syn in enumerate(repair_ref.unpack(st.keys[m], e), start=1):
                assert codec.locate_syndrome2(c, syn) == [(m, x)], (c, m, x)
        assert codec.locate_syndrome2(c, [0] * e) == []


def explicit_pairs(st):
    """(a, b) with member 0's data cell (X = 0), two parity cells, data + parity."""
    data, par = [m for m in range(st.p) if st.row[m] < 0], [m for m in range(st.p) if st.row[m] >= 0]
    zero = [(0, data[1]), (0, par[0])] if data[0] == 0 else []  # stripes >= e: member 0 holds data
    assert zero or st.c < st.e
    return zero + [(par[0], par[-1]), (data[-1], par[1])]


@pytest.mark.parametrize("p,e", SHAPES)
def test_locate_syndrome2_equals_brute_force(rd, oracle, p, e):
    codec = rd.RSCodec(p, e)
    rng = np.random.default_rng(200 + p)
    n = 60 if p < 100 else 12
    for c in (0, e):  # member 0 holds parity (point 0 is shortened), then data
        st = stripe(rd, oracle, p, c)
        S, nerr = [], []
        for k in (1, 2, 3):
            for _ in range(n):
                mem = rng.choice(p, k, replace=False)
                S.append(np.bitwise_xor.reduce([st.keys[m][rng.integers(0, 255)] for m in mem]))
                nerr.append(k)
        for a, b in explicit_pairs(st):
            for x1, x2 in ((1, 1), (0x53, 0x53), (0x80, 0x1D)):
                S.append(st.keys[a][x1 - 1] ^ st.keys[b][x2 - 1])
                nerr.append(-2)  # a pair that must be found, exactly
                assert repair2_ref.locate2(st, S[-1:]) == [sorted([(a, x1), (b, x2)])]
        want = repair2_ref.locate2(st, np.array(S, np.uint32))
        for s, k, w, syn in zip(S, nerr, want, repair_ref.unpack(S, e)):
            assert codec.locate_syndrome2(c, syn) == w, (c, syn, k)
            assert len(w) == abs(k) or k == 3  # distance 5: one and two wrong bytes are always found
            # whatever is answered zeroes the syndrome
            assert np.bitwise_xor.reduce([st.keys[m][x - 1] for m, x in w] + [np.uint32(0)]) == (s if w else 0)


@pytest.mark.parametrize("p,e", [(4, 2), (11, 3)])
def test_other_encodings_are_errors(rd, p, e):
    codec = rd.RSCodec(p, e)
    with pytest.raises(rd.RedsetHipError, match="4 parity rows"):
        codec.power_basis(0)
    with pytest.raises(rd.RedsetHipError, match="4 parity rows"):
        codec.locate_syndrome2(0, [1] * e)
    fake = [0x1000 * (r + 1) for r in range(p)]  # never dereferenced: refused first
    with pytest.raises(ValueError, match="e = 4"):
        codec.plan_repair(fake, fake, 64, 64, max_errors=2)
