"""CPU tests of the wide repair's host contract (include/redset_hip.h,
"repair_wide"): the power basis identity recomputed in numpy, and
locate_syndrome_wide against the errors the syndromes were built from."""
import numpy as np
import pytest

import repair_ref
import repair_wide_ref as ref

SHAPES = [(8, 5), (10, 6), (12, 7), (12, 8), (248, 8)]


@pytest.fixture(scope="module")
def rd():
    import redset_amd

    redset_amd.load()
    return redset_amd


def stripes_of(oracle, codec):
    """Stripe 0 (member 0 holds parity) and stripe e (member 0 holds data: the point 0)."""
    sts = [repair_ref.Stripe(oracle, codec, c) for c in (0, codec.encoding)]
    assert sts[0].row[0] >= 0 and sts[1].row[0] < 0
    return sts


@pytest.mark.parametrize("p,e", SHAPES)
def test_power_basis_identity(rd, oracle, p, e):
    codec = rd.RSCodec(p, e)
    for st in stripes_of(oracle, codec):
        alpha, u, winv = codec.power_basis_wide(st.c)
        data, par = ref.members_of(st)
        assert alpha.tolist() == data + list(range(p, p + e)) and len(set(alpha.tolist())) == p
        H = np.concatenate([st.A[:, data], np.eye(e, dtype=np.uint8)], axis=1)
        for i in range(p):
            got = [int(np.bitwise_xor.reduce(st.mul[winv[k], H[:, i]])) for k in range(e)]
            want, v = [], int(u[i])
            for _ in range(e):
                want.append(v)
                v = int(st.mul[v, alpha[i]])
            assert u[i] != 0 and got == want, (st.c, i)


@pytest.mark.parametrize("p,e", SHAPES)
def test_locate_syndrome_wide(rd, oracle, p, e):
    codec = rd.RSCodec(p, e)
    t = e // 2
    rng = np.random.default_rng(p * e)
    for st in stripes_of(oracle, codec):
        assert codec.locate_syndrome_wide(st.c, [0] * e) == []
        for nu in range(1, t + 2):
            sets = ref.error_sets(st, nu, rng)
            assert len(sets) >= 3
            for errs in sets:
                S = ref.syndrome_of(st, errs)
                if nu <= t:
                    assert codec.locate_syndrome_wide(st.c, S) == errs
                    assert codec.locate_syndrome_wide(st.c, S, max_errors=nu) == errs
                # fewer levels than wrong bytes (or more wrong bytes than t): nothing, or a
                # correction with this very syndrome
                got = codec.locate_syndrome_wide(st.c, S, max_errors=min(nu - 1, t)) if nu > 1 else []
                assert got == [] or (len(got) < nu and ref.syndrome_of(st, got) == S)


def test_refused_shapes(rd):
    for e in (4, 9):
        codec = rd.RSCodec(20, e)
        with pytest.raises(rd.RedsetHipError, match="5..8"):
            codec.power_basis_wide(0)
        with pytest.raises(rd.RedsetHipError, match="5..8"):
            codec.locate_syndrome_wide(0, [1] * e, max_errors=1)
    with pytest.raises(rd.RedsetHipError, match="1..3"):
        rd.RSCodec(10, 6).locate_syndrome_wide(0, [1] * 6, max_errors=4)
    with pytest.raises(rd.RedsetHipError, match="258"):  # p + e > 256: the points run out, at rs_create already
        rd.RSCodec(250, 8).power_basis_wide(0)
