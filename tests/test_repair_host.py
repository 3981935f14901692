"""CPU tests of the repair feature's host side: the brute-force numpy locate
of tests/repair_ref.py and redset_hip_rs_locate_syndrome pin each other for
every stripe, member and error value and for sampled double errors; the new
symbols are exported; the plan-time refusals that need no device. The
library loads on the CPU for host-only calls (as tests/test_verify_host.py
relies on)."""
import ctypes

import numpy as np
import pytest

import repair_ref


@pytest.fixture(scope="module")
def rd():
    import redset_amd

    redset_amd.load()
    return redset_amd


@pytest.mark.parametrize("p,e", [(4, 2), (11, 3)])
def test_numpy_locate_equals_host_locate_single_errors(rd, oracle, p, e):
    codec = rd.RSCodec(p, e)
    for c in range(p):
        st = repair_ref.Stripe(oracle, codec, c)
        for m in range(p):
            S = st.keys[m]  # the syndrome of every error value 1..255 in member m
            member, xs = st.locate(S)
            assert (member == m).all() and (xs == np.arange(1, 256)).all(), (c, m)
            for syn in repair_ref.unpack(S, e):
                assert codec.locate_syndrome(c, syn) == m, (c, m, syn)
        assert codec.locate_syndrome(c, [0] * e) == -1
        assert st.locate(np.zeros(1, np.uint32))[0][0] == -1


@pytest.mark.parametrize("p,e", [(4, 2), (11, 3), (20, 4)])
def test_numpy_locate_equals_host_locate_double_errors(rd, oracle, p, e):
    """Two wrong members in one column: whatever the verdict (another member
    for e = 2 sometimes, -1 otherwise), both oracles give the same one."""
    codec = rd.RSCodec(p, e)
    rng = np.random.default_rng(77 + p)
    third = 0
    for c in range(p):
        st = repair_ref.Stripe(oracle, codec, c)
        m1 = rng.integers(0, p, 400)
        m2 = (m1 + rng.integers(1, p, 400)) % p
        S = np.array([st.keys[a][x1 - 1] ^ st.keys[b][x2 - 1]
                      for a, b, x1, x2 in zip(m1, m2, rng.integers(1, 256, 400), rng.integers(1, 256, 400))], np.uint32)
        member, _ = st.locate(S)
        for k, syn in enumerate(repair_ref.unpack(S, e)):
            assert codec.locate_syndrome(c, syn) == member[k], (c, syn)
        assert ((member != m1) & (member != m2)).all()  # never one of the two: each alone explains half
        third += int((member >= 0).sum())
    if e >= 3:
        assert third == 0  # distance >= 4: two errors are never taken for one
    else:
        assert third > 0   # distance 3: some are (the miscorrection the checksums guard against)


def test_exported_symbols(rd):
    from redset_amd import _lib

    for name in ("redset_hip_rs_plan_repair", "redset_hip_plan_repair_report", "redset_hip_rs_repair_stream"):
        assert name in _lib.EXPORTED_SYMBOLS
        assert hasattr(_lib.load(), name)
    assert _lib.PLAN_RS_REPAIR == 8
    assert callable(rd.repair_set) and callable(rd.rs_repair_stream)


@pytest.mark.parametrize("p,e,word", [(8, 1, "one parity row"), (12, 6, "2..4")])
def test_plan_refusals_need_no_device(rd, p, e, word):
    codec = rd.RSCodec(p, e)
    fake = [0x1000 * (r + 1) for r in range(p)]  # never dereferenced: refused first
    with pytest.raises(rd.RedsetHipError, match=word):
        codec.plan_repair(fake, fake, 64, 64)
    io = rd.stream.HostIO(p, fake, fake, 64)
    with pytest.raises(rd.RedsetHipError, match=word):
        rd.rs_repair_stream(codec, 64, io)
    io.close()


def test_xor_refusal(rd):
    with pytest.raises(rd.RedsetHipError, match="one parity row"):
        rd.xor_plan_repair(4, [1] * 4, [1] * 4, 64)


def test_plan_argument_checks_need_no_device(rd):
    codec = rd.RSCodec(4, 2)
    fake = [0x1000 * (r + 1) for r in range(4)]
    for stripes, word in (([4], "out of range"), ([1, 1], "twice"), ([-1], "out of range")):
        with pytest.raises(rd.RedsetHipError, match=word):
            codec.plan_repair(fake, fake, 64, 64, stripes=stripes)
    with pytest.raises(rd.RedsetHipError, match="cell_stride"):
        codec.plan_repair(fake, fake, 64, 32)
    # the report calls refuse a null plan
    from redset_amd import _lib

    assert _lib.load().redset_hip_plan_repair_report(None, None, None, 0, None, 0) == _lib.REDSET_FAILURE
    assert ctypes.sizeof(_lib.RepairSummary) == 48 and ctypes.sizeof(_lib.RepairCell) == 16
