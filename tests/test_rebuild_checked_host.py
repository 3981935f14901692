"""CPU tests of the checked rebuild's host algebra (include/redset_hip.h,
"checked rebuild"): redset_hip_rs_check_matrix against its defining
properties and the CPU oracle's codewords, redset_hip_rs_locate_reduced
against the brute-force reference of tests/rebuild_checked_ref.py, and the
plan-time refusals that need no device. The library loads on the CPU for
host-only calls (as tests/test_verify_host.py relies on)."""
import ctypes
import itertools
from ctypes import c_int, c_ubyte

import numpy as np
import pytest

import rebuild_checked_ref as ref

SMALL = [(5, 3), (6, 4), (4, 2)]
WIDE = [(20, 4), (24, 4)]


@pytest.fixture(scope="module")
def rd():
    import redset_amd

    redset_amd.load()
    return redset_amd


def subsets(p, e, sample=None, seed=0):
    """Every lost subset of size 1 .. e-1, or `sample` seeded ones per size."""
    out = []
    rng = np.random.default_rng(seed)
    for k in range(1, e):
        if sample is None:
            out += [list(s) for s in itertools.combinations(range(p), k)]
        else:
            out += [sorted(rng.choice(p, k, replace=False).tolist()) for _ in range(sample)]
    return out


_sets = {}


def codeword_columns(oracle, p, e, c, st):
    """[p, 8] bytes: member m's cell of stripe c of an oracle-encoded set."""
    if (p, e) not in _sets:
        chunk = 8
        lofi, parity = oracle.random_set(p, p - e, e, chunk, seed=900 + p * 7 + e)
        oracle.OracleRS(p, e).encode_set(lofi, parity, chunk)
        _sets[(p, e)] = np.stack([np.concatenate([lofi[r], parity[r]]).reshape(p, chunk) for r in range(p)])
    return np.stack([_sets[(p, e)][m, st.index[m]] for m in range(p)])


def gf_rank(mul, M):
    M = M.copy()
    inv = ref.inv_table(mul)
    rank = 0
    for col in range(M.shape[1]):
        r = next((j for j in range(rank, M.shape[0]) if M[j, col]), None)
        if r is None:
            continue
        M[[rank, r]] = M[[r, rank]]
        M[rank] = mul[inv[M[rank, col]], M[rank]]
        for j in range(M.shape[0]):
            if j != rank and M[j, col]:
                M[j] ^= mul[M[j, col], M[rank]]
        rank += 1
    return rank


@pytest.mark.parametrize("p,e,sample", [(p, e, None) for p, e in SMALL] + [(p, e, 3) for p, e in WIDE])
def test_check_matrix(rd, oracle, p, e, sample):
    codec = rd.RSCodec(p, e)
    mul = ref.mul_table(oracle)
    for c in range(p):
        for lost in subsets(p, e, sample, seed=c):
            k = len(lost)
            st = ref.Stripe(oracle, codec, c, lost)
            M, lost_cols = codec.check_matrix(lost, c)
            assert M.shape == (e, p) and lost_cols == [st.col_member.index(m) for m in lost], (c, lost)
            assert not M[:e - k][:, lost_cols].any(), (c, lost)                       # check rows vanish on L
            assert np.array_equal(M[e - k:][:, lost_cols], np.eye(k, dtype=np.uint8))  # rebuild rows: identity on L
            assert gf_rank(mul, M) == e, (c, lost)
            by = codeword_columns(oracle, p, e, c, st)     # by member
            cw = by[st.col_member]                         # by column
            assert not st.matvec(M, cw).any(), (c, lost)   # M c = 0 on oracle codewords
            # the rebuild rows over the survivors: decode_matrix's coefficients, and the lost bytes
            D = codec.decode_matrix(lost, c)
            surv_cols = [i for i in range(p) if i not in lost_cols]
            B = M[e - k:]
            assert np.array_equal(B[:, surv_cols], D[:, [st.col_member[i] for i in surv_cols]]), (c, lost)
            assert np.array_equal(st.matvec(B[:, surv_cols], cw[surv_cols]), by[lost]), (c, lost)


class Locator:
    """redset_hip_rs_locate_reduced through preallocated ctypes arguments."""

    def __init__(self, codec, lost, c):
        from redset_amd import _lib

        self.fn = _lib.load().redset_hip_rs_locate_reduced
        self.h, self.k, self.c = codec._h, len(lost), c
        self.r = (c_int * len(lost))(*lost)
        self.syn = (c_ubyte * 4)()
        self.m, self.x = c_int(-1), c_ubyte(0)
        self.pm, self.px = ctypes.byref(self.m), ctypes.byref(self.x)

    def __call__(self, R):
        for j, b in enumerate(R):
            self.syn[j] = b
        assert self.fn(self.h, self.k, self.r, self.c, self.syn, self.pm, self.px) == 0
        return self.m.value, self.x.value


def reduced(st, M, lost_cols, by):
    """R [e - k, N] = the check rows over the columns' bytes `by` [p, N] (by member)."""
    return st.matvec(M[:st.e - st.k], by[st.col_member])


@pytest.mark.parametrize("p,e,sample", [(p, e, None) for p, e in SMALL] + [(p, e, 1) for p, e in WIDE])
def test_locate_reduced_single_errors(rd, oracle, p, e, sample):
    """Every survivor, every error value 1..255: host rule == brute force ==
    (that survivor, that value) with two check rows or more, unlocated with one."""
    codec = rd.RSCodec(p, e)
    stripes = range(p) if sample is None else (0, p // 2, p - 1)
    for c in stripes:
        for lost in subsets(p, e, sample, seed=31 + c):
            st = ref.Stripe(oracle, codec, c, lost)
            M, lost_cols = codec.check_matrix(lost, c)
            loc = Locator(codec, lost, c)
            cw = codeword_columns(oracle, p, e, c, st)[:, :1]
            for m in st.surv:
                by = np.repeat(cw, 255, axis=1)
                by[m] ^= np.arange(1, 256, dtype=np.uint8)
                nonzero, member, xs, v = st.explain(by)
                assert nonzero.all()
                if e - len(lost) >= 2:
                    assert (member == m).all() and (xs == np.arange(1, 256)).all(), (c, lost, m)
                    assert (v == cw[lost]).all()  # the corrected solution is the original
                else:
                    assert (member == -1).all()
                R = reduced(st, M, lost_cols, by)
                for q in range(255):
                    assert loc(R[:, q]) == (member[q], xs[q]), (c, lost, m, q + 1)
            assert loc([0] * (e - len(lost))) == (-1, 0)


@pytest.mark.parametrize("p,e", SMALL + WIDE)
def test_locate_reduced_double_errors(rd, oracle, p, e):
    """Two wrong survivors in a column, seeded: host rule == brute force,
    whatever the verdict. e - k = 3: never located. e - k = 2: the sample
    holds both miscorrected and unlocated columns (asserted of the sample)."""
    codec = rd.RSCodec(p, e)
    rng = np.random.default_rng(1234 + p)
    mis = {2: 0, 3: 0}
    unl = {2: 0, 3: 0}
    n = 200 if p < 10 else 60
    for c in range(0, p, 1 if p < 10 else 5):
        for lost in subsets(p, e, 2 if p >= 10 else None, seed=c):
            nck = e - len(lost)
            st = ref.Stripe(oracle, codec, c, lost)
            M, lost_cols = codec.check_matrix(lost, c)
            loc = Locator(codec, lost, c)
            by = np.repeat(codeword_columns(oracle, p, e, c, st)[:, 1:2], n, axis=1)
            a = rng.integers(0, len(st.surv), n)
            b = (a + rng.integers(1, len(st.surv), n)) % len(st.surv)
            surv = np.array(st.surv)
            by[surv[a], np.arange(n)] ^= rng.integers(1, 256, n, dtype=np.uint8)
            by[surv[b], np.arange(n)] ^= rng.integers(1, 256, n, dtype=np.uint8)
            nonzero, member, xs, _ = st.explain(by)
            R = reduced(st, M, lost_cols, by)
            for q in range(n):
                assert loc(R[:, q]) == (member[q], xs[q]), (c, lost, q)
            if nck >= 2:
                assert nonzero.all()  # distance >= 3: two errors never cancel
                assert ((member != surv[a]) & (member != surv[b])).all()
            if nck in mis:
                mis[nck] += int((member >= 0).sum())
                unl[nck] += int((nonzero & (member < 0)).sum())
            if nck == 1:
                assert (member == -1).all()
    if e >= 3:
        assert mis[2] > 0 and unl[2] > 0, (mis, unl)  # distance 3: both outcomes are in the sample
    if e >= 4:
        assert mis[3] == 0 and unl[3] > 0, (mis, unl)  # distance 4: two errors are never taken for one
    if e == 2:
        assert mis[2] == 0 and unl[2] == 0  # no lost set leaves two check rows


def test_wrong_byte_in_a_lost_member_is_ignored(rd, oracle):
    p, e = 6, 4
    codec = rd.RSCodec(p, e)
    for c in range(p):
        for lost in ([1], [0, 4]):
            st = ref.Stripe(oracle, codec, c, lost)
            M, lost_cols = codec.check_matrix(lost, c)
            loc = Locator(codec, lost, c)
            by = codeword_columns(oracle, p, e, c, st)[:, :4].copy()
            by[lost[0]] ^= 0x77
            assert not reduced(st, M, lost_cols, by).any()
            assert loc(reduced(st, M, lost_cols, by)[:, 0]) == (-1, 0)
            assert not st.explain(by)[0].any()
            m = st.surv[2]
            by[m, 1] ^= 0x31
            assert loc(reduced(st, M, lost_cols, by)[:, 1]) == (m, 0x31)
            nonzero, member, xs, _ = st.explain(by)
            assert (member[1], xs[1]) == (m, 0x31) and nonzero.tolist() == [False, True, False, False]


def test_exported_symbols_and_structs(rd):
    from redset_amd import _lib

    for name in ("redset_hip_rs_check_matrix", "redset_hip_rs_locate_reduced", "redset_hip_rs_plan_rebuild_checked",
                 "redset_hip_plan_rebuild_checked_report", "redset_hip_rs_rebuild_checked_stream"):
        assert name in _lib.EXPORTED_SYMBOLS
        assert hasattr(_lib.load(), name)
    assert _lib.PLAN_RS_REBUILD_CHECKED == 9 and _lib.ABI_VERSION == 6
    assert ctypes.sizeof(_lib.RebuildCheckedSummary) == 24
    assert callable(rd.rs_rebuild_checked_stream) and callable(rd.RSCodec.plan_rebuild_checked)
    assert _lib.load().redset_hip_plan_rebuild_checked_report(None, None, None, 0, None, 0) == _lib.REDSET_FAILURE


@pytest.mark.parametrize("p,e,lost,word", [
    (6, 4, [], "no member is lost"),
    (6, 4, [0, 1, 2, 3], "nothing left to check"),
    (5, 3, [0, 1, 2, 3], "cannot rebuild 4 members"),
    (12, 6, [1], "2..4"),
    (6, 4, [2, 2], "listed twice"),
    (6, 4, [6], "out of range"),
    (6, 4, [-1], "out of range"),
])
def test_refusals_need_no_device(rd, p, e, lost, word):
    codec = rd.RSCodec(p, e)
    fake = [0x1000 * (r + 1) for r in range(p)]  # never dereferenced: refused first
    with pytest.raises(rd.RedsetHipError, match=word):
        codec.plan_rebuild_checked(lost, fake, fake, 64, 64)
    io = rd.stream.HostIO(p, fake, fake, 64)
    with pytest.raises(rd.RedsetHipError, match=word):
        rd.rs_rebuild_checked_stream(codec, lost, 64, io)
    io.close()


def test_unsorted_ranks_are_refused_by_the_c_abi(rd):
    from redset_amd import _lib

    codec = rd.RSCodec(6, 4)
    buf, cols = (c_ubyte * 24)(), (c_int * 2)()
    assert _lib.load().redset_hip_rs_check_matrix(codec._h, 2, (c_int * 2)(3, 1), 0, buf, cols) == _lib.REDSET_FAILURE
    assert b"ascending" in _lib.load().redset_hip_last_error()
    # k == e: no check rows, the rebuild rows alone
    M, lost_cols = codec.check_matrix([0, 1, 2, 3], 0)
    assert np.array_equal(M[:, lost_cols], np.eye(4, dtype=np.uint8))
