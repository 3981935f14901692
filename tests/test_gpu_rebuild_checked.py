"""GPU tests of checked rebuild plans (include/redset_hip.h, "checked
rebuild"). The set before loss and damage comes from the CPU oracle; the
verdict on every damaged byte column from the brute-force reference of
tests/rebuild_checked_ref.py; the bytes of unlocated columns from the CPU
oracle's plain rebuild of the damaged survivors. After an execute the WHOLE
device allocation -- survivors, the lost cells and the sentinel-filled padding
up to cell_stride and around the set -- must equal the prediction byte for
byte, and the report the predicted counts and first offsets exactly.

Clean images are made once per (shape, chunk, layout) and shared, never
modified."""
import numpy as np
import pytest

import rebuild_checked_ref as ref
from rebuild_checked_ref import NO, Dev

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

# (p, e, lost): e - k = 2 corrects, 3 also detects doubles, 1 only detects;
# 16 and more than 16 data inputs (the kernel takes any number of survivors)
SHAPES = [(5, 3, [1]), (6, 4, [1, 3]), (6, 4, [2]), (5, 3, [0, 3]), (4, 2, [1]), (20, 4, [7]), (24, 4, [5, 20])]
# 1, 15: byte path only; 16: one vector, no tail; 4096 + 5: one block's worth
# of vectors then a tail; 3 * 4096 + 16 + 7: several blocks per job plus a tail
CHUNKS = [1, 15, 16, 4096 + 5, 3 * 4096 + 16 + 7]
# (chunk, packed, shift): the last has no cell 16-B aligned (byte path throughout)
LAYOUTS = [(ch, False, 0) for ch in CHUNKS] + [(4096 + 5, True, 3)]
CASES = [(p, e, lost, ch, pk, sh) for p, e, lost in SHAPES for ch, pk, sh in LAYOUTS]
IDS = [f"p{p}e{e}k{len(lost)}-c{ch}{'u' if pk else ''}" for p, e, lost, ch, pk, sh in CASES]


@pytest.fixture(scope="module")
def rd():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import redset_amd

    redset_amd.load()
    return redset_amd


@pytest.fixture(scope="module", autouse=True)
def fault_counts_unchanged(rd):
    """No checked-rebuild test may move the ring-fault or hang-fault counts."""
    torch.cuda.synchronize()
    before = (rd.ring_faults(clear=False), rd.hang_faults(clear=False))
    assert before == (0, 0)
    yield
    torch.cuda.synchronize()
    assert (rd.ring_faults(clear=False), rd.hang_faults(clear=False)) == (0, 0)


def plan(codec, dev, lost, **kw):
    return codec.plan_rebuild_checked(lost, dev.lofi(), dev.parity(), dev.chunk, dev.stride, **kw)


def run(pl):
    pl.execute()
    torch.cuda.synchronize()
    return pl.report()


def check_report(got, want):
    for g, w, name in zip(got, want, ("corrected", "first", "unlocated", "first_unlocated")):
        assert np.array_equal(g, w), f"{name}: got {g.tolist()} want {w.tolist()}"


def positions(chunk):
    """The damaged offsets of a cell: 0, the last byte, the last byte of the
    vector region, the first tail byte, both sides of a block boundary, two
    adjacent columns and a 64-byte run; clipped to the cell."""
    nv = chunk // 16 * 16
    single = {0, chunk - 1, nv - 1, nv, 4095, 4096}
    single = sorted(o for o in single if 0 <= o < chunk)
    adjacent = [o for o in (7, 8) if o < chunk and o not in single]
    run = [o for o in range(4200, 4264) if o < chunk] or [o for o in range(2, 12) if o < chunk and o not in single + adjacent]
    return single, adjacent, run


def single_damage(oracle, codec, clean, lost, chunk, stripes, seed):
    """One wrong byte per damaged column: (damaged image, {stripe: columns})."""
    rng = np.random.default_rng(seed)
    img = clean.copy()
    cols = {}
    for c in stripes:
        st = ref.Stripe(oracle, codec, c, lost)
        data = [m for m in st.surv if st.row[m] < 0]
        par = [m for m in st.surv if st.row[m] >= 0]
        single, adjacent, run = positions(chunk)
        who = data + par  # surviving data cells and surviving parity cells alike
        for i, o in enumerate(single):
            m = who[(i + c) % len(who)]
            img[m, st.index[m], o] ^= rng.integers(1, 256, dtype=np.uint8)
        for m, o in zip((who[0], who[-1]), adjacent):  # adjacent columns, two different survivors
            img[m, st.index[m], o] ^= rng.integers(1, 256, dtype=np.uint8)
        m = who[len(who) // 2]
        img[m, st.index[m], run] ^= rng.integers(1, 256, len(run), dtype=np.uint8)
        cols[c] = single + adjacent + run
    return img, cols


def damaged_stripes(p):
    return sorted({0, p // 2, p - 1})


@pytest.mark.parametrize("p,e,lost,chunk,packed,shift", CASES, ids=IDS)
def test_clean_survivors(rd, oracle, p, e, lost, chunk, packed, shift):
    clean = ref.clean_image(oracle, p, e, chunk, packed)
    codec = rd.RSCodec(p, e)
    start = ref.lose(clean, lost, chunk)
    dev = Dev(start, chunk, e, shift)
    pl = plan(codec, dev, lost, fix_survivors=True)
    got = run(pl)
    assert not got[0].any() and not got[2].any() and (got[1] == NO).all() and (got[3] == NO).all()
    assert np.array_equal(dev.download(), dev.expect(clean))
    # the plain rebuild plan from the same start: the same allocation, byte for byte
    plain = Dev(start, chunk, e, shift)
    codec.plan_rebuild(lost, plain.lofi(), plain.parity(), chunk, plain.stride).execute()
    assert np.array_equal(plain.download(), dev.download())
    k, i = len(lost), pl.info
    assert (i.kind, i.ranks, i.encoding, i.missing, i.jobs, i.launches) == (9, p, e, k, p, 2)
    assert pl.bytes_read == p * (p - k) * chunk and pl.bytes_written == p * k * chunk


@pytest.mark.parametrize("p,e,lost,chunk,packed,shift", CASES, ids=IDS)
def test_one_wrong_byte_per_column(rd, oracle, p, e, lost, chunk, packed, shift):
    """e - k >= 2: rebuilt cells equal the originals, the report the
    reference's; survivors stay as damaged without fix_survivors and are
    restored with it. e - k = 1: every damaged column is unlocated, the
    rebuilt bytes are the plain rebuild's, no survivor byte is written."""
    clean = ref.clean_image(oracle, p, e, chunk, packed)
    codec = rd.RSCodec(p, e)
    k = len(lost)
    img, cols = single_damage(oracle, codec, clean, lost, chunk, damaged_stripes(p), seed=chunk + p)
    want, kept, fixed = ref.predict_set(oracle, codec, img, lost, chunk, cols)
    ncols = sum(len(v) for v in cols.values())
    if e - k >= 2:  # the reference alone: everything located, the originals come back
        assert int(want[0].sum()) == ncols and not want[2].any()
        assert np.array_equal(fixed, clean)
        assert np.array_equal(kept[lost], clean[lost])
    else:
        assert int(want[2].sum()) == ncols and not want[0].any()
        assert np.array_equal(kept, fixed)
        assert not np.array_equal(kept[lost], clean[lost])  # the survivors' errors are in the rebuilt cells
    start = ref.lose(img, lost, chunk)
    for fix, expect in ((False, kept), (True, fixed)):
        dev = Dev(start, chunk, e, shift)
        check_report(run(plan(codec, dev, lost, fix_survivors=fix)), want)
        assert np.array_equal(dev.download(), dev.expect(expect)), f"fix_survivors={fix}"


def double_damage(oracle, codec, clean, lost, chunk, c, seed, n=192, built=0):
    """Two wrong survivors in each of n columns of stripe c (random pairs and
    values), one wrong byte in some further columns and, from column 300 on,
    up to `built` columns whose two errors the reference takes for a third
    survivor's (searched over the second error's value)."""
    rng = np.random.default_rng(seed)
    st = ref.Stripe(oracle, codec, c, lost)
    surv = np.array(st.surv)
    img = clean.copy()
    cols = np.arange(100, 100 + n)
    a = rng.integers(0, len(surv), n)
    b = (a + rng.integers(1, len(surv), n)) % len(surv)
    for which in (a, b):
        for q, o in enumerate(cols):
            m = surv[which[q]]
            img[m, st.index[m], o] ^= rng.integers(1, 256, dtype=np.uint8)
    m = st.surv[-1]
    img[m, st.index[m], 1000:1040] ^= 0x3C
    extra = []
    for q in range(built):
        ma, mb = surv[q % len(surv)], surv[(q + 1) % len(surv)]
        by = np.zeros((st.p, 255), np.uint8)  # the code is linear: errors on the zero codeword
        by[ma] = q + 1
        by[mb] = np.arange(1, 256)
        hit = np.nonzero(st.explain(by)[1] >= 0)[0]
        if hit.size:
            o = 300 + len(extra)
            img[ma, st.index[ma], o] ^= q + 1
            img[mb, st.index[mb], o] ^= int(hit[0]) + 1
            extra.append(o)
    return img, {c: list(cols) + list(range(1000, 1040)) + extra}


@pytest.mark.parametrize("p,e,lost", [(6, 4, [2]), (20, 4, [7])])
def test_two_wrong_bytes_in_a_column_three_check_rows(rd, oracle, p, e, lost):
    """e - k = 3: unlocated, no survivor byte changes, the rebuilt bytes are
    the uncorrected linear rebuild (the CPU oracle's, and the plain plan's)."""
    chunk = 4096 + 5
    clean = ref.clean_image(oracle, p, e, chunk)
    codec = rd.RSCodec(p, e)
    c = 1
    img, cols = double_damage(oracle, codec, clean, lost, chunk, c, seed=5 + p)
    want, kept, fixed = ref.predict_set(oracle, codec, img, lost, chunk, cols)
    assert int(want[2][c]) == 192 and int(want[3][c]) == 100 and int(want[0][c].sum()) == 40
    plain_cpu = ref.oracle_rebuild(oracle, img, e, lost, chunk)
    assert np.array_equal(kept[:, :, 100:292], plain_cpu[:, :, 100:292])
    start = ref.lose(img, lost, chunk)
    dev = Dev(start, chunk, e)
    check_report(run(plan(codec, dev, lost, fix_survivors=True)), want)
    got = dev.download()
    assert np.array_equal(got, dev.expect(fixed))
    plain = Dev(start, chunk, e)
    codec.plan_rebuild(lost, plain.lofi(), plain.parity(), chunk, plain.stride).execute()
    pg = plain.download()[plain.off:plain.off + img.size].reshape(img.shape)
    assert np.array_equal(pg, plain_cpu)
    gi = got[dev.off:dev.off + img.size].reshape(img.shape)
    assert np.array_equal(gi[:, :, 100:292], pg[:, :, 100:292])


@pytest.mark.parametrize("p,e,lost", [(5, 3, [1]), (6, 4, [1, 3]), (24, 4, [5, 20])])
def test_two_wrong_bytes_in_a_column_two_check_rows(rd, oracle, p, e, lost):
    """e - k = 2 (distance 3): every column's outcome is the reference's,
    miscorrection into a third survivor included; the sample holds both
    outcomes."""
    chunk = 4096 + 5
    clean = ref.clean_image(oracle, p, e, chunk)
    codec = rd.RSCodec(p, e)
    c = 2
    img, cols = double_damage(oracle, codec, clean, lost, chunk, c, seed=11 + p, built=8)
    want, kept, fixed = ref.predict_set(oracle, codec, img, lost, chunk, cols)
    mis = int(want[0][c].sum()) - 40
    assert mis >= 4 and int(want[2][c]) > 0 and mis + int(want[2][c]) == len(cols[c]) - 40
    assert not np.array_equal(fixed, clean)  # a miscorrection changes a third survivor
    start = ref.lose(img, lost, chunk)
    for fix, expect in ((False, kept), (True, fixed)):
        dev = Dev(start, chunk, e)
        check_report(run(plan(codec, dev, lost, fix_survivors=fix)), want)
        assert np.array_equal(dev.download(), dev.expect(expect)), f"fix_survivors={fix}"


def test_graph_capture_replay(rd, oracle):
    p, e, lost, chunk = 6, 4, [1, 3], 3 * 4096 + 16 + 7
    clean = ref.clean_image(oracle, p, e, chunk)
    codec = rd.RSCodec(p, e)
    img, cols = single_damage(oracle, codec, clean, lost, chunk, damaged_stripes(p), seed=77)
    want, kept, fixed = ref.predict_set(oracle, codec, img, lost, chunk, cols)
    start = ref.lose(img, lost, chunk)
    direct = Dev(start, chunk, e)
    direct_report = run(plan(codec, direct, lost, fix_survivors=True))
    check_report(direct_report, want)
    dev = Dev(start, chunk, e)
    pl = plan(codec, dev, lost, fix_survivors=True)
    s = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):  # a linear chain: reset, decode
            pl.execute(s)
    torch.cuda.synchronize()
    dev.upload(start)  # a freshly damaged copy, whatever the capture did
    torch.cuda.synchronize()
    g.replay()
    torch.cuda.synchronize()
    check_report(pl.report(), direct_report)
    assert np.array_equal(dev.download()[dev.off:], direct.download()[direct.off:])
    assert np.array_equal(dev.download(), dev.expect(fixed))


@pytest.mark.parametrize("p,e,lost,word", [
    (6, 4, [], "no member is lost"),
    (6, 4, [0, 1, 2, 3], "nothing left to check"),
    (5, 3, [0, 1, 2, 3], "cannot rebuild 4 members"),
    (12, 6, [1], "2..4"),
    (6, 4, [2, 2], "listed twice"),
    (6, 4, [6], "out of range"),
])
def test_refusals_at_plan_time(rd, p, e, lost, word):
    codec = rd.RSCodec(p, e)
    lay = rd.SetLayout.allocate(p, p - e, e, 64, device="cuda")
    with pytest.raises(rd.RedsetHipError, match=word):
        codec.plan_rebuild_checked(lost, lay.lofi_ptrs(), lay.parity_ptrs(), 64, lay.cell_stride)


def test_wrong_kind_reports(rd, oracle):
    from redset_amd import _lib

    p, e, chunk = 5, 3, 16
    clean = ref.clean_image(oracle, p, e, chunk)
    codec = rd.RSCodec(p, e)
    dev = Dev(clean, chunk, e)
    lib = _lib.load()
    pl = plan(codec, dev, [1])
    v = codec.plan_verify(dev.lofi(), dev.parity(), chunk, dev.stride)
    cells, stripes = (_lib.RepairCell * (p * p))(), (_lib.RepairStripe * p)()
    assert lib.redset_hip_plan_rebuild_checked_report(v._h, None, cells, p * p, stripes, p) == _lib.REDSET_FAILURE
    assert b"not a checked rebuild plan" in lib.redset_hip_last_error()
    assert lib.redset_hip_plan_repair_report(pl._h, None, cells, p * p, stripes, p) == _lib.REDSET_FAILURE
    assert lib.redset_hip_plan_rebuild_checked_report(pl._h, None, cells, p, stripes, p) == _lib.REDSET_FAILURE
