"""GPU tests of repair plans (include/redset_hip.h, "repair"): the clean set
comes from the CPU oracle, the expected verdict of every byte column from the
brute-force numpy locate of tests/repair_ref.py. After an apply execute the
WHOLE device allocation -- the padding between cells, pre-filled with a
sentinel, included -- must equal the prediction byte for byte, and the report
the predicted counts and first offsets exactly.

Oracle encodes are the slow part: a clean image is made once per
(shape, chunk, layout) and shared, never modified."""
import numpy as np
import pytest

import repair_ref
from repair_ref import NO

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

SENTINEL = 0xA5
SHAPES = [(4, 2), (11, 3), (20, 4), (40, 3)]
BIG = (3 << 20) + 5
# (chunk, packed): 16 and 37 are smaller than one wave's vectors; 4096 + 7 packed
# leaves every cell unaligned (byte path only), padded it is vectors plus a tail
LAYOUTS = [(16, False), (37, False), (4096 + 7, True), (4096 + 7, False)]
CASES = [(p, e, ch, pk) for p, e in SHAPES for ch, pk in LAYOUTS] + [(4, 2, BIG, False)]


@pytest.fixture(scope="module")
def rd():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import redset_amd

    redset_amd.load()
    return redset_amd


@pytest.fixture(scope="module", autouse=True)
def fault_counts_unchanged(rd):
    """No repair test may move the ring-fault or hang-fault counts."""
    torch.cuda.synchronize()
    before = (rd.ring_faults(clear=False), rd.hang_faults(clear=False))
    yield
    torch.cuda.synchronize()
    assert (rd.ring_faults(clear=False), rd.hang_faults(clear=False)) == before


_images = {}


def stride_of(chunk, packed):
    return chunk if packed else -(-chunk // 256) * 256


def clean_image(oracle, p, e, chunk, packed):
    """[p, d + e, stride] host bytes of an encoded set, sentinel in the padding."""
    key = (p, e, chunk, packed)
    if key not in _images:
        d = p - e
        lofi, parity = oracle.random_set(p, d, e, chunk, seed=5000 + 100 * p + e + chunk % 991)
        oracle.OracleRS(p, e).encode_set(lofi, parity, chunk)
        img = np.full((p, d + e, stride_of(chunk, packed)), SENTINEL, np.uint8)
        for r in range(p):
            img[r, :d, :chunk] = lofi[r].reshape(d, chunk)
            img[r, d:, :chunk] = parity[r].reshape(e, chunk)
        img.setflags(write=False)
        _images[key] = img
    return _images[key]


class Dev:
    """The image in one device tensor (16 spare bytes in front so that the
    packed layout can start unaligned)."""

    def __init__(self, img, chunk, e):
        self.p, self.cells, self.stride = img.shape
        self.e, self.d, self.chunk = e, self.cells - e, chunk
        self.buf = torch.full((img.size + 32,), SENTINEL, dtype=torch.uint8, device="cuda")
        self.off = (-self.buf.data_ptr()) % 16  # image starts 16-B aligned
        self.upload(img)

    def upload(self, img):
        self.buf[self.off:self.off + img.size].copy_(torch.from_numpy(np.array(img).reshape(-1)))

    def download(self):
        torch.cuda.synchronize()
        return self.buf.cpu().numpy()

    def expect(self, img):
        want = np.full(self.buf.numel(), SENTINEL, np.uint8)
        want[self.off:self.off + img.size] = img.reshape(-1)
        return want

    def lofi(self):
        base = self.buf.data_ptr() + self.off
        return [base + r * self.cells * self.stride for r in range(self.p)]

    def parity(self):
        return [x + self.d * self.stride for x in self.lofi()]


def plan(rd, codec, dev, **kw):
    return codec.plan_repair(dev.lofi(), dev.parity(), dev.chunk, dev.stride, **kw)


def run(pl):
    pl.execute()
    torch.cuda.synchronize()
    return pl.report()


def predict_all(oracle, codec, img, chunk, stripes, cols=None):
    """Predicted report for the listed stripes and the predicted image."""
    p = codec.ranks
    n = len(stripes)
    corrected, first = np.zeros((n, p), np.uint64), np.full((n, p), NO, np.uint64)
    unloc, first_un = np.zeros(n, np.uint64), np.full(n, NO, np.uint64)
    fixed = img.copy()
    for k, c in enumerate(stripes):
        st = repair_ref.Stripe(oracle, codec, c)
        corrected[k], first[k], unloc[k], first_un[k], fixes = repair_ref.predict(st, img, chunk, cols)
        repair_ref.apply_fixes(st, fixed, fixes)
    return (corrected, first, unloc, first_un), fixed


def check_report(got, want):
    for g, w, name in zip(got, want, ("corrected", "first", "unlocated", "first_unlocated")):
        assert np.array_equal(g, w), f"{name}: got {g.tolist()} want {w.tolist()}"


def damage_patterns(oracle, codec, clean, chunk, c, rng):
    """(name, damaged image, damaged columns) for the single-damage patterns of stripe c."""
    st = repair_ref.Stripe(oracle, codec, c)
    data = [m for m in range(st.p) if st.row[m] < 0]
    par = [m for m in range(st.p) if st.row[m] >= 0]
    out = []
    img = clean.copy()
    img[data[-1], st.index[data[-1]], chunk // 2] ^= 0x5A
    out.append(("data byte", img, [chunk // 2]))
    img = clean.copy()
    img[par[-1], st.index[par[-1]], chunk - 1] ^= 0x01
    out.append(("parity byte", img, [chunk - 1]))
    # a 4 KiB run from an odd offset: crosses 16-B positions and, at vector 256
    # (byte 4096), the first block's share; clipped to small cells
    a = 4096 - 100 if chunk > 8192 else min(3, chunk - 1)
    b = min(chunk, a + 4096)
    img = clean.copy()
    img[data[0], st.index[data[0]], a:b] ^= rng.integers(1, 256, b - a, dtype=np.uint8)
    out.append(("4 KiB run", img, np.arange(a, b)))
    img = clean.copy()
    img[data[len(data) // 2], st.index[data[len(data) // 2]], :chunk] = rng.integers(0, 256, chunk, dtype=np.uint8)
    out.append(("whole cell", img, None))
    return out


@pytest.mark.parametrize("p,e,chunk,packed", CASES)
def test_single_damage(rd, oracle, p, e, chunk, packed):
    clean = clean_image(oracle, p, e, chunk, packed)
    codec = rd.RSCodec(p, e)
    rng = np.random.default_rng(chunk + p)
    c = p // 2
    dev = Dev(clean, chunk, e)
    pl = plan(rd, codec, dev)
    for name, img, cols in damage_patterns(oracle, codec, clean, chunk, c, rng):
        cols = None if chunk <= 8192 else (np.arange(chunk) if cols is None else cols)
        want, fixed = predict_all(oracle, codec, img, chunk, list(range(p)), cols)
        assert np.array_equal(fixed, clean) and not want[2].any(), name  # the oracle alone: one wrong byte per column
        dev.upload(img)
        check_report(run(pl), want)
        assert np.array_equal(dev.download(), dev.expect(clean)), name
    # a second execute on the repaired set reports nothing and changes nothing
    got = run(pl)
    assert not got[0].any() and not got[2].any() and (got[1] == NO).all() and (got[3] == NO).all()
    assert np.array_equal(dev.download(), dev.expect(clean))


def test_every_error_value(rd, oracle):
    """(4, 2), chunk 1040: all 255 error values, one column each, spread over
    the members of every stripe."""
    p, e, chunk = 4, 2, 1040
    clean = clean_image(oracle, p, e, chunk, False)
    codec = rd.RSCodec(p, e)
    img = clean.copy()
    for x in range(1, 256):
        c, m = x % p, (x // p) % p
        img[m, repair_ref.Stripe(oracle, codec, c).index[m], 4 * x + 3] ^= x
    want, fixed = predict_all(oracle, codec, img, chunk, list(range(p)))
    assert np.array_equal(fixed, clean) and int(want[0].sum()) == 255
    dev = Dev(img, chunk, e)
    check_report(run(plan(rd, codec, dev)), want)
    assert np.array_equal(dev.download(), dev.expect(clean))


@pytest.mark.parametrize("p,e,nmem", [(4, 2, 3), (11, 3, 4)])
def test_scattered_damage_beyond_rebuild(rd, oracle, p, e, nmem):
    """More damaged members than e -- no erasure set a rebuild could take --
    each with a disjoint 512-byte run in the same stripe: one execute restores
    the set, and a verify plan afterwards is clean."""
    chunk = 4096 + 7
    clean = clean_image(oracle, p, e, chunk, False)
    codec = rd.RSCodec(p, e)
    rng = np.random.default_rng(9)
    c = 1
    st = repair_ref.Stripe(oracle, codec, c)
    img = clean.copy()
    members = list(range(nmem))
    assert nmem > e
    for k, m in enumerate(members):
        a = 5 + k * 700
        img[m, st.index[m], a:a + 512] ^= rng.integers(1, 256, 512, dtype=np.uint8)
    want, fixed = predict_all(oracle, codec, img, chunk, list(range(p)))
    assert np.array_equal(fixed, clean) and not want[2].any()
    assert [int(x) for x in want[0][c][:nmem]] == [512] * nmem
    with pytest.raises(rd.RedsetHipError):
        codec.plan_rebuild(members, [1] * p, [1] * p, chunk, chunk)
    dev = Dev(img, chunk, e)
    check_report(run(plan(rd, codec, dev)), want)
    assert np.array_equal(dev.download(), dev.expect(clean))
    v = codec.plan_verify(dev.lofi(), dev.parity(), chunk, dev.stride)
    v.execute()
    torch.cuda.synchronize()
    assert v.clean


@pytest.mark.parametrize("p,e", [(11, 3), (20, 4), (4, 2)])
def test_two_wrong_members_in_a_column(rd, oracle, p, e):
    """Two members wrong in the same 64 columns, a third damaged elsewhere in
    the stripe. e >= 3: those columns are unlocated and left as damaged, the
    rest is corrected. e = 2: whatever the numpy locate says of each column
    (a miscorrection into a third member, or unlocated) is what happens."""
    chunk = 4096 + 7
    clean = clean_image(oracle, p, e, chunk, False)
    codec = rd.RSCodec(p, e)
    rng = np.random.default_rng(31 + p)
    c = 2
    st = repair_ref.Stripe(oracle, codec, c)
    img = clean.copy()
    for m in (0, 1):
        img[m, st.index[m], 1000:1064] ^= rng.integers(1, 256, 64, dtype=np.uint8)
    img[3, st.index[3], 2000:2100] ^= rng.integers(1, 256, 100, dtype=np.uint8)
    if e == 2:  # four columns built to look like a third member's single error
        x1, x2, t, x3 = repair_ref.miscorrecting_pair(st, 0, 1)
        img[0, st.index[0], 3000:3004] ^= x1
        img[1, st.index[1], 3000:3004] ^= x2
    want, fixed = predict_all(oracle, codec, img, chunk, list(range(p)))
    if e >= 3:
        assert int(want[2][c]) == 64 and int(want[3][c]) == 1000 and int(want[0][c][3]) == 100
        assert np.array_equal(fixed[:, :, 1000:1064], img[:, :, 1000:1064])
    else:
        assert int(want[2][c]) + int(want[0][c].sum()) == 168
        assert t not in (0, 1) and (fixed[t, st.index[t], 3000:3004] == clean[t, st.index[t], 3000:3004] ^ x3).all()
    dev = Dev(img, chunk, e)
    check_report(run(plan(rd, codec, dev)), want)
    assert np.array_equal(dev.download(), dev.expect(fixed))


@pytest.mark.parametrize("p,e,chunk,packed", [(4, 2, 4096 + 7, True), (11, 3, 4096 + 7, False), (40, 3, 37, False)])
def test_dry_run_and_clean_set(rd, oracle, p, e, chunk, packed):
    clean = clean_image(oracle, p, e, chunk, packed)
    codec = rd.RSCodec(p, e)
    dev = Dev(clean, chunk, e)
    for apply in (True, False):
        got = run(plan(rd, codec, dev, apply=apply))
        assert not got[0].any() and not got[2].any() and (got[1] == NO).all() and (got[3] == NO).all()
        assert np.array_equal(dev.download(), dev.expect(clean))
    rng = np.random.default_rng(3)
    img = clean.copy()
    st = repair_ref.Stripe(oracle, codec, 0)
    img[1, st.index[1], 1:min(chunk - 1, 300)] ^= rng.integers(1, 256, min(chunk - 1, 300) - 1, dtype=np.uint8)
    img[p - 1, st.index[p - 1], chunk - 1] ^= 0x80
    want, fixed = predict_all(oracle, codec, img, chunk, list(range(p)))
    assert np.array_equal(fixed, clean)
    dev.upload(img)
    check_report(run(plan(rd, codec, dev, apply=False)), want)
    assert np.array_equal(dev.download(), dev.expect(img))  # no byte modified


def test_stripe_list(rd, oracle):
    p, e, chunk = 11, 3, 4096 + 7
    clean = clean_image(oracle, p, e, chunk, False)
    codec = rd.RSCodec(p, e)
    img = clean.copy()
    for c in (4, 7):
        st = repair_ref.Stripe(oracle, codec, c)
        img[2, st.index[2], 100 + c:140 + c] ^= 0x33
    dev = Dev(img, chunk, e)
    pl = plan(rd, codec, dev, stripes=[7])
    assert pl.info.jobs == 1
    want, fixed = predict_all(oracle, codec, img, chunk, [7])
    assert not np.array_equal(fixed, clean)  # stripe 4 stays damaged
    got = run(pl)
    assert got[0].shape == (1, p) and got[2].shape == (1,)
    check_report(got, want)
    assert np.array_equal(dev.download(), dev.expect(fixed))


def test_graph_capture_replay(rd, oracle):
    p, e, chunk = 4, 2, 4096 + 7
    clean = clean_image(oracle, p, e, chunk, False)
    codec = rd.RSCodec(p, e)
    img = clean.copy()
    st = repair_ref.Stripe(oracle, codec, 3)
    img[0, st.index[0], 17:600] ^= 0x42
    want, fixed = predict_all(oracle, codec, img, chunk, list(range(p)))
    assert np.array_equal(fixed, clean)
    dev = Dev(img, chunk, e)
    pl = plan(rd, codec, dev)
    s = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):  # a linear chain: reset, repair
            pl.execute(s)
    torch.cuda.synchronize()
    dev.upload(img)  # a freshly damaged copy, whatever the capture did
    torch.cuda.synchronize()
    g.replay()
    torch.cuda.synchronize()
    check_report(pl.report(), want)
    assert np.array_equal(dev.download(), dev.expect(clean))


def test_plan_info_and_wrong_kind_reports(rd, oracle):
    from redset_amd import _lib

    p, e, chunk = 11, 3, 37
    clean = clean_image(oracle, p, e, chunk, False)
    codec = rd.RSCodec(p, e)
    dev = Dev(clean, chunk, e)
    pl = plan(rd, codec, dev)
    i = pl.info
    assert (i.kind, i.ranks, i.encoding, i.jobs, i.chunk_size) == (8, p, e, p, chunk)
    assert pl.bytes_read == p * p * chunk and pl.bytes_written == 0
    assert plan(rd, codec, dev, stripes=[3, 5]).bytes_read == 2 * p * chunk
    lib = _lib.load()
    v = codec.plan_verify(dev.lofi(), dev.parity(), chunk, dev.stride)
    cells, stripes = (_lib.RepairCell * (p * p))(), (_lib.RepairStripe * p)()
    assert lib.redset_hip_plan_repair_report(v._h, None, cells, p * p, stripes, p) == _lib.REDSET_FAILURE
    assert b"not a repair plan" in lib.redset_hip_last_error()
    rows = (_lib.VerifyRow * (p * e))()
    assert lib.redset_hip_plan_verify_report(pl._h, None, rows, p * e, None) == _lib.REDSET_FAILURE
    assert b"not a verify plan" in lib.redset_hip_last_error()
    crcs = (_lib.c_uint * p)()
    assert lib.redset_hip_plan_crc32_report(pl._h, None, crcs, p) == _lib.REDSET_FAILURE
    assert b"not a CRC plan" in lib.redset_hip_last_error()
    assert lib.redset_hip_plan_repair_report(pl._h, None, cells, p, stripes, p) == _lib.REDSET_FAILURE  # too little room


@pytest.mark.parametrize("p,e,word", [(8, 1, "one parity row"), (12, 6, "2..4")])
def test_unsupported_shapes_fail_at_plan_time(rd, p, e, word):
    codec = rd.RSCodec(p, e)
    lay = rd.SetLayout.allocate(p, p - e, e, 64, device="cuda")
    with pytest.raises(rd.RedsetHipError, match=word):
        codec.plan_repair(lay.lofi_ptrs(), lay.parity_ptrs(), 64, lay.cell_stride)
    with pytest.raises(rd.RedsetHipError, match="one parity row"):
        rd.xor_plan_repair(p, lay.lofi_ptrs(), lay.parity_ptrs(), 64, lay.cell_stride)
