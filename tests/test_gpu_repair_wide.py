"""GPU tests of the wide repair (include/redset_hip.h, "repair_wide";
gf_repair_wide_kernel<E>, E = 5..8). The reference is the undamaged set: the
oracle encodes it, the test XORs chosen nonzero values into chosen cells, and
a column with at most max_errors wrong bytes must come back as it was. After
an apply execute the WHOLE device allocation, sentinel padding included, must
equal the clean image except in the columns with t + 1 wrong bytes, each of
which is either untouched and counted unlocated or has a zero syndrome; the
reports must be what the injected damage implies, and a dry run gives them
already and changes nothing.

Chunk 4117 = 257 vectors + 5 tail bytes (more than one 256-lane step);
(40, 6) has d > 16; `shift` starts the image one byte off alignment, which
puts every job on the byte path; (248, 8) at chunk 48 is the largest table set
in LDS (66816 B a block)."""
import numpy as np
import pytest

import repair_ref
import repair_wide_ref as ref
from repair_ref import NO
from test_gpu_repair import SENTINEL, Dev, clean_image
from test_gpu_repair_setfiles import make_set, read, xor_at

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

CASES = [(8, 5, 4117, 0), (10, 6, 4117, 0), (12, 7, 4117, 0), (12, 8, 4117, 0), (40, 6, 4117, 0), (10, 6, 4117, 1),
         (248, 8, 48, 1)]


@pytest.fixture(scope="module")
def rd():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import redset_amd

    redset_amd.load()
    return redset_amd


@pytest.fixture(scope="module", autouse=True)
def fault_counts_unchanged(rd):
    torch.cuda.synchronize()
    before = (rd.ring_faults(clear=False), rd.hang_faults(clear=False))
    yield
    torch.cuda.synchronize()
    assert (rd.ring_faults(clear=False), rd.hang_faults(clear=False)) == before


def damage(oracle, codec, clean, chunk):
    """In stripes 0, e (member 0 holds data: the point 0) and p - 1: runs of 1,
    16 and 300 columns (as far as the chunk goes) in which wrong member i of t
    starts i * len // 8 columns into the run, so nu goes 1..t along it; one
    wrong byte in the last column; and columns with t + 1 wrong bytes.
    -> (image, {stripe: (wrong[p, chunk] bool, hard columns)})"""
    p, e = codec.ranks, codec.encoding
    t = e // 2
    rng = np.random.default_rng(p + e + chunk)
    img, plan = clean.copy(), {}
    runs = [(5, 1), (1003, 16), (2000, 300)] if chunk > 2400 else [(5, 1), (9, 16)]
    hard = [3000, 3001, chunk - 3] if chunk > 3100 else [40]
    for c in (0, e, p - 1):
        st = repair_ref.Stripe(oracle, codec, c)
        data, par = ref.members_of(st)
        mem = [data[0], par[0], data[-1], par[-1], data[1]][:t + 1]
        wrong = np.zeros((p, chunk), bool)
        for x0, n in runs:
            for i, m in enumerate(mem[:t]):
                wrong[m, x0 + i * n // 8:x0 + n] = True
        wrong[mem[0], chunk - 1] = True
        for col in hard:
            wrong[mem, col] = True
        for m in range(p):
            cols = np.nonzero(wrong[m])[0]
            img[m, st.index[m], cols] ^= rng.integers(1, 256, cols.size, dtype=np.uint8)
        plan[c] = (wrong, hard)
    return img, plan


def device(img, chunk, e, shift):
    dev = Dev(img, chunk, e)
    if shift:
        dev.buf.fill_(SENTINEL)
        dev.off += shift
        dev.upload(img)
    return dev


def make_plan(codec, dev, **kw):
    return codec.plan_repair_wide(dev.lofi(), dev.parity(), dev.chunk, dev.stride, **kw)


def run(pl):
    pl.execute()
    torch.cuda.synchronize()
    return pl.report()


def check(oracle, codec, clean, img, plan, dev, report, max_errors):
    """The device image and the report against what the damage implies."""
    p, chunk = codec.ranks, dev.chunk
    got = dev.download()[dev.off:dev.off + img.size].reshape(img.shape)
    corrected, first = np.zeros((p, p), np.uint64), np.full((p, p), NO, np.uint64)
    unloc, first_un, multi = np.zeros(p, np.uint64), np.full(p, NO, np.uint64), np.zeros((p, 3), np.uint64)
    want = clean.copy()
    for c, (wrong, hard) in plan.items():
        st = repair_ref.Stripe(oracle, codec, c)
        nu = wrong.sum(axis=0)
        fixed = (nu > 0) & (nu <= max_errors)
        for col in np.nonzero(nu > max_errors)[0].tolist():
            cell = (np.arange(p), st.index, col)
            want[cell] = got[cell]
            changed = got[cell] != img[cell]
            if changed.any():  # only past the distance: another codeword
                assert col in hard and not any(ref.syndrome_of(st, list(zip(range(p), got[cell]))))
                wrong[:, col], nu[col], fixed[col] = changed, changed.sum(), True
            else:
                unloc[c] += 1
                first_un[c] = min(int(first_un[c]), col)
        for m in range(p):
            cols = np.nonzero(wrong[m] & fixed)[0]
            if cols.size:
                corrected[c, m], first[c, m] = cols.size, cols.min()
        for k in (2, 3, 4):
            multi[c, k - 2] = np.count_nonzero(fixed & (nu == k))
    assert np.array_equal(dev.download(), dev.expect(want))
    for g, w, name in zip(report, (corrected, first, unloc, first_un, multi),
                          ("corrected", "first", "unlocated", "first_unlocated", "multi_columns")):
        assert np.array_equal(g, w), f"{name}: got {g.tolist()} want {w.tolist()}"


@pytest.mark.parametrize("p,e,chunk,shift", CASES)
def test_dry_run_then_apply(rd, oracle, p, e, chunk, shift):
    clean = clean_image(oracle, p, e, chunk, chunk < 256)
    codec = rd.RSCodec(p, e)
    img, plan = damage(oracle, codec, clean, chunk)
    dev = device(img, chunk, e, shift)
    dry = make_plan(codec, dev, apply=False)
    assert (dry.info.kind, dry.info.jobs, dry.bytes_read, dry.bytes_written) == (11, p, p * p * chunk, 0)
    rep_dry = run(dry)
    assert np.array_equal(dev.download(), dev.expect(img))  # no byte modified
    rep = run(make_plan(codec, dev))
    for a, b in zip(rep_dry, rep):
        assert np.array_equal(a, b)
    assert rep[4][e, e // 2 - 2] > 0  # columns with t wrong bytes were corrected
    check(oracle, codec, clean, img, plan, dev, rep, e // 2)


def test_max_errors_1_leaves_the_multi_columns(rd, oracle):
    p, e, chunk = 10, 6, 4117
    clean = clean_image(oracle, p, e, chunk, False)
    codec = rd.RSCodec(p, e)
    img, plan = damage(oracle, codec, clean, chunk)
    dev = device(img, chunk, e, 0)
    rep = run(make_plan(codec, dev, max_errors=1))
    assert rep[2][0] > 200 and not rep[4].any()  # the nu >= 2 columns of the runs
    check(oracle, codec, clean, img, plan, dev, rep, 1)


def test_graph_capture_replays(rd, oracle):
    p, e, chunk = 12, 8, 4117
    clean = clean_image(oracle, p, e, chunk, False)
    codec = rd.RSCodec(p, e)
    img, plan = damage(oracle, codec, clean, chunk)
    dev = device(img, chunk, e, 0)
    eager = run(make_plan(codec, dev, apply=False))
    pl = make_plan(codec, dev, apply=False)
    s = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):  # a linear chain: reset, repair
            pl.execute(s)
    for _ in range(3):
        g.replay()
        torch.cuda.synchronize()
        for a, b in zip(pl.report(), eager):
            assert np.array_equal(a, b)
    assert eager[0].any() and np.array_equal(dev.download(), dev.expect(img))


def test_stream_over_host_memory(rd, oracle):
    from redset_amd import stream

    p, e, chunk = 10, 6, 4117
    d = p - e
    clean = clean_image(oracle, p, e, chunk, False)
    codec = rd.RSCodec(p, e)
    img, plan = damage(oracle, codec, clean, chunk)
    for c in plan:  # the columns past t are not this test's
        st = repair_ref.Stripe(oracle, codec, c)
        for col in plan[c][1]:
            img[np.arange(p), st.index, col] = clean[np.arange(p), st.index, col]

    def host(image):
        lofi = [np.ascontiguousarray(image[r, :d, :chunk]).reshape(-1) for r in range(p)]
        parity = [np.ascontiguousarray(image[r, d:, :chunk]).reshape(-1) for r in range(p)]
        return lofi, parity, stream.HostIO(p, [x.ctypes.data for x in lofi], [x.ctypes.data for x in parity], chunk,
                                            keepalive=(lofi, parity))

    _, _, io = host(clean)
    res = rd.rs_repair_wide_stream(codec, chunk, io, slice_bytes=2048)
    assert (res["repair_units"], res["verify_mismatch_bytes"], res["cells_written"]) == (0, 0, 0)
    io.close()
    lofi, parity, io = host(img)
    res = rd.rs_repair_wide_stream(codec, chunk, io, slice_bytes=2048)
    io.close()
    assert res["damaged_stripes"] == 3 and res["remaining_mismatch_bytes"] == 0 and res["unlocated_columns"] == 0
    assert res["multi_columns"][0] > 0 and res["multi_columns"][1] > 0 and res["multi_columns"][2] == 0
    want_l, want_p, io = host(clean)
    io.close()
    assert all(np.array_equal(a, b) for a, b in zip(lofi + parity, want_l + want_p))


def test_repair_set_files_with_checksums(rd, oracle, tmp_path):
    from redset_amd import setfiles as sf

    p, e = 10, 6
    members, res = make_set(sf, str(tmp_path), k=e, checksums=True, sizes=[[9000]] * 8 + [[5000, 3999], [8000]])
    reds, hs, chunk = res["redundancy"], res["header_bytes"], res["chunk"]
    everything = [f for fl in members for f in fl] + reds
    saved = {f: read(f) for f in everything}
    st = repair_ref.Stripe(oracle, rd.RSCodec(p, e), 1)
    data, par = ref.members_of(st)
    a, b, c = [m for m in data if m < 8][:2] + [par[0]]
    # 40 columns wrong in two data cells and a parity cell of stripe 1, 10 more in the first data cell alone
    xor_at(members[a][0], st.index[a] * chunk + 300, [0x5A] * 50)
    xor_at(members[b][0], st.index[b] * chunk + 300, list(range(101, 141)))
    xor_at(reds[c], hs[c] + st.row[c] * chunk + 300, list(range(1, 41)))
    with pytest.raises(ValueError, match="2..4"):
        sf.repair_set(reds)
    out = sf.repair_set(reds, checksums=True, wide=True, max_errors=None)
    assert out["repaired"] and out["multi_columns"] == [0, 40, 0] and out["corrected_bytes"] == 130
    assert out["unlocated_columns"] == 0 and out["checksum_damaged"] == []
    assert {f: read(f) for f in everything} == saved


def test_other_encodings_raise(rd, tmp_path):
    from redset_amd import setfiles as sf

    with pytest.raises(ValueError, match="5..8"):
        sf.repair_set(make_set(sf, str(tmp_path), k=3, sizes=[[500]] * 11)[1]["redundancy"], wide=True)
    codec = rd.RSCodec(20, 4)
    lay = rd.SetLayout.allocate(20, 16, 4, 64, device="cuda")
    with pytest.raises(ValueError, match="5..8"):
        codec.plan_repair_wide(lay.lofi_ptrs(), lay.parity_ptrs(), 64, lay.cell_stride)
    with pytest.raises(ValueError, match="1..3"):
        rd.RSCodec(10, 6).plan_repair_wide(lay.lofi_ptrs(), lay.parity_ptrs(), 64, lay.cell_stride, max_errors=4)
