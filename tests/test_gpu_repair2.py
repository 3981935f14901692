"""GPU tests of repair plans with max_errors=2 (include/redset_hip.h,
"repair2"; gf_repair2_kernel): the clean set comes from the CPU oracle, the
expected verdict of every damaged byte column from the brute-force numpy
locate of tests/repair2_ref.py. After an apply execute the WHOLE device
allocation, sentinel padding included, must equal the prediction byte for
byte, and the cell, stripe and pair reports the predicted counts and first
offsets exactly; a dry run gives the same report and leaves every byte.

(6, 4) has d = 2, (20, 4) is the bench's widest set, (40, 4) has d > 32 (the
table build loops). Chunk 37 packed leaves every cell unaligned (byte path);
4096 + 7 padded is vectors plus a tail."""
import numpy as np
import pytest

import repair2_ref
import repair_ref
from repair_ref import NO
from test_gpu_repair import Dev, clean_image
from test_gpu_repair_setfiles import make_set, read, xor_at

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

E = 4
CASES = [(p, chunk, packed) for p in (6, 20, 40) for chunk, packed in ((37, True), (4096 + 7, False))]


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


def damage(oracle, codec, clean, chunk, triples=True):
    """The clean image with, in stripe 0 (member 0 holds parity: point 0 is
    shortened) and stripe 4 (member 0 holds data: X = 0), single errors, pairs
    of every kind with random and with equal values, and columns with three
    wrong bytes, spread over the vector lanes and repeated in the tail; long
    cells also get a 64-column run damaged in two members.
    -> (image, {stripe: damaged columns}, the columns with three wrong bytes)"""
    p = codec.ranks
    rng = np.random.default_rng(p + chunk)
    img, cols_of, hard = clean.copy(), {}, set()
    for c in (0, E):
        st = repair_ref.Stripe(oracle, codec, c)
        data, par = [m for m in range(p) if st.row[m] < 0], [m for m in range(p) if st.row[m] >= 0]
        kinds = [(data[0], data[1]), (data[0], par[0]), (par[0], par[-1]), (data[-1], par[1])]
        pats = [(data[-1],), (par[2],)]
        pats += [k + (eq,) for k in kinds for eq in ("random", "equal")]
        pats += [(data[0], data[1], par[3]), (data[-1], par[0], par[1])] if triples else []
        nvec16 = chunk // 16 * 16
        where = np.linspace(0, nvec16 - 1, len(pats)).astype(int).tolist() + list(range(nvec16, chunk))
        for col, pat in zip(where, pats + pats[2:]):
            mem = [m for m in pat if not isinstance(m, str)]
            x = rng.integers(1, 256, len(mem), dtype=np.uint8)
            if pat[-1] == "equal":
                x[:] = x[0]
            for m, v in zip(mem, x):
                img[m, st.index[m], col] ^= v
            if len(mem) == 3:
                hard.add(col)
        cols_of[c] = where + (list(range(1000, 1064)) if chunk > 2000 else [])
        if chunk > 2000:
            for m in (data[0], par[1]):
                img[m, st.index[m], 1000:1064] ^= rng.integers(1, 256, 64, dtype=np.uint8)
    return img, cols_of, hard


def predict_all(oracle, codec, img, chunk, cols_of):
    p = codec.ranks
    corrected, first = np.zeros((p, p), np.uint64), np.full((p, p), NO, np.uint64)
    unloc, first_un, pairs = np.zeros(p, np.uint64), np.full(p, NO, np.uint64), np.zeros(p, np.uint64)
    fixed = img.copy()
    for c, cols in cols_of.items():
        st = repair_ref.Stripe(oracle, codec, c)
        (corrected[c], first[c], unloc[c], first_un[c], pairs[c]), fixes = repair2_ref.predict(st, img, chunk, cols)
        repair2_ref.apply_fixes(st, fixed, fixes)
    return (corrected, first, unloc, first_un, pairs), fixed


def check_report(got, want):
    for g, w, name in zip(got, want, ("corrected", "first", "unlocated", "first_unlocated", "pair_columns")):
        assert np.array_equal(g, w), f"{name}: got {g.tolist()} want {w.tolist()}"


def run(pl):
    pl.execute()
    torch.cuda.synchronize()
    return pl.report()


def plan(codec, dev, **kw):
    return codec.plan_repair(dev.lofi(), dev.parity(), dev.chunk, dev.stride, **kw)


@pytest.mark.parametrize("p,chunk,packed", CASES)
def test_dry_run_then_apply(rd, oracle, p, chunk, packed):
    clean = clean_image(oracle, p, E, chunk, packed)
    codec = rd.RSCodec(p, E)
    img, cols_of, hard = damage(oracle, codec, clean, chunk)
    want, fixed = predict_all(oracle, codec, img, chunk, cols_of)
    # the oracle alone: pairs are found in both stripes, and only three-error columns may
    # stay wrong (unlocated, or miscorrected into a pair)
    assert want[4][0] >= 8 and want[4][E] >= 8
    assert set(np.nonzero((fixed != clean).any(axis=(0, 1)))[0].tolist()) <= hard
    dev = Dev(img, chunk, E)
    dry = plan(codec, dev, apply=False, max_errors=2)
    assert (dry.info.kind, dry.info.jobs, dry.bytes_read, dry.bytes_written) == (10, p, p * p * chunk, 0)
    check_report(run(dry), want)
    assert np.array_equal(dev.download(), dev.expect(img))  # no byte modified
    check_report(run(plan(codec, dev, max_errors=2)), want)
    assert np.array_equal(dev.download(), dev.expect(fixed))


def test_max_errors_1_leaves_exactly_the_pair_columns(rd, oracle):
    p, chunk = 20, 4096 + 7
    clean = clean_image(oracle, p, E, chunk, False)
    codec = rd.RSCodec(p, E)
    img, cols_of, _ = damage(oracle, codec, clean, chunk, triples=False)
    want, fixed = predict_all(oracle, codec, img, chunk, cols_of)
    assert np.array_equal(fixed, clean) and not want[2].any() and want[4][0] > 64 and want[4][E] > 64
    dev = Dev(img, chunk, E)
    one = run(plan(codec, dev, apply=False))
    assert np.array_equal(one[2], want[4]) and np.array_equal(one[0].sum(axis=1), want[0].sum(axis=1) - 2 * want[4])
    check_report(run(plan(codec, dev, max_errors=2)), want)
    assert np.array_equal(dev.download(), dev.expect(clean))


def test_graph_capture_replays(rd, oracle):
    p, chunk = 6, 4096 + 7
    clean = clean_image(oracle, p, E, chunk, False)
    codec = rd.RSCodec(p, E)
    img, cols_of, _ = damage(oracle, codec, clean, chunk)
    want, fixed = predict_all(oracle, codec, img, chunk, cols_of)
    dev = Dev(img, chunk, E)
    pl = plan(codec, dev, max_errors=2)
    s = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):  # a linear chain: reset, repair
            pl.execute(s)
    for _ in range(3):
        dev.upload(img)  # a freshly damaged copy, whatever the capture or the last replay did
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        check_report(pl.report(), want)
        assert np.array_equal(dev.download(), dev.expect(fixed))


def test_repair_set_files_with_checksums(rd, oracle, tmp_path):
    from redset_amd import setfiles as sf

    p = 6
    members, res = make_set(sf, str(tmp_path), k=E, checksums=True, sizes=[[9000]] * 4 + [[5000, 3999], [8000]])
    reds, hs, chunk = res["redundancy"], res["header_bytes"], res["chunk"]
    everything = [f for fl in members for f in fl] + reds
    saved = {f: read(f) for f in everything}
    st = repair_ref.Stripe(oracle, rd.RSCodec(p, E), 1)
    a = next(m for m in range(4) if st.row[m] < 0)
    b = next(m for m in range(p) if st.row[m] >= 0)
    # 40 columns wrong in a data cell and in a parity cell of stripe 1, 10 more in the data cell alone
    xor_at(members[a][0], st.index[a] * chunk + 300, [0x5A] * 50)
    xor_at(reds[b], hs[b] + st.row[b] * chunk + 300, list(range(1, 41)))
    with pytest.raises(ValueError, match="e = 4"):
        sf.repair_set(make_set(sf, str(tmp_path / "e3"), k=3, sizes=[[500]] * 11)[1]["redundancy"], max_errors=2)
    first = sf.repair_set(reds, apply=False)
    assert first["unlocated_columns"] == 40 and first["corrected_bytes"] == 10 and "pair_columns" not in first
    out = sf.repair_set(reds, checksums=True, max_errors=2)
    assert out["repaired"] and out["pair_columns"] == 40 and out["corrected_bytes"] == 90
    assert out["unlocated_columns"] == 0 and out["checksum_damaged"] == []
    assert {f: read(f) for f in everything} == saved


def test_other_encodings_raise(rd):
    codec = rd.RSCodec(11, 3)
    lay = rd.SetLayout.allocate(11, 8, 3, 64, device="cuda")
    with pytest.raises(ValueError, match="e = 4"):
        codec.plan_repair(lay.lofi_ptrs(), lay.parity_ptrs(), 64, lay.cell_stride, max_errors=2)
    io = rd.stream.HostIO(11, [0x1000] * 11, [0x1000] * 11, 64)  # never dereferenced: refused first
    with pytest.raises(ValueError, match="e = 4"):
        rd.rs_repair_stream(codec, 64, io, max_errors=2)
    io.close()
