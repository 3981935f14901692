"""GPU tests of redset_hip_rs_rebuild_checked_stream over host memory
(HostIO, pageable and pinned): the set before loss and damage is the CPU
oracle's, the expected corrections the brute-force reference's
(tests/rebuild_checked_ref.py). Chunks of a few KiB, a slice smaller than the
chunk and a chunk that is no multiple of the slice."""
import numpy as np
import pytest

import rebuild_checked_ref as ref

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

SLICE = 1024
# (p, e, lost, chunk): 5000 = 4 slices of 1024 and 904 bytes; 4096 = 4 whole slices
CASES = [(6, 4, [2], 5000), (6, 4, [1, 4], 5000), (5, 3, [3], 4096)]


@pytest.fixture(scope="module")
def rd():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import redset_amd

    redset_amd.load()
    return redset_amd


def host_set(rd, img, e, pinned):
    """The image in one host tensor and a HostIO over it."""
    p, cells, stride = img.shape
    t = torch.from_numpy(img.copy().reshape(-1))
    if pinned:
        t = t.pin_memory()
    base = t.data_ptr()
    lofi = [base + r * cells * stride for r in range(p)]
    parity = [x + (cells - e) * stride for x in lofi]
    return t, rd.stream.HostIO(p, lofi, parity, stride, keepalive=(t,), pinned=pinned)


def damage(oracle, codec, clean, lost, chunk):
    """One wrong byte per column: in stripe 0 a run across the first slice
    boundary in one survivor and the last byte in another; in stripe p - 1
    one byte in the last, short slice."""
    rng = np.random.default_rng(chunk)
    img = clean.copy()
    cols = {}
    p = codec.ranks
    st = ref.Stripe(oracle, codec, 0, lost)
    m = st.surv[0]
    img[m, st.index[m], SLICE - 20:SLICE + 30] ^= rng.integers(1, 256, 50, dtype=np.uint8)
    m = st.surv[-1]
    img[m, st.index[m], chunk - 1] ^= 0x81
    cols[0] = list(range(SLICE - 20, SLICE + 30)) + [chunk - 1]
    st = ref.Stripe(oracle, codec, p - 1, lost)
    m = st.surv[1]
    img[m, st.index[m], chunk - 7] ^= 0x10
    cols[p - 1] = [chunk - 7]
    return img, cols


@pytest.mark.parametrize("pinned", [False, True])
@pytest.mark.parametrize("p,e,lost,chunk", CASES)
def test_rebuild_checked_stream(rd, oracle, p, e, lost, chunk, pinned):
    clean = ref.clean_image(oracle, p, e, chunk)
    codec = rd.RSCodec(p, e)
    img, cols = damage(oracle, codec, clean, lost, chunk)
    want, kept, fixed = ref.predict_set(oracle, codec, img, lost, chunk, cols)
    assert np.array_equal(fixed, clean) and int(want[0].sum()) == 52 and not want[2].any()
    start = ref.lose(img, lost, chunk)
    # the plain rebuild stream inherits the survivors' errors: the point of the feature
    t, io = host_set(rd, start, e, pinned)
    rd.stream.rs_rebuild_stream(codec, lost, chunk, io, slice_bytes=SLICE)
    io.close()
    plain = t.numpy().reshape(img.shape)
    assert np.array_equal(plain, ref.oracle_rebuild(oracle, img, e, lost, chunk))
    assert not np.array_equal(plain[lost], clean[lost])
    for fix, expect in ((False, kept), (True, fixed)):
        t, io = host_set(rd, start, e, pinned)
        out = rd.rs_rebuild_checked_stream(codec, lost, chunk, io, slice_bytes=SLICE, fix_survivors=fix)
        io.close()
        for got, w, name in zip((out["corrected"], out["first"], out["unlocated"], out["first_unlocated"]), want,
                                ("corrected", "first", "unlocated", "first_unlocated")):
            assert np.array_equal(got, w), name
        assert np.array_equal(t.numpy().reshape(img.shape), expect), f"fix_survivors={fix}"  # padding included
        nslices = -(-chunk // SLICE)
        assert out["corrected_bytes"] == 52 and out["unlocated_columns"] == 0 and out["stripes_with_findings"] == 2
        # every rebuilt slice, plus (fix) the corrected survivor slices: two of the run, the last-byte one, stripe p-1's
        assert out["cells_written"] == p * len(lost) * nslices + (4 if fix else 0)
        assert out["stats"]["bytes_read"] == p * (p - len(lost)) * chunk
        assert out["stats"]["units"] == p * nslices


def test_stripe_range_detect_only_and_refusals(rd, oracle):
    p, e, lost, chunk = 5, 3, [0, 3], 4096
    clean = ref.clean_image(oracle, p, e, chunk)
    codec = rd.RSCodec(p, e)
    img = clean.copy()
    st = ref.Stripe(oracle, codec, 2, lost)
    m = st.surv[0]
    img[m, st.index[m], 2000:2010] ^= 0x55
    want, kept, fixed = ref.predict_set(oracle, codec, img, lost, chunk, {2: range(2000, 2010)})
    assert int(want[2][2]) == 10 and np.array_equal(kept, fixed)  # one check row: detected, never located
    start = ref.lose(img, lost, chunk)
    t, io = host_set(rd, start, e, False)
    out = rd.rs_rebuild_checked_stream(codec, lost, chunk, io, first=2, nstripes=2, slice_bytes=SLICE,
                                       fix_survivors=True)
    assert out["unlocated"].tolist() == [10, 0] and out["first_unlocated"][0] == 2000 and not out["corrected"].any()
    assert out["unlocated_columns"] == 10 and out["stripes_with_findings"] == 1
    got = t.numpy().reshape(img.shape)
    for c in range(p):  # stripes 2 and 3 rebuilt (the plain rebuild's bytes), the others untouched
        stc = ref.Stripe(oracle, codec, c, lost)
        for r in lost:
            expect = kept if c in (2, 3) else start
            assert np.array_equal(got[r, stc.index[r]], expect[r, stc.index[r]]), (c, r)
    assert np.array_equal(np.delete(got, lost, axis=0), np.delete(img, lost, axis=0))  # no survivor byte written
    with pytest.raises(rd.RedsetHipError, match="stripe range"):
        rd.rs_rebuild_checked_stream(codec, lost, chunk, io, first=4, nstripes=2)
    with pytest.raises(rd.RedsetHipError, match="nothing left to check"):
        rd.rs_rebuild_checked_stream(codec, [0, 1, 3], chunk, io)
    io.close()
