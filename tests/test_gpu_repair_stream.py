"""GPU tests of redset_hip_rs_repair_stream over host memory (pageable and
pinned): the clean set is the CPU oracle's, the expected corrections the
brute-force numpy locate's (tests/repair_ref.py)."""
import numpy as np
import pytest

import repair_ref
from repair_ref import NO

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

CHUNK = (1 << 20) + 48
SLICE = 256 << 10


@pytest.fixture(scope="module")
def rd():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import redset_amd

    redset_amd.load()
    return redset_amd


_images = {}


def clean_image(oracle, p, e):
    """[p, d + e, stride] host bytes of an encoded set (stride = chunk rounded to 256)."""
    if (p, e) not in _images:
        d = p - e
        lofi, parity = oracle.random_set(p, d, e, CHUNK, seed=700 + p)
        oracle.OracleRS(p, e).encode_set(lofi, parity, CHUNK)
        img = np.full((p, d + e, -(-CHUNK // 256) * 256), 0xA5, np.uint8)
        for r in range(p):
            img[r, :d, :CHUNK] = lofi[r].reshape(d, CHUNK)
            img[r, d:, :CHUNK] = parity[r].reshape(e, CHUNK)
        img.setflags(write=False)
        _images[(p, e)] = img
    return _images[(p, e)]


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


def damage(oracle, codec, clean, spots):
    """spots: (stripe, member, first column, length). Returns the damaged image
    and the damaged columns per stripe."""
    rng = np.random.default_rng(5)
    img = clean.copy()
    cols = {}
    for c, m, a, n in spots:
        st = repair_ref.Stripe(oracle, codec, c)
        img[m, st.index[m], a:a + n] ^= rng.integers(1, 256, n, dtype=np.uint8)
        cols.setdefault(c, []).extend(range(a, a + n))
    return img, cols


@pytest.mark.parametrize("pinned", [False, True])
@pytest.mark.parametrize("p,e", [(4, 2), (11, 3)])
def test_repair_stream_restores_the_set(rd, oracle, p, e, pinned):
    clean = clean_image(oracle, p, e)
    codec = rd.RSCodec(p, e)
    # stripe 1: member 0 across the first slice boundary, member 2 inside slice 3,
    # member 3 in the 48-byte last slice; stripe 3: one byte of member 1
    spots = [(1, 0, SLICE - 100, 300), (1, 2, 3 * SLICE + 7, 1000), (1, 3, CHUNK - 40, 30), (3, 1, 12345, 1)]
    img, cols = damage(oracle, codec, clean, spots)
    want_c, want_f = np.zeros((p, p), np.uint64), np.full((p, p), NO, np.uint64)
    fixed = img.copy()
    for c in cols:
        st = repair_ref.Stripe(oracle, codec, c)
        want_c[c], want_f[c], un, _, fixes = repair_ref.predict(st, img, CHUNK, cols[c])
        assert un == 0
        repair_ref.apply_fixes(st, fixed, fixes)
    assert np.array_equal(fixed, clean)
    nslices = -(-CHUNK // SLICE)
    for apply in (False, True):
        t, io = host_set(rd, img, e, pinned)
        res = rd.rs_repair_stream(codec, CHUNK, io, slice_bytes=SLICE, apply=apply)
        io.close()
        assert np.array_equal(res["corrected"], want_c) and np.array_equal(res["first"], want_f)
        assert not res["unlocated"].any() and (res["first_unlocated"] == NO).all()
        assert res["damaged_stripes"] == 2 and res["repair_units"] == 2 * nslices
        assert res["corrected_bytes"] == 1331 and res["unlocated_columns"] == 0
        assert res["verify_mismatch_bytes"] > 0
        got = t.numpy().reshape(clean.shape)
        if apply:
            # (cell, slice) pairs that held damage: member 0 in slices 0 and 1, then one each
            assert res["cells_written"] == 5 and res["remaining_mismatch_bytes"] == 0
            assert np.array_equal(got, clean)
        else:
            assert res["cells_written"] == 0 and res["remaining_mismatch_bytes"] == res["verify_mismatch_bytes"]
            assert np.array_equal(got, img)


def test_clean_set_and_stripe_window(rd, oracle):
    p, e = 4, 2
    clean = clean_image(oracle, p, e)
    codec = rd.RSCodec(p, e)
    t, io = host_set(rd, clean, e, False)
    res = rd.rs_repair_stream(codec, CHUNK, io, slice_bytes=SLICE)
    assert res["repair_units"] == 0 and res["damaged_stripes"] == 0 and res["verify_mismatch_bytes"] == 0
    assert res["cells_written"] == 0 and not res["corrected"].any()
    io.close()
    assert np.array_equal(t.numpy().reshape(clean.shape), clean)
    # damage in stripes 0 and 2; the window [2, 4) repairs and reports stripe 2 only
    img, cols = damage(oracle, codec, clean, [(0, 1, 500, 20), (2, 3, 70000, 64)])
    t, io = host_set(rd, img, e, False)
    res = rd.rs_repair_stream(codec, CHUNK, io, first=2, nstripes=2, slice_bytes=SLICE)
    io.close()
    assert res["corrected"].shape == (2, p) and int(res["corrected"][0, 3]) == 64 and int(res["corrected"].sum()) == 64
    assert int(res["first"][0, 3]) == 70000 and res["damaged_stripes"] == 1 and res["cells_written"] == 1
    st0 = repair_ref.Stripe(oracle, codec, 0)
    want = clean.copy()
    want[1, st0.index[1], 500:520] = img[1, st0.index[1], 500:520]  # stripe 0 stays damaged
    assert np.array_equal(t.numpy().reshape(clean.shape), want)
