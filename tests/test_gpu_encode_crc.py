"""GPU tests of the fused encode + CRC-32 plans (include/redset_hip.h, "encode
and checksum in one read"). Every case fills a set whose stride padding holds
a sentinel, executes the plan once and compares the WHOLE device image with
the prediction -- data untouched, parity as tests/np_ref.py computes it, the
padding still the sentinel -- and every one of the p * p reported CRCs with
zlib.crc32 of that cell's bytes in the host copy, never with another kernel.

The kernel works on rows of 1 KiB in tiles of 128 KiB (256 segments of 512 B)
whose short tile comes first, each of a block's four waves walking 32 rows;
bytes past the last whole segment take a tail path, the last chunk % 16 of
them byte by byte. CHUNKS surrounds each of those edges."""
import zlib

import numpy as np
import pytest

import np_ref

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

SEG, TILE = 512, 512 * 256
SENTINEL = 0xA5
CHUNKS = [1, 15, 16, 17, 48, SEG - 16, SEG, SEG + 16, SEG + 17, 1024 + 16, 32768 - 16, 32768 + SEG, TILE - SEG, TILE,
          TILE + 16, TILE + SEG + 17, 2 * TILE - SEG - 3]
# NIN 2, 8, 16 (the combine in two chunks) and NOUT 1..4; e = 0 stands for the XOR scheme
SHAPES = [(3, 1), (4, 2), (11, 3), (12, 4), (17, 1), (20, 4), (2, 0), (8, 0), (17, 0)]
CASES = [(4, 2, ch, "random") for ch in CHUNKS] + \
        [(p, e, ch, "random") for p, e in SHAPES for ch in (SEG + 17, TILE + SEG + 17) if (p, e) != (4, 2)] + \
        [(4, 2, TILE + 16, "zero"), (4, 2, TILE + 16, "ff"),
         (4, 2, 65 * TILE + 16, "random")]  # the finish wave folds two tiles per lane


@pytest.fixture(scope="module")
def rd():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import redset_amd

    redset_amd.load()
    return redset_amd


@pytest.fixture(scope="module", autouse=True)
def no_faults(rd):
    yield
    torch.cuda.synchronize()
    assert (rd.ring_faults(clear=False), rd.hang_faults(clear=False)) == (0, 0)


def fill(kind, n, seed):
    if kind == "zero":
        return np.zeros(n, np.uint8)
    if kind == "ff":
        return np.full(n, 0xFF, np.uint8)
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8)


def layout(rd, p, e, chunk, kind="random", seed=1):
    """(device SetLayout, plan, expected host image [member, cell, stride]):
    the data cells filled, everything else the sentinel on the device; the
    expected image has the parity cells of np_ref."""
    ep = e or 1
    d = p - ep
    lay = rd.SetLayout.allocate(p, d, ep, chunk, pad=256)
    img = np.full((p, p, lay.cell_stride), SENTINEL, np.uint8)
    img[:, :d, :chunk] = fill(kind, p * d * chunk, seed).reshape(p, d, chunk)
    lay.storage.copy_(torch.from_numpy(img.reshape(-1)))
    lofi = [np.ascontiguousarray(img[r, :d, :chunk]).reshape(-1) for r in range(p)]
    want = img.copy()
    if e:
        parity = np_ref.rs_encode_set(p, e, lofi, chunk)
        plan = rd.RSCodec(p, e).plan_encode_crc32(lay.lofi_ptrs(), lay.parity_ptrs(), chunk, lay.cell_stride)
    else:
        parity = np_ref.xor_encode_set(p, lofi, chunk)
        plan = rd.xor_plan_encode_crc32(p, lay.lofi_ptrs(), lay.parity_ptrs(), chunk, lay.cell_stride)
    for r in range(p):
        want[r, d:, :chunk] = parity[r].reshape(ep, chunk)
    return lay, plan, want


def check(lay, plan, want, chunk):
    p = want.shape[0]
    torch.cuda.synchronize()
    got = lay.storage.cpu().numpy().reshape(want.shape)
    bad = np.argwhere(got != want)
    assert bad.size == 0, f"{len(bad)} bytes differ, first at [member, cell, offset] {bad[0].tolist()}"
    crcs = np.array([[zlib.crc32(want[r, c, :chunk].tobytes()) for c in range(p)] for r in range(p)], np.uint32)
    rep = plan.report()
    assert rep.shape == (p, p) and rep.dtype == np.uint32
    assert np.array_equal(rep, crcs), f"wrong CRCs at [member, cell] {np.argwhere(rep != crcs).tolist()}"


@pytest.mark.parametrize("p,e,chunk,kind", CASES, ids=[f"p{p}e{e}-c{ch}-{k}" for p, e, ch, k in CASES])
def test_encode_crc(rd, p, e, chunk, kind):
    lay, plan, want = layout(rd, p, e, chunk, kind)
    ep = e or 1
    assert (plan.info.kind, plan.info.jobs) == (13 if e else 14, p)
    assert (plan.bytes_read, plan.bytes_written) == (p * (p - ep) * chunk, p * ep * chunk)
    plan.execute()
    check(lay, plan, want, chunk)


def test_graph_replays_follow_the_data(rd):
    p, e, chunk = 4, 2, TILE + SEG + 17
    lay, plan, want = layout(rd, p, e, chunk)
    s = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):  # a linear chain: encode + tiles, finish
            plan.execute(s)
    torch.cuda.synchronize()
    g.replay()
    check(lay, plan, want, chunk)
    other, _, want2 = layout(rd, p, e, chunk, seed=2)
    lay.storage.copy_(other.storage)
    torch.cuda.synchronize()
    g.replay()
    check(lay, plan, want2, chunk)
    assert not np.array_equal(want, want2)


@pytest.mark.parametrize("p,e,shift", [(22, 4, 0), (12, 5, 0), (18, 0, 0), (4, 2, 1)])
def test_refused_at_plan_time(rd, p, e, shift):
    ep = e or 1
    lay = rd.SetLayout.allocate(p, p - ep, ep, 1024)
    lofi = [x + shift for x in lay.lofi_ptrs()]
    with pytest.raises(rd.RedsetHipError):
        if e:
            rd.RSCodec(p, e).plan_encode_crc32(lofi, lay.parity_ptrs(), 1024, lay.cell_stride)
        else:
            rd.xor_plan_encode_crc32(p, lofi, lay.parity_ptrs(), 1024, lay.cell_stride)
