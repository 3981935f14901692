"""GPU tests of the fused verify + CRC-32 plans (include/redset_hip.h, "scrub
and checksum in one read"). Every expectation comes from the host: the parity
of tests/np_ref.py against the stored parity of the host image gives the report
rows -- row [c * e + i] is the parity cell of member (c - i) mod p, one row a
stripe for XOR -- and zlib.crc32 of the stored bytes gives the p * p CRCs; never
another kernel. Every case also compares the whole device image, stride padding
of sentinels included, with what was uploaded: the plan writes no byte of it.

The kernel works on rows of 1 KiB in tiles of 128 KiB (256 segments of 512 B)
whose short tile comes first, each of a block's four waves walking 32 rows;
bytes past the last whole segment take a tail path, the last chunk % 16 of them
byte by byte. At TILE + SEG + 17 the first tile is one segment: half a row, the
other half's lanes working at vector 0 with nothing to count."""
import functools
import zlib

import numpy as np
import pytest

import np_ref

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

SEG, TILE = 512, 512 * 256
SENTINEL = 0xA5
BIG = TILE + SEG + 17
# e = 0 stands for the XOR scheme; (20, 4): 16 inputs, loaded in two chunks
CLEAN = [(4, 2, ch) for ch in (1, 17, SEG - 16, SEG + 17, TILE, BIG, 2 * TILE - SEG - 3)] + \
        [(p, e, ch) for p, e in [(3, 1), (11, 3), (12, 4), (20, 4), (2, 0), (8, 0), (17, 0)] for ch in (SEG + 17, BIG)]
DAMAGED = [(4, 2, BIG), (11, 3, BIG), (20, 4, BIG), (8, 0, BIG), (4, 2, SEG + 17), (4, 2, 17)]


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


def encode(p, e, img, chunk):
    """the parity of the image's data cells, [member, slot, chunk]"""
    d = p - (e or 1)
    lofi = [np.ascontiguousarray(img[r, :d, :chunk]).reshape(-1) for r in range(p)]
    parity = np_ref.rs_encode_set(p, e, lofi, chunk) if e else np_ref.xor_encode_set(p, lofi, chunk)
    return np.stack(parity).reshape(p, e or 1, chunk)


@functools.lru_cache(maxsize=None)
def clean_image(p, e, chunk, stride):
    """(host image [member, cell, stride] of a clean set, its parity): the
    data cells random, the parity cells np_ref's, the padding the sentinel"""
    d = p - (e or 1)
    img = np.full((p, p, stride), SENTINEL, np.uint8)
    img[:, :d, :chunk] = np.random.default_rng(p + e).integers(0, 256, (p, d, chunk), dtype=np.uint8)
    parity = encode(p, e, img, chunk)
    img[:, d:, :chunk] = parity
    img.setflags(write=False)
    return img, parity


def layout(rd, p, e, chunk):
    """(device SetLayout holding the clean image, plan, clean image, its parity)"""
    ep = e or 1
    lay = rd.SetLayout.allocate(p, p - ep, ep, chunk, pad=256)
    img, parity = clean_image(p, e, chunk, lay.cell_stride)
    lay.storage.copy_(torch.from_numpy(img.reshape(-1).copy()))
    if e:
        plan = rd.RSCodec(p, e).plan_verify_crc32(lay.lofi_ptrs(), lay.parity_ptrs(), chunk, lay.cell_stride)
    else:
        plan = rd.xor_plan_verify_crc32(p, lay.lofi_ptrs(), lay.parity_ptrs(), chunk, lay.cell_stride)
    return lay, plan, img, parity


def data_cell(p, e, c, k):
    """(member, cell) of the k-th data member of stripe c"""
    if not e:
        s = [s for s in range(p) if s != c][k]
        return s, (c if c < s else c - 1)
    s = [s for s in range(p) if np_ref.encoding_id(p, e, s, c) < p][k]
    return s, np_ref.data_id(p, e, s, c)


def damage(img, p, e, chunk):
    """(a damaged copy, {stripe: (member, first offset)} of the stripes with one
    damaged data member). Stripe 0: a data cell at offset 0 (the duplicated half
    row's vector), one row on in the same lane column, and another lane of the
    first row. Stripe 1: its last parity row's cell at the last byte of the
    first tile and the first of the second. Stripe 2: a data cell just before
    the tail, in the vector tail and in the byte tail."""
    ep = e or 1
    bad = img.copy()
    hits = {0: (data_cell(p, e, 0, 0), [0, 83, 1024]),
            1: (((1 - (ep - 1)) % p, p - 1), [SEG - 1, SEG] if chunk > SEG else [chunk // 2]),
            2: (data_cell(p, e, 2, 1), [chunk - 18, chunk - 2, chunk - 1])}
    located = {}
    for c, ((m, cell), offs) in hits.items():
        offs = [o for o in offs if 0 <= o < chunk]
        bad[m, cell, offs] ^= 0x5A
        if c != 1:
            located[c] = (m, min(offs))
    return bad, located


def check(rd, lay, plan, img, p, e, chunk, parity=None):
    """report rows, CRCs and the untouched device image against the host image"""
    ep, d = e or 1, p - (e or 1)
    parity = encode(p, e, img, chunk) if parity is None else parity
    mism = np.zeros((p, ep), np.uint64)
    first = np.full((p, ep), rd.codec.NO_OFFSET, np.uint64)
    for c in range(p):
        for i in range(ep):
            m = (c - i) % p
            diff = np.flatnonzero(parity[m, i] != img[m, d + i, :chunk])
            if diff.size:
                mism[c, i], first[c, i] = diff.size, diff[0]
    crcs = np.array([[zlib.crc32(img[r, c, :chunk].tobytes()) for c in range(p)] for r in range(p)], np.uint32)
    got_m, got_f = plan.report()
    print("rows that differ [stripe, row, bytes, first]:", [(c, i, int(got_m[c, i]), int(got_f[c, i]))
                                                          for c, i in np.argwhere(got_m != 0).tolist()])
    assert np.array_equal(got_m, mism) and np.array_equal(got_f, first), (mism.tolist(), first.tolist())
    assert plan.clean == (not mism.any())
    rep = plan.crcs()
    assert rep.shape == (p, p) and rep.dtype == np.uint32
    assert np.array_equal(rep, crcs), f"wrong CRCs at [member, cell] {np.argwhere(rep != crcs).tolist()}"
    got = lay.storage.cpu().numpy().reshape(img.shape)
    assert np.array_equal(got, img), f"the plan wrote to the set: {np.argwhere(got != img)[:4].tolist()}"
    return mism


@pytest.mark.parametrize("p,e,chunk", CLEAN, ids=[f"p{p}e{e}-c{ch}" for p, e, ch in CLEAN])
def test_clean_set(rd, p, e, chunk):
    lay, plan, img, parity = layout(rd, p, e, chunk)
    assert (plan.info.kind, plan.info.jobs) == (15 if e else 16, p)
    assert (plan.bytes_read, plan.bytes_written) == (p * p * chunk, 0)
    plan.execute()
    assert not check(rd, lay, plan, img, p, e, chunk, parity).any()


@pytest.mark.parametrize("p,e,chunk", DAMAGED, ids=[f"p{p}e{e}-c{ch}" for p, e, ch in DAMAGED])
def test_damaged_set(rd, p, e, chunk):
    lay, plan, img, _ = layout(rd, p, e, chunk)
    bad, located = damage(img, p, e, chunk)
    lay.storage.copy_(torch.from_numpy(bad.reshape(-1)))
    plan.execute()
    mism = check(rd, lay, plan, bad, p, e, chunk)
    assert mism[0].all() and mism[2].all() and np.count_nonzero(mism[1]) == 1 and not mism[3:].any()
    for c, (m, off) in located.items():
        assert plan.locate(c) == ((m, off) if e >= 2 else (-1, off))
    assert plan.locate(3) == (-1, None)


def test_graph_replays_follow_the_data(rd):
    p, e, chunk = 4, 2, BIG
    lay, plan, img, parity = layout(rd, p, e, chunk)
    bad, _ = damage(img, p, e, chunk)
    s = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):  # a linear chain: report reset, verify + tiles, finish
            plan.execute(s)
    for host in (img, bad, img):
        lay.storage.copy_(torch.from_numpy(host.reshape(-1).copy()))
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        check(rd, lay, plan, host, p, e, chunk, parity if host is img else None)


@pytest.mark.parametrize("p,e,shift", [(22, 4, 0), (12, 5, 0), (18, 0, 0), (4, 2, 1)])
def test_refused_at_plan_time(rd, p, e, shift):
    ep = e or 1
    lay = rd.SetLayout.allocate(p, p - ep, ep, 1024)
    lofi = [x + shift for x in lay.lofi_ptrs()]
    with pytest.raises(rd.RedsetHipError):
        if e:
            rd.RSCodec(p, e).plan_verify_crc32(lofi, lay.parity_ptrs(), 1024, lay.cell_stride)
        else:
            rd.xor_plan_verify_crc32(p, lofi, lay.parity_ptrs(), 1024, lay.cell_stride)
