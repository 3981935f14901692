"""GPU tests of the CRC-32 plans (include/redset_hip.h, "member checksums"):
every CRC the kernels give is compared with zlib.crc32 of the same bytes
taken from the host copy -- never with another run of the kernels.

The kernels cut a range into 512-B segments on its 16-B address grid, 256 to
a tile (128 KiB), and finish a range of more than 64 tiles with more than one
tile per lane: the lengths below surround 512 + 16 (the longest tail), one
tile and 64 tiles besides the powers of two."""
import zlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

SEG, TILE = 512, 512 * 256
LENGTHS = sorted(set(
    [0, 1, 3, 15, 16, 17, 255, 1008, 1040, 4096 + 7, (1 << 20) + 48] +
    [(1 << k) + d for k in range(4, 21) for d in (-1, 0, 1)] +
    [SEG + 14, SEG + 15, SEG + 16, SEG + 17, 2 * SEG + 15, TILE + 15, TILE + 16, TILE + SEG + 17, 2 * TILE - SEG - 3]))
MISALIGN = [0, 1, 3, 13]
BIG = [64 * TILE - 1, 64 * TILE + 16, 65 * TILE + 9, 130 * TILE + SEG + 5]  # the finishing wave's 1 -> 2 -> 3 tiles per lane


@pytest.fixture(scope="module")
def rd():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import redset_amd

    redset_amd.load()
    return redset_amd


def fill(kind, n, seed=0):
    if kind == "zero":
        return np.zeros(n, np.uint8)
    if kind == "ff":
        return np.full(n, 0xFF, np.uint8)
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8)


def placed(lengths, misaligns):
    """(offset, length) of every (length, misalignment) in one buffer, each
    at its misalignment from a 256-B aligned base; and the buffer's size."""
    out, pos = [], 0
    for n in lengths:
        for m in misaligns:
            out.append((pos + m, n))
            pos += -(-(m + n) // 256) * 256 + 256
    return out, pos


def device_buffer(host):
    """`host` on the device at a 256-B aligned address"""
    raw = torch.empty(host.size + 256, dtype=torch.uint8, device="cuda")
    shift = -raw.data_ptr() % 256
    buf = raw[shift:shift + host.size]
    buf.copy_(torch.from_numpy(host))
    assert buf.data_ptr() % 256 == 0
    return buf


def run(plan):
    plan.execute()
    torch.cuda.synchronize()
    return plan.report()


def want(host, ranges):
    return [zlib.crc32(host[o:o + n].tobytes()) for o, n in ranges]


def check(rd, host, ranges):
    buf = device_buffer(host)
    plan = rd.Crc32Plan([(buf.data_ptr() + o, n) for o, n in ranges], keepalive=buf)
    got, exp = run(plan), want(host, ranges)
    bad = [(ranges[i], hex(got[i]), hex(exp[i])) for i in range(len(ranges)) if got[i] != exp[i]]
    assert not bad, bad[:8]
    return plan, buf


@pytest.mark.parametrize("kind", ["random", "zero", "ff"])
def test_lengths_and_misalignments(rd, kind):
    ranges, size = placed(LENGTHS, MISALIGN)
    plan, _ = check(rd, fill(kind, size, seed=7), ranges)
    info = plan.info()
    assert info["kind"] == 7 and info["jobs"] == len(ranges) and info["bytes_written"] == 0
    assert info["bytes_read"] == sum(n for _, n in ranges) and info["launches"] == 2


@pytest.mark.parametrize("kind", ["random", "zero"])
def test_many_tiles(rd, kind):
    ranges, size = placed(BIG, [0, 13])
    check(rd, fill(kind, size, seed=8), ranges)


def test_known_vector_and_empty_plan_shapes(rd):
    host = np.frombuffer(b"123456789" + bytes(247), np.uint8).copy()
    plan, _ = check(rd, host, [(0, 9), (0, 0), (3, 0)])
    assert plan.report()[0] == 0xCBF43926
    assert plan.info()["launches"] == 1  # no range has a full segment: the finishing launch only
    # an empty range may have no address at all
    assert run(rd.Crc32Plan([(None, 0)])) == [0]


def test_three_hundred_mixed_ranges(rd):
    rng = np.random.default_rng(11)
    host = fill("random", 6 << 20, seed=12)
    ranges = []
    for i in range(300):
        n = 0 if i % 17 == 0 else int(rng.choice([rng.integers(1, 64), rng.integers(64, 5000), rng.integers(5000, 700000)]))
        ranges.append((int(rng.integers(0, host.size - n)), n))
    plan, _ = check(rd, host, ranges)  # they overlap freely
    assert plan.info()["jobs"] == 300


def test_overlapping_ranges(rd):
    host = fill("random", 3 * TILE, seed=13)
    check(rd, host, [(0, host.size), (5, host.size - 5), (5, 2 * TILE), (TILE - 7, TILE + 100), (TILE, 1), (0, host.size)])


def test_replay_after_a_byte_changes(rd):
    host = fill("random", 4 * TILE, seed=14)
    ranges = [(0, TILE + 100), (TILE + 100, TILE), (2 * TILE + 100, 1000), (3 * TILE, TILE)]
    plan, buf = check(rd, host, ranges)
    first = plan.report()
    for pos in (TILE + 100 + 70000, 2 * TILE + 100 + 999):  # inside a tile, then in a tail
        host[pos] ^= 0x40
        buf[pos] = int(host[pos])
        got, exp = run(plan), want(host, ranges)
        assert got == exp
        hit = [i for i, (o, n) in enumerate(ranges) if o <= pos < o + n]
        assert [i for i in range(len(ranges)) if got[i] != first[i]] == hit and len(hit) == 1
        first = got


def test_graph_capture_and_replay(rd):
    host = fill("random", 2 * TILE + 4096, seed=15)
    ranges = [(1, 2 * TILE + 77), (TILE, 0), (4096 + 3, 1040), (0, host.size)]
    buf = device_buffer(host)
    plan = rd.Crc32Plan([(buf.data_ptr() + o, n) for o, n in ranges], keepalive=buf)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        plan.execute()  # warm: modules loaded before the capture
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        plan.execute()
    for pos in (5, 2 * TILE + 50):
        host[pos] ^= 0xA5
        buf[pos] = int(host[pos])
        g.replay()
        torch.cuda.synchronize()
        assert plan.report() == want(host, ranges)


class Layout:
    """The set in one device tensor: member r's d data cells then its e
    parity cells, `stride` apart. packed: stride = chunk, so cells are
    unaligned whenever chunk % 16 != 0 (the kernels' byte path)."""

    def __init__(self, p, d, e, chunk, packed):
        self.p, self.d, self.e, self.chunk = p, d, e, chunk
        self.stride = chunk if packed else -(-chunk // 256) * 256
        self.member = (d + e) * self.stride
        self.storage = torch.zeros(p * self.member, dtype=torch.uint8, device="cuda")

    def upload(self, lofi, parity):
        host = np.zeros(self.p * self.member, np.uint8)
        v = host.reshape(self.p, self.d + self.e, self.stride)
        for r in range(self.p):
            v[r, :self.d, :self.chunk] = lofi[r].reshape(self.d, self.chunk)
            v[r, self.d:, :self.chunk] = parity[r].reshape(self.e, self.chunk)
        self.storage.copy_(torch.from_numpy(host))
        return self

    def data_cell(self, r, s):
        o = r * self.member + s * self.stride
        return self.storage[o:o + self.chunk]

    def parity_cell(self, r, i):
        o = r * self.member + (self.d + i) * self.stride
        return self.storage[o:o + self.chunk]


@pytest.mark.parametrize("packed", [True, False])
@pytest.mark.parametrize("chunk", [1040, 65536])
@pytest.mark.parametrize("p,e", [(4, 2), (11, 3)])
def test_one_range_per_cell_of_a_set(rd, oracle, p, e, chunk, packed):
    d = p - e
    lofi, parity = oracle.random_set(p, d, e, chunk, seed=100 * p + e + chunk % 91)
    for r in range(p):
        parity[r][:] = fill("random", e * chunk, seed=1000 + r)
    lay = Layout(p, d, e, chunk, packed).upload(lofi, parity)
    cells = [lay.data_cell(r, s) for r in range(p) for s in range(d)] + \
            [lay.parity_cell(r, i) for r in range(p) for i in range(e)]
    exp = [zlib.crc32(lofi[r][s * chunk:(s + 1) * chunk].tobytes()) for r in range(p) for s in range(d)] + \
          [zlib.crc32(parity[r][i * chunk:(i + 1) * chunk].tobytes()) for r in range(p) for i in range(e)]
    plan = rd.Crc32Plan([(c, chunk) for c in cells], keepalive=lay)
    assert run(plan) == exp
    # the oracle's own CRC agrees with zlib on the first cell
    if hasattr(oracle, "crc32"):
        assert oracle.crc32(lofi[0][:chunk]) == exp[0]
    info = plan.info()
    assert (info["kind"], info["jobs"], info["bytes_read"], info["bytes_written"]) == (7, p * p, p * p * chunk, 0)


def test_report_argument_checks(rd):
    from ctypes import c_uint

    from redset_amd import _lib

    buf = device_buffer(fill("random", 4096))
    plan = rd.Crc32Plan([(buf.data_ptr(), 100), (buf.data_ptr() + 100, 200)], keepalive=buf)
    out = (c_uint * 2)()
    L = _lib.load()
    assert L.redset_hip_plan_crc32_report(plan._h, None, out, 1) == _lib.REDSET_FAILURE
    assert b"room for 1 CRCs, the plan reports 2" in L.redset_hip_last_error()
