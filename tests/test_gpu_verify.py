"""GPU tests of set verification (include/redset_hip.h, "set verification"):
the check kernels' report against the CPU oracle -- the oracle's parity of
the cells as uploaded, XORed with the stored parity, gives the expected count
of differing bytes and the first differing offset per (stripe, parity row),
and both must match exactly -- for clean and damaged sets, device plans,
the streaming pipeline and sets on disk; then locate and repair end to end.

Oracle encodes are the slow part, so a clean encoded set is made once per
(scheme, shape, chunk) and shared; tests damage copies of single cells."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

NO = (1 << 64) - 1
CHUNKS = [16, 1008, 1040, 4096 + 7, 65536, (1 << 20) + 48]
RS_SHAPES = [(4, 2), (11, 3), (20, 4), (12, 6), (40, 3)]
XOR_RANKS = [4, 8, 20]
SELF = "tests/test_gpu_verify.py"


@pytest.fixture(scope="module")
def rd():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import redset_amd

    redset_amd.load()
    return redset_amd


_sets = {}


def clean_set(oracle, scheme, p, e, chunk):
    """(lofi, parity) host arrays of an encoded set; shared, never modified."""
    key = (scheme, p, e, chunk)
    if key not in _sets:
        lofi, parity = oracle.random_set(p, p - e, e, chunk, seed=1000 * p + 10 * e + chunk % 997)
        encode(oracle, scheme, p, e, chunk, lofi, parity)
        for a in lofi + parity:
            a.setflags(write=False)
        _sets[key] = (lofi, parity)
    return _sets[key]


def encode(oracle, scheme, p, e, chunk, lofi, parity):
    if scheme == "RS":
        oracle.OracleRS(p, e).encode_set(lofi, parity, chunk)
    else:
        oracle.xor_encode_set(p, lofi, parity, chunk)


def expected(oracle, scheme, p, e, chunk, lofi, parity):
    """mismatch[p, e], first[p, e] from the oracle's parity of the stored
    data XOR the stored parity. Stripe c's parity row i is member
    (c - i) mod p's slot i (RS); member c's only slot (XOR)."""
    want = [np.zeros(e * chunk, np.uint8) for _ in range(p)]
    encode(oracle, scheme, p, e, chunk, [np.ascontiguousarray(x) for x in lofi], want)
    mism = np.zeros((p, e), np.uint64)
    first = np.full((p, e), NO, np.uint64)
    for c in range(p):
        for i in range(e):
            r = (c - i) % p
            seg = want[r][i * chunk:(i + 1) * chunk] ^ parity[r][i * chunk:(i + 1) * chunk]
            n = int(np.count_nonzero(seg))
            if n:
                mism[c, i] = n
                first[c, i] = int(np.argmax(seg != 0))
    return mism, first


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

    def lofi_ptrs(self):
        return [self.storage.data_ptr() + r * self.member for r in range(self.p)]

    def parity_ptrs(self):
        return [self.storage.data_ptr() + r * self.member + self.d * self.stride for r in range(self.p)]


def make_plan(rd, scheme, p, e, lay):
    if scheme == "RS":
        return rd.RSCodec(p, e).plan_verify(lay.lofi_ptrs(), lay.parity_ptrs(), lay.chunk, lay.stride)
    return rd.xor_plan_verify(p, lay.lofi_ptrs(), lay.parity_ptrs(), lay.chunk, lay.stride)


def run(plan):
    plan.execute()
    torch.cuda.synchronize()
    return plan.report()


def check_info(plan, scheme, p, e, chunk):
    d = p - e
    fused = d <= 16 and e <= 4 if scheme == "RS" else p <= 16
    if fused:
        assert plan.bytes_written == 0
        assert plan.bytes_read == (p * (d + e) * chunk if scheme == "RS" else p * p * chunk)
    else:
        assert plan.bytes_written > 0 and plan.bytes_read > p * p * chunk


CLEAN_CASES = ([("RS", p, e, False) for p, e in RS_SHAPES] + [("XOR", p, 1, False) for p in XOR_RANKS] +
               [("RS", 11, 3, True), ("XOR", 4, 1, True)])


@pytest.mark.parametrize("chunk", CHUNKS)
@pytest.mark.parametrize("scheme,p,e,packed", CLEAN_CASES)
def test_clean_set(rd, oracle, scheme, p, e, packed, chunk):
    lofi, parity = clean_set(oracle, scheme, p, e, chunk)
    lay = Layout(p, p - e, e, chunk, packed).upload(lofi, parity)
    before = lay.storage.clone()
    plan = make_plan(rd, scheme, p, e, lay)
    mism, first = run(plan)
    print(f"{scheme}({p},{e}) chunk {chunk}: mismatch {int(mism.sum())}, launches {plan.launches}")
    assert mism.shape == (p, e) and not mism.any() and (first == NO).all()
    assert plan.clean
    check_info(plan, scheme, p, e, chunk)
    assert torch.equal(lay.storage, before), "verify modified a cell"


def places(chunk):
    """(offset, length) of the damage: offset 0, the last byte, the last byte
    of the last whole 16-B vector, the first tail byte, 1023, 1024, a 4 KiB run."""
    whole = chunk // 16 * 16
    return [(0, 1), (chunk - 1, 1), (whole - 1, 1), (whole if whole < chunk else chunk - 1, 1), (1023, 1), (1024, 1),
            (chunk // 2 - 100, min(4096, chunk - (chunk // 2 - 100)))]


def damage(cell, off, n, rng):
    """XOR nonzero bytes into n bytes of a host cell."""
    cell[off:off + n] ^= rng.integers(1, 256, n, dtype=np.uint8)


DAMAGE_CASES = [("RS", 11, 3), ("RS", 20, 4), ("RS", 40, 3), ("XOR", 8, 1)]


@pytest.mark.parametrize("chunk", [4096 + 7, (1 << 20) + 48])
@pytest.mark.parametrize("scheme,p,e", DAMAGE_CASES)
def test_damage(rd, oracle, scheme, p, e, chunk):
    """Damage at every place, each place in a stripe of its own (stripe k:
    place k), first in one data cell per stripe, then, separately, in one
    parity cell per stripe; stripe 7 of the data run has two members damaged.
    Then the report's lifetime: a second execute, repair, graph replays."""
    d = p - e
    lofi0, parity0 = clean_set(oracle, scheme, p, e, chunk)
    rng = np.random.default_rng(chunk + p)
    pl = places(chunk)
    assert len(pl) < 8 <= p
    lay = Layout(p, d, e, chunk, False).upload(lofi0, parity0)
    plan = make_plan(rd, scheme, p, e, lay)

    def data_cell_of(c, skip=0):
        """(member, segment) of a data cell of stripe c"""
        import np_ref

        ms = [m for m in range(p) if (np_ref.encoding_id(p, e, m, c) < p if scheme == "RS" else m != c)]
        m = ms[(c + skip) % len(ms)]
        seg = np_ref.data_id(p, e, m, c) if scheme == "RS" else (c if c < m else c - 1)
        return m, seg

    # data cells
    lofi = [x.copy() for x in lofi0]
    touched = []
    for k, (off, n) in enumerate(pl):
        m, seg = data_cell_of(k)
        damage(lofi[m][seg * chunk:(seg + 1) * chunk], off, n, rng)
        touched.append((m, seg))
    for skip, off in ((0, 5), (1, 4090)):  # two members of stripe 7, different offsets
        m, seg = data_cell_of(7, skip)
        damage(lofi[m][seg * chunk:(seg + 1) * chunk], off, 3, rng)
        touched.append((m, seg))
    for m, seg in touched:
        lay.data_cell(m, seg).copy_(torch.from_numpy(lofi[m][seg * chunk:(seg + 1) * chunk]))
    want_m, want_f = expected(oracle, scheme, p, e, chunk, lofi, parity0)
    assert want_m[:8].all() and not want_m[8:].any()
    mism, first = run(plan)
    print(f"data damage {scheme}({p},{e}) chunk {chunk}: mismatch rows {mism[:8].tolist()}")
    assert np.array_equal(mism, want_m) and np.array_equal(first, want_f)
    assert not plan.clean
    # execute twice: the same report, not an accumulated one
    mism2, first2 = run(plan)
    assert np.array_equal(mism2, want_m) and np.array_equal(first2, want_f)
    # damaged replay under a captured graph (one stream, no parallel branches)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        plan.execute(s)
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        plan.execute(torch.cuda.current_stream())
    g.replay()
    torch.cuda.synchronize()
    mism3, first3 = plan.report()
    assert np.array_equal(mism3, want_m) and np.array_equal(first3, want_f)
    # repair the bytes: clean again, by execute and by replaying the same graph
    for m, seg in touched:
        lay.data_cell(m, seg).copy_(torch.from_numpy(lofi0[m][seg * chunk:(seg + 1) * chunk].copy()))
    g.replay()
    torch.cuda.synchronize()
    mism4, first4 = plan.report()
    assert not mism4.any() and (first4 == NO).all()
    mism5, _ = run(plan)
    assert not mism5.any() and plan.clean

    # parity cells, separately: stripe k's parity row k % e, place k
    parity = [x.copy() for x in parity0]
    for k, (off, n) in enumerate(pl):
        i = k % e
        r = (k - i) % p
        damage(parity[r][i * chunk:(i + 1) * chunk], off, n, rng)
        lay.parity_cell(r, i).copy_(torch.from_numpy(parity[r][i * chunk:(i + 1) * chunk]))
    want_m, want_f = expected(oracle, scheme, p, e, chunk, lofi0, parity)
    for k, (off, n) in enumerate(pl):
        # a parity cell's damage shows in its own row only
        assert want_m[k, k % e] == n and want_f[k, k % e] == off and np.count_nonzero(want_m[k]) == 1
    mism, first = run(plan)
    assert np.array_equal(mism, want_m) and np.array_equal(first, want_f)


@pytest.mark.parametrize("p,e", [(6, 3), (11, 3)])
def test_scrub_end_to_end(rd, oracle, p, e):
    """Damage several cells of one member: locate names it in every damaged
    stripe, a rebuild of that member verifies clean and restores the bytes."""
    import np_ref

    d, chunk = p - e, 4096 + 7
    lofi0, parity0 = clean_set(oracle, "RS", p, e, chunk)
    lay = Layout(p, d, e, chunk, False).upload(lofi0, parity0)
    codec = rd.RSCodec(p, e)
    plan = codec.plan_verify(lay.lofi_ptrs(), lay.parity_ptrs(), chunk, lay.stride)
    rng = np.random.default_rng(p)
    bad = 2
    hit = {}
    lofi = [x.copy() for x in lofi0]
    parity = [x.copy() for x in parity0]
    for c, off in ((0, 17), (1, 4100), (3, 2048), (p - 1, 0)):
        enc = np_ref.encoding_id(p, e, bad, c)
        if enc < p:
            seg = np_ref.data_id(p, e, bad, c)
            damage(lofi[bad][seg * chunk:(seg + 1) * chunk], off, 2, rng)
            lay.data_cell(bad, seg).copy_(torch.from_numpy(lofi[bad][seg * chunk:(seg + 1) * chunk]))
        else:
            i = enc - p
            damage(parity[bad][i * chunk:(i + 1) * chunk], off, 2, rng)
            lay.parity_cell(bad, i).copy_(torch.from_numpy(parity[bad][i * chunk:(i + 1) * chunk]))
        hit[c] = off
    mism, first = run(plan)
    want_m, want_f = expected(oracle, "RS", p, e, chunk, lofi, parity)
    assert np.array_equal(mism, want_m) and np.array_equal(first, want_f)
    for c in range(p):
        member, off = plan.locate(c)
        assert (member, off) == ((bad, hit[c]) if c in hit else (-1, None)), c
    reb = codec.plan_rebuild([bad], lay.lofi_ptrs(), lay.parity_ptrs(), chunk, lay.stride)
    reb.execute()
    mism, _ = run(plan)
    assert not mism.any() and plan.clean
    for s in range(d):
        assert np.array_equal(lay.data_cell(bad, s).cpu().numpy(), lofi0[bad][s * chunk:(s + 1) * chunk])
    for i in range(e):
        assert np.array_equal(lay.parity_cell(bad, i).cpu().numpy(), parity0[bad][i * chunk:(i + 1) * chunk])

    # two members damaged in one stripe at different offsets: the first
    # differing column holds one wrong byte, the second another; at one shared
    # offset the answer is whatever the CPU rule says of that column
    M = np_ref.encoding_matrix(p, e)
    c = 4
    ms = [m for m in range(p) if np_ref.encoding_id(p, e, m, c) < p][:2]
    segs = [np_ref.data_id(p, e, m, c) for m in ms]
    for (m, seg), off in zip(zip(ms, segs), (100, 3000)):
        cell = lofi0[m][seg * chunk:(seg + 1) * chunk].copy()
        damage(cell, off, 1, rng)
        lay.data_cell(m, seg).copy_(torch.from_numpy(cell))
    run(plan)
    assert plan.locate(c) == (ms[0], 100)
    eps = {}
    for m, seg in zip(ms, segs):  # both at offset 100
        cell = lofi0[m][seg * chunk:(seg + 1) * chunk].copy()
        damage(cell, 100, 1, rng)
        lay.data_cell(m, seg).copy_(torch.from_numpy(cell))
        eps[m] = int(cell[100] ^ lofi0[m][seg * chunk + 100])
    run(plan)
    syn = np_ref.MUL[M[p:, ms[0]], eps[ms[0]]] ^ np_ref.MUL[M[p:, ms[1]], eps[ms[1]]]
    want = [m for m in range(p) if np_ref.encoding_id(p, e, m, c) < p and
            any(np.array_equal(np_ref.MUL[M[p:, m], x], syn) for x in range(1, 256))]
    want = want[0] if len(want) == 1 and np.count_nonzero(syn) > 1 else -1
    assert np.count_nonzero(syn) != 1  # two data errors never look like one parity row (e >= 3)
    assert plan.locate(c) == (want, 100)


def test_xor_locates_nothing(rd, oracle):
    p, chunk = 8, 4096 + 7
    lofi0, xorc0 = clean_set(oracle, "XOR", p, 1, chunk)
    lay = Layout(p, p - 1, 1, chunk, False).upload(lofi0, xorc0)
    lay.data_cell(3, 0)[77] ^= 1
    plan = rd.xor_plan_verify(p, lay.lofi_ptrs(), lay.parity_ptrs(), chunk, lay.stride)
    mism, first = run(plan)
    assert int(mism[0, 0]) == 1 and int(first[0, 0]) == 77 and int(mism.sum()) == 1
    assert plan.locate(0) == (-1, 77) and plan.locate(1) == (-1, None)


# ---- streaming ---------------------------------------------------------------

def _host_ptrs(lofi, parity):
    return [a.ctypes.data for a in lofi], [a.ctypes.data for a in parity]


@pytest.mark.parametrize("pinned", [False, True])
@pytest.mark.parametrize("scheme,p,e", [("RS", 11, 3), ("RS", 40, 3), ("XOR", 8, 1)])
def test_verify_stream_host_memory(rd, oracle, scheme, p, e, pinned):
    """Host memory, pinned (checked in place) and not (staged in slices
    smaller than the chunk): clean, then damage in a later slice, reported
    at its cell offset."""
    from redset_amd import stream

    d, chunk, sl = p - e, 65536, 16384
    lofi0, parity0 = clean_set(oracle, scheme, p, e, chunk)
    if pinned:
        hl = torch.empty(p * d * chunk, dtype=torch.uint8).pin_memory()
        hp = torch.empty(p * e * chunk, dtype=torch.uint8).pin_memory()
        lofi = [hl[r * d * chunk:(r + 1) * d * chunk].numpy() for r in range(p)]
        parity = [hp[r * e * chunk:(r + 1) * e * chunk].numpy() for r in range(p)]
        for r in range(p):
            lofi[r][:] = lofi0[r]
            parity[r][:] = parity0[r]
    else:
        lofi = [x.copy() for x in lofi0]
        parity = [x.copy() for x in parity0]
    io = stream.HostIO(p, *_host_ptrs(lofi, parity), chunk, keepalive=(lofi, parity), pinned=pinned)
    codec = rd.RSCodec(p, e) if scheme == "RS" else None

    def verify():
        if scheme == "RS":
            return stream.rs_verify_stream(codec, chunk, io, slice_bytes=sl, io_threads=4)
        return stream.xor_verify_stream(p, chunk, io, slice_bytes=sl, io_threads=4)

    res = verify()
    assert res["clean"] and not res["mismatch"].any() and (res["first"] == NO).all()
    assert res["stats"]["bytes_written"] == 0 and res["stats"]["write_seconds"] == 0
    assert res["stats"]["bytes_read"] == (p * p * chunk)
    rng = np.random.default_rng(3)
    damage(lofi[1][0:chunk], 3 * sl + 11, 5, rng)          # member 1's first data cell, fourth slice
    damage(parity[2][0:chunk], 2 * sl - 1, 2, rng)         # member 2's parity slot 0, across two slices
    snap_l, snap_p = [x.copy() for x in lofi], [x.copy() for x in parity]
    res = verify()
    want_m, want_f = expected(oracle, scheme, p, e, chunk, lofi, parity)
    assert want_m.any()
    assert np.array_equal(res["mismatch"], want_m) and np.array_equal(res["first"], want_f)
    assert not res["clean"]
    assert all(np.array_equal(a, b) for a, b in zip(lofi + parity, snap_l + snap_p)), "verify wrote to the set"


def _write_files(tmp, p, sizes, seed):
    rng = np.random.default_rng(seed)
    out = []
    for r in range(p):
        fl = []
        for k, size in enumerate(sizes[r]):
            path = os.path.join(tmp, f"rank{r}_file{k}.dat")
            rng.integers(0, 256, size, dtype=np.uint8).tofile(path)
            fl.append(path)
        out.append(fl)
    return out


@pytest.mark.parametrize("scheme,p,k", [("RS", 6, 2), ("XOR", 4, 1)])
def test_verify_set_files(rd, oracle, tmp_path, scheme, p, k):
    """verify_set on apply_set's output is clean (members of different sizes:
    reads past a short last file are zeros, as apply_set treats them); one
    flipped byte of a data file is reported with its member, stripe and
    offset; nothing is written; rebuild_set restores the member."""
    from redset_amd import setfiles

    tmp = str(tmp_path)
    sizes = [[150_000, 33], [1], [120_000], [0, 99_999], [149_000, 5], [4096]][:p]
    members = _write_files(tmp, p, sizes, seed=p + k)
    res = setfiles.apply_set(scheme, members, os.path.join(tmp, "ckpt."), encoding=k, slice_bytes=1 << 15)
    reds, chunk = res["redundancy"], res["chunk"]
    allpaths = [f for fl in members for f in fl] + reds
    stamp = {f: (os.stat(f).st_mtime_ns, os.stat(f).st_size) for f in allpaths}
    rep = rd.verify_set(reds, slice_bytes=1 << 14)
    assert rep["scheme"] == scheme and rep["clean"] and rep["mismatch_bytes"] == 0 and rep["damaged"] == []
    assert rep["stats"]["bytes_written"] == 0
    # flip one byte of member 2's data file: logical offset 70_000
    bad, pos = 2, 70_000
    orig = np.fromfile(members[bad][0], dtype=np.uint8)
    flipped = orig.copy()
    flipped[pos] ^= 0x5A
    flipped.tofile(members[bad][0])
    stamp[members[bad][0]] = (os.stat(members[bad][0]).st_mtime_ns, orig.size)
    rep = rd.verify_set(reds, slice_bytes=1 << 14)
    seg, off = divmod(pos, chunk)
    if scheme == "RS":
        import np_ref

        stripe = [c for c in range(p) if np_ref.encoding_id(p, k, bad, c) < p and np_ref.data_id(p, k, bad, c) == seg][0]
        want = {"stripe": stripe, "offset": off, "member": bad, "kind": "data"}
    else:
        stripe = seg if seg < bad else seg + 1
        want = {"stripe": stripe, "offset": off, "member": None, "kind": None}
    assert not rep["clean"] and rep["mismatch_bytes"] == k and rep["damaged"] == [want]
    assert {f: (os.stat(f).st_mtime_ns, os.stat(f).st_size) for f in allpaths} == stamp, "verify_set wrote a file"
    # repair: remove the member's files, rebuild, verify
    for f in members[bad] + [reds[bad]]:
        os.remove(f)
    out = setfiles.rebuild_set([r for i, r in enumerate(reds) if i != bad], slice_bytes=1 << 15)
    assert out["missing"] == [bad] and out["ok"]
    assert np.array_equal(np.fromfile(members[bad][0], dtype=np.uint8), orig)
    assert rd.verify_set(reds)["clean"]


def test_verify_stream_never_writes(rd, oracle):
    """io->write is never reached: a verify over an I/O whose write pointer
    is NULL runs, where an encode refuses it."""
    import ctypes

    from redset_amd import _lib, stream

    p, e, chunk = 11, 3, 65536
    lofi0, parity0 = clean_set(oracle, "RS", p, e, chunk)
    lofi, parity = [x.copy() for x in lofi0], [x.copy() for x in parity0]
    io = stream.HostIO(p, *_host_ptrs(lofi, parity), chunk, keepalive=(lofi, parity))
    io.io.write = None
    codec = rd.RSCodec(p, e)
    assert stream.rs_verify_stream(codec, chunk, io, slice_bytes=8192)["clean"]
    st = _lib.StreamStats()
    assert _lib.load().redset_hip_rs_encode_stream(codec._h, chunk, 0, 0, 8192, 0, ctypes.byref(io.io),
                                                   ctypes.byref(st)) == _lib.REDSET_FAILURE


# ---- the test twin -----------------------------------------------------------

@pytest.mark.timeout(600)
def test_verify_bit_exact_with_ring_fallbacks(tmp_path):
    """This file once more in a child process against the test twin library
    with a 4-poll ring cap: every check kernel then takes the direct-load
    fallbacks, which must check the same bytes -- the child is green -- and
    the capped spins are counted."""
    from conftest import gpu_available
    from test_gpu_test_build import TWIN, _child

    if not gpu_available():
        pytest.skip("needs an MI355X")
    assert os.path.exists(TWIN), f"{TWIN} missing: build with `make -C redset_amd/csrc`"
    log = tmp_path / "faults.txt"
    res, text = _child(tmp_path, "test_twin_verify.log", {
        "REDSET_HIP_TEST_SPIN_CAP": "4",
        "REDSET_RING_FALLBACK_RUN": "1",
        "REDSET_RING_FAULT_LOG": str(log),
    }, ["-m", "gpu", "--deselect", f"{SELF}::test_verify_bit_exact_with_ring_fallbacks"], 550,
        files=("test_gpu_verify.py",))
    assert res.returncode == 0, text[-6000:]
    lines = log.read_text().split()
    faults, libs = int(lines[0]), lines[1:]
    print(f"verify on the test twin, 4-poll cap: {faults} capped spins; {text.strip().splitlines()[-1]}")
    assert libs == [TWIN], libs
    assert faults > 100, faults
    assert " passed" in text.strip().splitlines()[-1] and "skipped" not in text.strip().splitlines()[-1]
