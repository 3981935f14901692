"""GPU tests of setfiles.rebuild_set(check_survivors=True) (FileIO): sets on
disk written by apply_set, members removed, a surviving data file silently
damaged. Expected bytes are the saved copies of the files; the miscorrected
double error comes from the brute-force reference
(tests/rebuild_checked_ref.py). Every case first shows the plain rebuild_set
giving a wrong file from the same inputs: that is the point of the feature."""
import os

import numpy as np
import pytest

import rebuild_checked_ref as ref

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

SLICE = 1024  # smaller than every chunk below, and no divisor of them
# several files per member, sizes that are no multiple of the chunk (d = 2 data cells per member)
SIZES6 = [[3000, 2001], [5001], [1000, 3990, 7], [4990], [5000], [2500, 2480]]   # chunk 2501
SIZES5 = [[4000, 2101], [6100], [90, 6000], [6099], [3000, 3000]]                # chunk 3051
CASES = [(SIZES6, 4, [2]), (SIZES6, 4, [0, 3]), (SIZES5, 3, [4])]


@pytest.fixture(scope="module")
def sf():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import redset_amd
    from redset_amd import setfiles

    redset_amd.load()
    return setfiles


def make_set(sf, tmp, sizes, k, scheme="RS", checksums=False):
    rng = np.random.default_rng(23)
    members = []
    for r, fs in enumerate(sizes):
        fl = []
        for i, size in enumerate(fs):
            path = os.path.join(tmp, "data", f"rank{r}_file{i}.dat")
            os.makedirs(os.path.dirname(path), exist_ok=True)
            rng.integers(0, 256, size, dtype=np.uint8).tofile(path)
            fl.append(path)
        members.append(fl)
    res = sf.apply_set(scheme, members, os.path.join(tmp, "ckpt."), encoding=k, slice_bytes=SLICE,
                       checksums=checksums)
    return members, res


def read(path):
    with open(path, "rb") as fh:
        return fh.read()


def write(path, data):
    with open(path, "wb") as fh:
        fh.write(data)


def xor_logical(files, pos, values):
    """XOR `values` into a member's logical file at `pos` (inside one data file)."""
    for path in files:
        size = os.path.getsize(path)
        if pos < size:
            assert pos + len(values) <= size
            with open(path, "r+b") as fh:
                fh.seek(pos)
                old = fh.read(len(values))
                fh.seek(pos)
                fh.write(bytes(a ^ b for a, b in zip(old, values)))
            return path
        pos -= size
    raise AssertionError("the position lies in the member's zero padding")


def stat3(path):
    s = os.stat(path)
    return s.st_size, s.st_mtime_ns, s.st_ino


def data_cell_stripe(codec, member, index):
    p = codec.ranks
    for c in range(p):
        if codec.encoding_id(member, c) < p and codec.data_id(member, c) == index:
            return c
    raise AssertionError


class Case:
    """A set on disk that can be put back to 'members lost, one survivor damaged'."""

    def __init__(self, sf, tmp, sizes, k, lost, checksums=False):
        self.members, self.res = make_set(sf, tmp, sizes, k, checksums=checksums)
        self.reds, self.chunk = self.res["redundancy"], self.res["chunk"]
        self.lost = lost
        self.everything = [f for fl in self.members for f in fl] + self.reds
        self.sidecars = [r + ".crc" for r in self.reds] if checksums else []
        self.saved = {f: read(f) for f in self.everything + self.sidecars}
        self.lost_files = [f for r in lost for f in self.members[r]] + [self.reds[r] for r in lost]

    def reset(self, damage):
        """damage: (member, logical position, values) list."""
        gone = self.lost_files + [self.reds[r] + ".crc" for r in self.lost if self.sidecars]
        for f, data in self.saved.items():
            if f not in gone and read(f) != data:
                write(f, data)
        touched = [xor_logical(self.members[m], pos, values) for m, pos, values in damage]
        for f in gone:
            if os.path.exists(f):
                os.remove(f)
        return touched

    def rebuilt_equal(self):
        return [f for f in self.lost_files if read(f) != self.saved[f]]


@pytest.mark.parametrize("sizes,k,lost", CASES, ids=["rs6e4k1", "rs6e4k2", "rs5e3k1"])
def test_checked_rebuild_gets_right_what_the_plain_rebuild_gets_wrong(sf, tmp_path, sizes, k, lost):
    import redset_amd

    p = len(sizes)
    case = Case(sf, str(tmp_path), sizes, k, lost)
    chunk = case.chunk
    codec = redset_amd.RSCodec(p, k)
    # a survivor's data cell 1, 40 bytes from cell offset 1010: across the first slice boundary
    s = next(r for r in range(p) if r not in lost)
    pos = chunk + 1010
    damage = [(s, pos, [0x5A] * 40)]
    stripe = data_cell_stripe(codec, s, 1)
    # the plain rebuild: a wrong file, and nothing says so
    (touched,) = case.reset(damage)
    out = sf.rebuild_set(case.reds, slice_bytes=SLICE)
    assert out["ok"] and out["missing"] == lost
    assert case.rebuilt_equal() != []
    # the checked rebuild: byte-identical files, the survivor named, its file untouched
    case.reset(damage)
    before = {f: stat3(f) for f in case.everything if f not in case.lost_files}
    damaged_bytes = read(touched)
    out = sf.rebuild_set(case.reds, slice_bytes=SLICE, check_survivors=True)
    assert out["ok"] and out["trusted"] and out["unlocated_columns"] == 0 and out["unlocated_stripes"] == []
    assert out["survivor_corrections"] == [{"member": s, "stripe": stripe, "bytes": 40, "first_offset": 1010}]
    assert case.rebuilt_equal() == []
    assert read(touched) == damaged_bytes
    assert {f: stat3(f) for f in before} == before  # no survivor file was opened for writing
    # fix_survivors: the survivor's file is restored too, and the set verifies clean
    case.reset(damage)
    out = sf.rebuild_set(case.reds, slice_bytes=SLICE, check_survivors=True, fix_survivors=True)
    assert out["ok"] and out["trusted"]
    assert out["survivor_corrections"] == [{"member": s, "stripe": stripe, "bytes": 40, "first_offset": 1010}]
    for f in case.everything:
        assert read(f) == case.saved[f], f
    for f in before:  # only the damaged survivor's data files were opened for writing
        if f not in case.members[s] and f not in case.reds:
            assert stat3(f) == before[f], f
    v = sf.verify_set(case.reds, slice_bytes=SLICE)
    assert v["clean"] and v["damaged"] == []


def test_checksums_arbitrate_a_miscorrection(sf, oracle, tmp_path):
    """e - k = 2: two wrong survivors in one column, with values the reference
    says look like a third survivor's single error. The checked rebuild
    'corrects' it, no column is unlocated, and the recorded CRCs of the
    rebuilt files say the result is wrong."""
    import redset_amd

    p, k, lost = 6, 4, [0, 3]
    case = Case(sf, str(tmp_path), SIZES6, k, lost, checksums=True)
    chunk = case.chunk
    codec = redset_amd.RSCodec(p, k)
    # a clean checked rebuild with checksums is ok
    case.reset([])
    out = sf.rebuild_set(case.reds, slice_bytes=SLICE, checksums=True, check_survivors=True)
    assert out["ok"] and out["trusted"] and out["checksum_damaged"] == [] and out["survivor_corrections"] == []
    assert case.rebuilt_equal() == []
    c = next(c for c in range(p) if sum(codec.encoding_id(m, c) < p for m in range(p) if m not in lost) >= 2)
    st = ref.Stripe(oracle, codec, c, lost)
    a, b = [m for m in st.surv if st.row[m] < 0][:2]
    found = None
    for x1 in range(1, 256):
        by = np.zeros((p, 255), np.uint8)
        by[a] = x1
        by[b] = np.arange(1, 256)
        _, member, xs, _ = st.explain(by)
        hit = np.nonzero(member >= 0)[0]
        if hit.size:
            found = (x1, int(hit[0]) + 1, int(member[hit[0]]))
            break
    assert found is not None
    x1, x2, t = found
    assert t not in (a, b) and t in st.surv
    col = 77
    case.reset([(a, st.index[a] * chunk + col, [x1]), (b, st.index[b] * chunk + col, [x2])])
    out = sf.rebuild_set(case.reds, slice_bytes=SLICE, checksums=True, check_survivors=True)
    assert out["trusted"] and out["unlocated_columns"] == 0
    assert out["survivor_corrections"] == [{"member": t, "stripe": c, "bytes": 1, "first_offset": col}]
    assert out["ok"] is False and out["checksum_damaged"] != []
    assert {d["member"] for d in out["checksum_damaged"]} <= set(lost)
    assert case.rebuilt_equal() != []


def test_defaults_change_nothing(sf, tmp_path):
    p, k, lost = 6, 4, [1]
    case = Case(sf, str(tmp_path), SIZES6, k, lost)
    outs, files = [], []
    for kw in ({}, {"check_survivors": False, "fix_survivors": False}):
        case.reset([])
        outs.append(sf.rebuild_set(case.reds, slice_bytes=SLICE, **kw))
        files.append({f: read(f) for f in case.everything})
        assert case.rebuilt_equal() == []
    a, b = outs
    assert list(a) == list(b) == ["scheme", "ranks", "encoding", "chunk", "missing", "redundancy", "errors", "stats", "ok"]
    assert {x: a[x] for x in a if x != "stats"} == {x: b[x] for x in b if x != "stats"}
    assert list(a["stats"]) == list(b["stats"])
    for key in ("bytes_read", "bytes_written", "units"):
        assert a["stats"][key] == b["stats"][key]
    assert files[0] == files[1]


def test_refusals(sf, tmp_path):
    # as many lost members as parity rows: nothing left to check
    members, res = make_set(sf, str(tmp_path / "rs"), [[5000], [6000], [7000], [4000]], 2)
    for r in (1, 2):
        os.remove(members[r][0])
    with pytest.raises(ValueError, match="nothing is left to check"):
        sf.rebuild_set(res["redundancy"], check_survivors=True)
    assert not os.path.exists(members[1][0])  # refused before anything was written
    members, res = make_set(sf, str(tmp_path / "xor"), [[5000], [6000], [7000]], 1, scheme="XOR")
    os.remove(members[0][0])
    with pytest.raises(ValueError, match="XOR"):
        sf.rebuild_set(res["redundancy"], check_survivors=True)
    members, res = make_set(sf, str(tmp_path / "rs5"), [[500], [600], [700], [400], [300], [200], [100]], 5)
    os.remove(members[0][0])
    with pytest.raises(ValueError, match="2..4"):
        sf.rebuild_set(res["redundancy"], check_survivors=True)
    with pytest.raises(ValueError, match="needs check_survivors"):
        sf.rebuild_set(res["redundancy"], fix_survivors=True)
