"""GPU tests of the checksum sidecars of sets on disk (redset_amd.setfiles,
checksums=True): apply_set records the CRC-32 of every member's data files
and redundancy payload, verify_set names what the parity cannot, rebuild_set
notices a rebuild made from a damaged survivor. Recorded CRCs are compared
with zlib.crc32 of the files' bytes."""
import json
import os
import zlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")


@pytest.fixture(scope="module")
def sf():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import redset_amd
    from redset_amd import setfiles

    redset_amd.load()
    return setfiles


def make_members(tmp, sizes, seed):
    rng = np.random.default_rng(seed)
    out = []
    for r, fs in enumerate(sizes):
        fl = []
        for k, size in enumerate(fs):
            path = os.path.join(tmp, "data", f"rank{r}_file{k}.dat")
            os.makedirs(os.path.dirname(path), exist_ok=True)
            rng.integers(0, 256, size, dtype=np.uint8).tofile(path)
            fl.append(path)
        out.append(fl)
    return out


def flip(path, pos, mask=0x5A):
    with open(path, "r+b") as fh:
        fh.seek(pos)
        b = fh.read(1)[0]
        fh.seek(pos)
        fh.write(bytes([b ^ mask]))


def read(path):
    with open(path, "rb") as fh:
        return fh.read()


def applied(sf, tmp, scheme, sizes, k, seed, checksums=True):
    members = make_members(tmp, sizes, seed)
    res = sf.apply_set(scheme, members, os.path.join(tmp, "ckpt."), encoding=k, slice_bytes=1 << 14, checksums=checksums)
    return members, res


def check_sidecars(res, members, k):
    """Every member has one; all are the same text; its CRCs are zlib's."""
    reds, hs, chunk = res["redundancy"], res["header_bytes"], res["chunk"]
    texts = [read(r + ".crc") for r in reds]
    assert len(set(texts)) == 1
    doc = json.loads(texts[0])
    assert doc["ranks"] == len(reds) and doc["chunk"] == chunk and doc["encoding"] == k
    for m in doc["members"]:
        r = m["rank"]
        assert [f[0] for f in m["files"]] == members[r]
        for path, size, crc in m["files"]:
            assert size == os.path.getsize(path) and crc == zlib.crc32(read(path)), path
        assert m["payload"] == zlib.crc32(read(reds[r])[hs[r]:hs[r] + k * chunk])
        assert res["checksums"][r]["payload"] == m["payload"]
        assert [list(f) for f in res["checksums"][r]["files"]] == m["files"]


def test_xor_names_the_member(sf, tmp_path):
    tmp = str(tmp_path)
    sizes = [[40_000, 25_001], [65_000], [3_000, 50_000, 7], [64_999]]
    members, res = applied(sf, tmp, "XOR", sizes, 1, seed=41)
    reds = res["redundancy"]
    check_sidecars(res, members, 1)
    v = sf.verify_set(reds, checksums=True)
    assert v["clean"] and v["checksum_damaged"] == [] and v["damaged"] == []
    flip(members[2][1], 12_345)  # member 2's second data file
    v = sf.verify_set(reds, checksums=True)
    assert not v["clean"]
    assert v["checksum_damaged"] == [{"member": 2, "kind": "data", "file": members[2][1]}]
    assert len(v["damaged"]) == 1 and v["damaged"][0]["member"] == 2 and v["damaged"][0]["kind"] == "data"
    plain = sf.verify_set(reds)
    assert not plain["clean"] and "checksum_damaged" not in plain
    assert [d["member"] for d in plain["damaged"]] == [None]
    assert plain["damaged"][0]["stripe"] == v["damaged"][0]["stripe"]


def test_rs_two_members_in_one_column(sf, tmp_path):
    tmp = str(tmp_path)
    p, k = 6, 2
    sizes = [[120_000]] * p
    members, res = applied(sf, tmp, "RS", sizes, k, seed=42)
    reds, chunk = res["redundancy"], res["chunk"]
    before = {f: read(f) for fl in members for f in fl}
    before.update({r: read(r) for r in reds})
    before.update({r + ".crc": read(r + ".crc") for r in reds})
    # members 1 and 4 hold data in stripe 0 (parity there is with members 0 and 5): same cell offset in both
    from redset_amd.codec import RSCodec

    codec = RSCodec(p, k)
    assert codec.encoding_id(1, 0) < p and codec.encoding_id(4, 0) < p
    off = 777
    flip(members[1][0], codec.data_id(1, 0) * chunk + off, 0x11)
    flip(members[4][0], codec.data_id(4, 0) * chunk + off, 0x2C)
    v = sf.verify_set(reds, checksums=True)
    assert not v["clean"]
    assert v["checksum_damaged"] == [{"member": 1, "kind": "data", "file": members[1][0]},
                                     {"member": 4, "kind": "data", "file": members[4][0]}]
    assert [d["stripe"] for d in v["damaged"]] == [0] and v["damaged"][0]["offset"] == off
    # repair: remove both members' files, rebuild with the check on
    for r in (1, 4):
        os.remove(members[r][0])
        os.remove(reds[r])
        os.remove(reds[r] + ".crc")
    out = sf.rebuild_set(reds, checksums=True)
    assert out["missing"] == [1, 4] and out["ok"] and out["checksum_damaged"] == [], out["errors"]
    for path, data in before.items():
        assert read(path) == data, path
    v = sf.verify_set(reds, checksums=True)
    assert v["clean"] and v["checksum_damaged"] == []


def test_rebuild_from_a_damaged_survivor_is_noticed(sf, tmp_path):
    tmp = str(tmp_path)
    p, k = 4, 2
    sizes = [[30_000, 9_000], [39_000], [38_500], [20_000, 19_000]]
    members, res = applied(sf, tmp, "RS", sizes, k, seed=43)
    reds = res["redundancy"]
    flip(members[0][0], 4_321)  # survivor 0, silently: its data cell 0
    # the stripe of that cell, and what member 2 holds there: that is what the rebuild gets wrong
    from redset_amd.codec import RSCodec

    codec = RSCodec(p, k)
    stripe, = [c for c in range(p) if codec.encoding_id(0, c) < p and codec.data_id(0, c) == 0]
    if codec.encoding_id(2, stripe) < p:
        pos, kind, n = codec.data_id(2, stripe) * res["chunk"], "data", 0
        while pos >= sizes[2][n]:
            pos, n = pos - sizes[2][n], n + 1
        wrong = members[2][n]
    else:
        kind, wrong = "parity", reds[2]
    for f in members[2]:
        os.remove(f)
    os.remove(reds[2])
    out = sf.rebuild_set(reds, checksums=True)
    assert out["missing"] == [2] and out["ok"] is False
    assert out["checksum_damaged"] == [{"member": 2, "kind": kind, "file": wrong}]
    assert len(out["errors"]) == 1 and wrong in out["errors"][0], out["errors"]
    # without the check: the same wrong rebuild, reported as today
    for f in members[2]:
        os.remove(f)
    os.remove(reds[2])
    plain = sf.rebuild_set(reds)
    assert plain["missing"] == [2] and plain["ok"] is True and plain["errors"] == []
    assert "checksum_damaged" not in plain


def test_lost_sidecar_comes_back(sf, tmp_path):
    tmp = str(tmp_path)
    sizes = [[10_000], [9_999, 1], [7_000], [10_000]]
    members, res = applied(sf, tmp, "XOR", sizes, 1, seed=44)
    reds = res["redundancy"]
    side = read(reds[0] + ".crc")
    data = read(members[0][0])
    for f in (members[0][0], reds[0], reds[0] + ".crc"):
        os.remove(f)
    out = sf.rebuild_set(reds, checksums=True)
    assert out["ok"] and out["missing"] == [0], out["errors"]
    assert read(reds[0] + ".crc") == side and read(members[0][0]) == data
    assert sf.verify_set(reds, checksums=True)["clean"]


def test_no_sidecar_is_an_error(sf, tmp_path):
    members, res = applied(sf, str(tmp_path), "XOR", [[5_000]] * 3, 1, seed=45, checksums=False)
    assert sf.verify_set(res["redundancy"])["clean"]
    with pytest.raises(ValueError):
        sf.verify_set(res["redundancy"], checksums=True)


def test_redundancy_files_do_not_change(sf, tmp_path):
    a, b = os.path.join(str(tmp_path), "a"), os.path.join(str(tmp_path), "b")
    sizes = [[20_000, 77], [1], [15_000], [0, 12_345]]
    out = {}
    for tmp, on in ((a, False), (b, True)):
        os.makedirs(tmp)
        members, res = applied(sf, tmp, "RS", sizes, 2, seed=46, checksums=on)
        out[on] = ([read(r) for r in res["redundancy"]], res)
        side = [f for f in os.listdir(tmp) if f.endswith(".crc")]
        assert len(side) == (4 if on else 0)
        assert ("checksums" in res) == on
    hs = out[True][1]["header_bytes"]
    assert hs == out[False][1]["header_bytes"]
    for r in range(4):
        # the headers name the data files, which live in two directories: the same length, and
        # everything after them -- the parity -- byte for byte
        assert len(out[False][0][r]) == len(out[True][0][r])
        assert out[False][0][r][hs[r]:] == out[True][0][r][hs[r]:]


def test_same_set_applied_twice_is_byte_identical(sf, tmp_path):
    """One directory, apply_set without and then with checksums: the
    redundancy files, headers included, do not differ by a byte (where the
    file system leaves the data files' access times alone between the two)."""
    tmp = str(tmp_path)
    members = make_members(tmp, [[20_000, 77], [1], [15_000], [0, 12_345]], seed=47)
    stamp = lambda: [os.stat(f).st_atime_ns for fl in members for f in fl]  # noqa: E731
    t0 = stamp()
    plain = sf.apply_set("RS", members, os.path.join(tmp, "ckpt."), encoding=2)
    first = [read(r) for r in plain["redundancy"]]
    assert not [f for f in os.listdir(tmp) if f.endswith(".crc")]
    t1 = stamp()
    with_crc = sf.apply_set("RS", members, os.path.join(tmp, "ckpt."), encoding=2, checksums=True)
    assert with_crc["redundancy"] == plain["redundancy"] and with_crc["header_bytes"] == plain["header_bytes"]
    second = [read(r) for r in with_crc["redundancy"]]
    hs = plain["header_bytes"]
    for r in range(4):
        assert first[r][hs[r]:] == second[r][hs[r]:]
        if t0 == t1:  # the headers record the access times
            assert first[r] == second[r]
    assert len([f for f in os.listdir(tmp) if f.endswith(".crc")]) == 4
