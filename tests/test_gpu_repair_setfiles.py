"""GPU tests of setfiles.repair_set: sets on disk written by apply_set,
damaged in their files, repaired in place. Expected bytes are the saved
copies of the files; the expected members, kinds and counts follow from where
the test put the damage (one wrong byte per column), and the e = 2
miscorrection from the brute-force numpy locate (tests/repair_ref.py)."""
import os

import numpy as np
import pytest

import repair_ref

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

# several files per member, sizes that are no multiple of the chunk, member 3
# shorter than the others: its logical file ends in zero padding
SIZES = [[40_000, 25_001], [65_000], [3_000, 50_000, 7], [41_234]]


@pytest.fixture(scope="module")
def sf():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import redset_amd
    from redset_amd import setfiles

    redset_amd.load()
    return setfiles


def make_set(sf, tmp, scheme="RS", k=2, checksums=False, sizes=SIZES):
    rng = np.random.default_rng(11)
    members = []
    for r, fs in enumerate(sizes):
        fl = []
        for i, size in enumerate(fs):
            path = os.path.join(tmp, "data", f"rank{r}_file{i}.dat")
            os.makedirs(os.path.dirname(path), exist_ok=True)
            rng.integers(0, 256, size, dtype=np.uint8).tofile(path)
            fl.append(path)
        members.append(fl)
    res = sf.apply_set(scheme, members, os.path.join(tmp, "ckpt."), encoding=k, slice_bytes=1 << 14,
                       checksums=checksums)
    return members, res


def read(path):
    with open(path, "rb") as fh:
        return fh.read()


def xor_at(path, pos, values):
    with open(path, "r+b") as fh:
        fh.seek(pos)
        old = fh.read(len(values))
        fh.seek(pos)
        fh.write(bytes(a ^ b for a, b in zip(old, values)))


def stat3(path):
    s = os.stat(path)
    return s.st_size, s.st_mtime_ns, s.st_ino


def test_repair_set_in_place(sf, tmp_path):
    import redset_amd

    members, res = make_set(sf, str(tmp_path))
    reds, hs, chunk = res["redundancy"], res["header_bytes"], res["chunk"]
    assert chunk == 32_501  # ceil(65001 / 2)
    everything = [f for fl in members for f in fl] + reds
    saved = {f: read(f) for f in everything}
    codec = redset_amd.RSCodec(4, 2)
    # member 0: 300 bytes across its file boundary (logical 39900..40200, inside data cell 1 = columns 7399..7699);
    # member 2: 50 bytes of its second file (logical 3000+17000 = cell 0, columns 20000..20050);
    # member 1: 40 bytes of its redundancy payload, slot 1 (columns 100..140)
    xor_at(members[0][0], 39_900, [0x11] * 100)
    xor_at(members[0][1], 0, [0x22] * 200)
    xor_at(members[2][1], 17_000, [0x33] * 50)
    xor_at(reds[1], hs[1] + chunk + 100, [0x44] * 40)
    damaged = {f: read(f) for f in everything}

    def cell_stripe(member, kind_data, index):
        for c in range(4):
            enc = codec.encoding_id(member, c)
            if kind_data and enc < 4 and codec.data_id(member, c) == index:
                return c
            if not kind_data and enc == 4 + index:
                return c
        raise AssertionError

    expect = {}  # stripe -> {member: (kind, bytes, first)}
    expect.setdefault(cell_stripe(0, True, 1), {})[0] = ("data", 300, 39_900 - chunk)
    expect.setdefault(cell_stripe(2, True, 0), {})[2] = ("data", 50, 20_000)
    expect.setdefault(cell_stripe(1, False, 1), {})[1] = ("parity", 40, 100)

    def check(out, applied):
        assert out["scheme"] == "RS" and out["corrected_bytes"] == 390 and out["unlocated_columns"] == 0
        assert out["verify_mismatch_bytes"] > 0 and out["damaged_stripes"] == len(expect)
        got = {d["stripe"]: {m["member"]: (m["kind"], m["corrected_bytes"], m["first_offset"]) for m in d["members"]}
               for d in out["damaged"]}
        assert got == expect
        assert all(d["unlocated_columns"] == 0 for d in out["damaged"])
        assert out["repaired"] == applied
        assert out["remaining_mismatch_bytes"] == (0 if applied else out["verify_mismatch_bytes"])

    before = {f: stat3(f) for f in everything}
    check(sf.repair_set(reds, slice_bytes=1 << 14, apply=False), False)
    assert {f: read(f) for f in everything} == damaged
    assert {f: stat3(f) for f in everything} == before  # a dry run opens nothing for writing
    out = sf.repair_set(reds, slice_bytes=1 << 14)
    check(out, True)
    assert out["cells_written"] == 3 + (1 if 7399 // (1 << 14) != 7698 // (1 << 14) else 0)
    for f in everything:
        assert read(f) == saved[f], f
    # member 3 needed nothing: its data file and redundancy file are as they were; so is
    # every redundancy file's header, and the redundancy files of members 0 and 2 whole
    for f in members[3] + [reds[3], reds[0], reds[2]]:
        assert stat3(f) == before[f], f
    for r in range(4):
        assert read(reds[r])[:hs[r]] == saved[reds[r]][:hs[r]]
    v = sf.verify_set(reds)
    assert v["clean"] and v["damaged"] == []
    again = sf.repair_set(reds)
    assert again["repaired"] and again["repair_units"] == 0 and again["damaged"] == []


def test_checksums_arbitrate(sf, oracle, tmp_path):
    import redset_amd

    members, res = make_set(sf, str(tmp_path), checksums=True)
    reds, hs, chunk = res["redundancy"], res["header_bytes"], res["chunk"]
    everything = [f for fl in members for f in fl] + reds
    saved = {f: read(f) for f in everything}
    # single damage: repaired, and the recorded CRCs agree
    xor_at(members[1][0], 1234, [0x77] * 9)
    out = sf.repair_set(reds, checksums=True)
    assert out["repaired"] and out["checksum_damaged"] == [] and out["corrected_bytes"] == 9
    assert {f: read(f) for f in everything} == saved
    # two members wrong in one column of stripe c, with values the numpy oracle says look like a
    # third member's single error: the parity check passes after the "repair", the CRCs do not
    codec = redset_amd.RSCodec(4, 2)
    c = 0
    st = repair_ref.Stripe(oracle, codec, c)
    a, b = [m for m in range(4) if st.row[m] < 0]  # the stripe's two data members
    x1, x2, t, x3 = repair_ref.miscorrecting_pair(st, a, b)
    assert t not in (a, b)
    col = 77
    for m, x in ((a, x1), (b, x2)):
        pos = st.index[m] * chunk + col  # in the member's logical file
        for path in members[m]:
            if pos < os.path.getsize(path):
                xor_at(path, pos, [x])
                break
            pos -= os.path.getsize(path)
        else:
            raise AssertionError("the column lies in the member's zero padding")
    out = sf.repair_set(reds, checksums=True)
    assert out["remaining_mismatch_bytes"] == 0 and out["unlocated_columns"] == 0 and out["corrected_bytes"] == 1
    assert out["damaged"][0]["stripe"] == c and out["damaged"][0]["members"][0]["member"] == t
    assert out["repaired"] is False
    bad = {(d["member"], d["kind"]) for d in out["checksum_damaged"]}
    assert (a, "data") in bad and (b, "data") in bad and (t, st.kind(t)) in bad


def test_refusals(sf, tmp_path):
    members, res = make_set(sf, str(tmp_path / "rs"), sizes=[[5000], [6000], [7000], [4000]])
    os.remove(members[2][0])
    with pytest.raises(ValueError, match="rebuild_set"):
        sf.repair_set(res["redundancy"])
    _, res = make_set(sf, str(tmp_path / "xor"), scheme="XOR", k=1, sizes=[[5000], [6000], [7000]])
    with pytest.raises(ValueError, match="sidecar"):
        sf.repair_set(res["redundancy"])
    _, res = make_set(sf, str(tmp_path / "rs1"), k=1, sizes=[[5000], [6000], [7000]])
    with pytest.raises(ValueError, match="sidecar"):
        sf.repair_set(res["redundancy"])
