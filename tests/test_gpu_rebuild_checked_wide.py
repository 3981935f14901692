"""GPU tests of the wide checked rebuild (include/redset_hip.h, "checked
rebuild, wide"; gf_rebuild_checked_wide_kernel<S>, S = 1..7). The reference is
the undamaged set as the CPU oracle encodes it: a column with at most
max_errors wrong survivor bytes must be rebuilt (and, with fix_survivors,
restored) to it. A column with more is placed only where detection is
guaranteed (nu + max_errors <= s): it must be counted unlocated and hold the
CPU oracle's plain rebuild of the damaged survivors. After every execute the
WHOLE device allocation, sentinel padding included, must equal the prediction
byte for byte, and the reports what the injected damage implies.

Chunk 4117 = 257 vectors + 5 tail bytes (more than one 256-lane step); (40, 6)
has more than 16 survivors; `shift` starts the image one byte off alignment
(byte path throughout), chunk 15 has no whole vector; (248, 8) at chunk 48 is
the largest table set in LDS."""
import os

import numpy as np
import pytest

import rebuild_checked_ref as ref
import repair_ref
import repair_wide_ref as wref
from rebuild_checked_ref import NO, Dev, clean_image, lose
from test_gpu_rebuild_checked_stream import host_set
from test_gpu_repair_setfiles import make_set, read, xor_at

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

# (p, e, lost, chunk, shift): s = 4, 2, 5, 7, 1, 4, 5, 5, 7
CASES = [(8, 5, [1], 4117, 0), (8, 5, [0, 3, 6], 4117, 0), (10, 6, [2], 4117, 0), (12, 8, [4], 4117, 0),
         (12, 7, [1, 5, 6, 9, 10, 11], 4117, 0), (40, 6, [3, 20], 4117, 0), (10, 6, [2], 4117, 1),
         (10, 6, [2], 15, 0), (248, 8, [5], 48, 1)]


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


def damage(oracle, codec, clean, lost, chunk):
    """In stripes 0, e and p - 1, in surviving data and parity cells alike:
    runs of 1, 16 and 300 columns (as far as the chunk goes) in which wrong
    member i of t starts i * len // 8 columns into the run, so nu goes 1..t
    along it; one wrong byte in the last column; and, only where s is odd,
    columns with t + 1 wrong bytes. -> (image, {stripe: wrong[p, chunk] bool})"""
    p, e = codec.ranks, codec.encoding
    s = e - len(lost)
    t = s // 2
    rng = np.random.default_rng(p + e + chunk + s)
    img, plan = clean.copy(), {}
    runs = [(5, 1), (1003, 16), (2000, 300)] if chunk > 2400 else [(5, 1), (9, 16)]
    hard = ([3000, 3001, chunk - 3] if chunk > 3100 else [40] if chunk > 40 else [3]) if s % 2 else []
    for c in (0, e, p - 1):
        st = repair_ref.Stripe(oracle, codec, c)
        data, par = ([m for m in ms if m not in lost] for ms in wref.members_of(st))
        mem = list(dict.fromkeys(data[:1] + par[:1] + data[-1:] + par[-1:] + data + par))[:t + 1]
        wrong = np.zeros((p, chunk), bool)
        for x0, n in runs:
            for i, m in enumerate(mem[:t]):
                wrong[m, x0 + i * n // 8:x0 + n] = True
        wrong[mem[0], chunk - 1] = True
        for col in hard:
            wrong[mem, col] = True
        for m in range(p):
            cols = np.nonzero(wrong[m])[0]
            img[m, st.index[m], cols] ^= rng.integers(1, 256, cols.size, dtype=np.uint8)
        plan[c] = wrong
    return img, plan


def predict(oracle, codec, clean, img, plan, lost, chunk, max_errors):
    """(report, image after fix_survivors=False, image after fix_survivors=True)"""
    p, e = codec.ranks, codec.encoding
    assert all(int(w.sum(axis=0).max()) + max_errors <= e - len(lost) for w in plan.values())  # detection is guaranteed
    corrected, first = np.zeros((p, p), np.uint64), np.full((p, p), NO, np.uint64)
    unloc, first_un, multi = np.zeros(p, np.uint64), np.full(p, NO, np.uint64), np.zeros((p, 2), np.uint64)
    plain = ref.oracle_rebuild(oracle, img, e, lost, chunk)
    kept, fixed = img.copy(), clean.copy()
    kept[lost] = clean[lost]
    for c, wrong in plan.items():
        st = repair_ref.Stripe(oracle, codec, c)
        nu = wrong.sum(axis=0)
        ok = (nu > 0) & (nu <= max_errors)
        for m in range(p):
            cols = np.nonzero(wrong[m] & ok)[0]
            if cols.size:
                corrected[c, m], first[c, m] = cols.size, cols.min()
        un = np.nonzero(nu > max_errors)[0]
        if un.size:
            unloc[c], first_un[c] = un.size, un.min()
        for m in range(p):  # an unlocated column: the plain rebuild's bytes, survivors as they are
            src = plain if m in lost else img
            kept[m, st.index[m], un] = src[m, st.index[m], un]
            fixed[m, st.index[m], un] = src[m, st.index[m], un]
        for k in (2, 3):
            multi[c, k - 2] = np.count_nonzero(ok & (nu == k))
    return (corrected, first, unloc, first_un, multi), kept, fixed


def run(pl):
    pl.execute()
    torch.cuda.synchronize()
    return pl.report()


def check_report(got, want):
    for g, w, name in zip(got, want, ("corrected", "first", "unlocated", "first_unlocated", "multi_columns")):
        assert np.array_equal(g, w), f"{name}: got {g.tolist()} want {w.tolist()}"


def setup(rd, oracle, p, e, lost, chunk, max_errors=None):
    clean = clean_image(oracle, p, e, chunk, chunk < 256)
    codec = rd.RSCodec(p, e)
    img, plan = damage(oracle, codec, clean, lost, chunk)
    t = (e - len(lost)) // 2 if max_errors is None else max_errors
    want, kept, fixed = predict(oracle, codec, clean, img, plan, lost, chunk, t)
    return codec, clean, img, lose(img, lost, chunk), want, kept, fixed


@pytest.mark.parametrize("p,e,lost,chunk,shift", CASES)
def test_rebuild_then_fix_survivors(rd, oracle, p, e, lost, chunk, shift):
    codec, clean, img, start, want, kept, fixed = setup(rd, oracle, p, e, lost, chunk)
    k, t = len(lost), (e - len(lost)) // 2
    if t:
        assert want[0].any() and (t < 2 or want[4][e, t - 2] > 0)  # columns with t wrong bytes are corrected
    assert want[2].any() == bool((e - k) % 2)
    for fix, expect in ((False, kept), (True, fixed)):
        dev = Dev(start, chunk, e, shift)
        pl = codec.plan_rebuild_checked_wide(lost, dev.lofi(), dev.parity(), chunk, dev.stride, fix_survivors=fix)
        assert (pl.info.kind, pl.info.jobs, pl.bytes_read, pl.bytes_written) == (12, p, p * (p - k) * chunk, p * k * chunk)
        check_report(run(pl), want)
        assert np.array_equal(dev.download(), dev.expect(expect)), f"fix_survivors={fix}"


def test_clean_survivors_equal_the_plain_rebuild(rd, oracle):
    p, e, lost, chunk = 10, 6, [2], 4117
    clean = clean_image(oracle, p, e, chunk)
    codec = rd.RSCodec(p, e)
    start = lose(clean, lost, chunk)
    dev, plain = Dev(start, chunk, e), Dev(start, chunk, e)
    got = run(codec.plan_rebuild_checked_wide(lost, dev.lofi(), dev.parity(), chunk, dev.stride, fix_survivors=True))
    assert not got[0].any() and not got[2].any() and not got[4].any()
    codec.plan_rebuild(lost, plain.lofi(), plain.parity(), chunk, plain.stride).execute()
    assert np.array_equal(dev.download(), plain.download()) and np.array_equal(dev.download(), dev.expect(clean))


def test_max_errors_1_leaves_the_multi_columns(rd, oracle):
    p, e, lost, chunk = 10, 6, [2], 4117
    codec, clean, img, start, want, kept, fixed = setup(rd, oracle, p, e, lost, chunk, max_errors=1)
    assert want[2][0] > 200 and not want[4].any()  # the nu >= 2 columns of the runs
    dev = Dev(start, chunk, e)
    pl = codec.plan_rebuild_checked_wide(lost, dev.lofi(), dev.parity(), chunk, dev.stride, fix_survivors=True,
                                         max_errors=1)
    check_report(run(pl), want)
    assert np.array_equal(dev.download(), dev.expect(fixed))


def test_stream_over_host_memory(rd, oracle):
    p, e, lost, chunk = 10, 6, [2], 4117
    codec, clean, img, start, want, kept, fixed = setup(rd, oracle, p, e, lost, chunk)
    for fix, expect in ((False, kept), (True, fixed)):
        t, io = host_set(rd, start, e, True)
        out = rd.rs_rebuild_checked_wide_stream(codec, lost, chunk, io, slice_bytes=2048, fix_survivors=fix)
        io.close()
        check_report((out["corrected"], out["first"], out["unlocated"], out["first_unlocated"]), want)
        assert out["multi_columns"] == want[4].sum(axis=0).tolist()
        assert out["corrected_bytes"] == want[0].sum() and out["unlocated_columns"] == want[2].sum()
        assert np.array_equal(t.numpy().reshape(img.shape), expect), f"fix_survivors={fix}"


def test_rebuild_set_files_with_checksums(rd, oracle, tmp_path):
    from redset_amd import setfiles as sf

    p, e, lost = 10, 6, 9
    members, res = make_set(sf, str(tmp_path), k=e, checksums=True, sizes=[[9000]] * 8 + [[5000, 3999], [8000]])
    reds, chunk = res["redundancy"], res["chunk"]
    everything = [f for fl in members for f in fl] + reds
    saved = {f: read(f) for f in everything}
    st = repair_ref.Stripe(oracle, rd.RSCodec(p, e), 1)
    a, b = [m for m in wref.members_of(st)[0] if m < 8][:2]
    xor_at(members[a][0], st.index[a] * chunk + 300, [0x5A] * 40)
    xor_at(members[b][0], st.index[b] * chunk + 300, list(range(101, 141)))
    for f in members[lost] + [reds[lost], reds[lost] + ".crc"]:
        os.remove(f)
    with pytest.raises(ValueError, match="2..4"):
        sf.rebuild_set(reds, check_survivors=True)
    out = sf.rebuild_set(reds, check_survivors=True, wide=True, checksums=True, fix_survivors=True)
    assert out["ok"] and out["trusted"] and out["multi_columns"] == [40, 0] and out["checksum_damaged"] == []
    assert sorted((d["member"], d["bytes"], d["first_offset"]) for d in out["survivor_corrections"]) == \
        sorted([(a, 40, 300), (b, 40, 300)])
    assert {f: read(f) for f in everything} == saved


def test_refusals(rd, tmp_path):
    from redset_amd import setfiles as sf

    lay = rd.SetLayout.allocate(20, 16, 4, 64, device="cuda")
    args = (lay.lofi_ptrs(), lay.parity_ptrs(), 64, lay.cell_stride)
    with pytest.raises(ValueError, match="5..8"):
        rd.RSCodec(20, 4).plan_rebuild_checked_wide([1], *args)
    members, res = make_set(sf, str(tmp_path), k=3, sizes=[[500]] * 11)
    os.remove(members[0][0])
    with pytest.raises(ValueError, match="5..8"):
        sf.rebuild_set(res["redundancy"], check_survivors=True, wide=True)
    codec = rd.RSCodec(10, 6)
    with pytest.raises(ValueError, match="1..5"):  # k = e
        codec.plan_rebuild_checked_wide([0, 1, 2, 3, 4, 5], *args)
    with pytest.raises(ValueError, match="1..2"):
        codec.plan_rebuild_checked_wide([2], *args, max_errors=3)
    with pytest.raises(ValueError, match="0..0"):
        codec.plan_rebuild_checked_wide([0, 1, 2, 3, 4], *args, max_errors=1)
