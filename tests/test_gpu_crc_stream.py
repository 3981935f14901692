"""GPU tests of redset_hip_crc32_stream (include/redset_hip.h): CRC-32 of
spans of a host-resident set, in memory (staged and page-locked) and in files
with the logical-file layout, against zlib.crc32 of the same bytes."""
import os
import zlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

DATA, PARITY = 0, 1


@pytest.fixture(scope="module")
def rd():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import redset_amd

    redset_amd.load()
    return redset_amd


def host_set(p, d, e, chunk, pinned, seed):
    """Random members in host memory, cells `stride` apart: (lofi, parity
    arrays of the cells' bytes only, the io)."""
    from redset_amd import stream

    stride = -(-chunk // 256) * 256
    rng = np.random.default_rng(seed)
    store = torch.empty(p * (d + e) * stride, dtype=torch.uint8)
    if pinned:
        store = store.pin_memory()
    view = store.numpy()
    view[:] = rng.integers(0, 256, view.size, dtype=np.uint8)
    cells = view.reshape(p, d + e, stride)
    lofi = [np.ascontiguousarray(cells[r, :d, :chunk]).reshape(-1) for r in range(p)]
    parity = [np.ascontiguousarray(cells[r, d:, :chunk]).reshape(-1) for r in range(p)]
    base = store.data_ptr()
    member = (d + e) * stride
    io = stream.HostIO(p, [base + r * member for r in range(p)], [base + r * member + d * stride for r in range(p)],
                       stride, keepalive=store, pinned=pinned)
    return lofi, parity, io


@pytest.mark.parametrize("pinned", [False, True])
def test_host_spans(rd, pinned):
    from redset_amd import stream

    p, e, chunk = 4, 2, 4096 + 7
    d = p - e
    lofi, parity, io = host_set(p, d, e, chunk, pinned, seed=21)
    whole = d * chunk
    spans = [
        (0, DATA, 0, whole),                   # a whole logical file: every cell, many slices
        (1, DATA, 1500, 700),                  # starts mid-cell, inside one slice
        (1, DATA, 1000, 2 * chunk - 1000 - 5),  # mid-cell to short of the end: crosses a cell and slices
        (2, DATA, chunk - 1, 2),               # one byte either side of a cell boundary
        (2, DATA, 77, 0),                      # empty
        (3, DATA, 0, whole - 301),             # the whole file minus a ragged tail
        (3, DATA, 100, whole - 500),           # overlaps the one before
        (0, DATA, 1024, 1024),                 # exactly one slice
        (0, PARITY, 0, e * chunk),             # a member's whole payload
        (2, PARITY, chunk - 3, chunk),         # across its two parity cells
        (1, PARITY, 5, 0),
        (3, PARITY, 2048, 1),
    ]
    res = stream.crc32_stream(chunk, io, spans, slice_bytes=1024)
    want = [zlib.crc32((lofi if k == DATA else parity)[r][o:o + n].tobytes()) for r, k, o, n in spans]
    assert res["crcs"] == want
    total = sum(n for _, _, _, n in spans)
    assert res["stats"]["bytes_read"] == total and res["stats"]["bytes_written"] == 0
    assert res["stats"]["units"] >= (1 if pinned else 2)
    # the default slice, and no spans at all
    assert stream.crc32_stream(chunk, io, spans[:4])["crcs"] == want[:4]
    assert stream.crc32_stream(chunk, io, [])["crcs"] == []
    io.close()


def test_file_spans(rd, tmp_path):
    """Members of 1 to 3 files whose boundaries fall inside cells, a
    zero-length file and a short member: a file's span ends where the file
    does, so the logical file's zero padding is in no file's CRC -- while a
    span over the padding reads it as zeros."""
    from redset_amd import stream

    p, e = 4, 2
    d = p - e
    sizes = [[5000, 3211], [8211], [100, 0, 4000], [37]]
    chunk = stream.chunk_size_for(max(sum(s) for s in sizes), d)
    assert chunk == 4106 and all(s[0] % chunk for s in sizes)
    rng = np.random.default_rng(31)
    files, blobs, reds, payload = [], [], [], []
    for r in range(p):
        fl, bl = [], []
        for i, n in enumerate(sizes[r]):
            path = os.path.join(str(tmp_path), f"m{r}_f{i}.dat")
            b = rng.integers(0, 256, n, dtype=np.uint8).tobytes()
            with open(path, "wb") as fh:
                fh.write(b)
            fl.append((path, n))
            bl.append(b)
        files.append(fl)
        blobs.append(bl)
        red = os.path.join(str(tmp_path), f"m{r}.red")
        pay = rng.integers(0, 256, e * chunk, dtype=np.uint8).tobytes()
        with open(red, "wb") as fh:
            fh.write(bytes(100 + r) + pay)  # a header of 100 + r bytes, not part of the payload
        reds.append(red)
        payload.append(pay)
    io = stream.FileIO(files, reds, [100 + r for r in range(p)], chunk)
    spans, want = [], []
    for r in range(p):
        pos = 0
        for b in blobs[r]:
            spans.append((r, DATA, pos, len(b)))
            want.append(zlib.crc32(b))
            pos += len(b)
        spans.append((r, PARITY, 0, e * chunk))
        want.append(zlib.crc32(payload[r]))
    # the short member's whole logical file: its 37 bytes, then zeros
    spans.append((3, DATA, 0, d * chunk))
    want.append(zlib.crc32(blobs[3][0] + bytes(d * chunk - 37)))
    res = stream.crc32_stream(chunk, io, spans, slice_bytes=1024)
    io.close()
    assert res["crcs"] == want
    assert spans[6] == (2, DATA, 100, 0) and want[6] == 0  # member 2's zero-length file


def test_a_failing_read_fails_the_call(rd, tmp_path):
    """A data file shorter than recorded: the read fails, the call fails."""
    from redset_amd import _lib, stream

    path = os.path.join(str(tmp_path), "short.dat")
    with open(path, "wb") as fh:
        fh.write(bytes(1000))
    red = os.path.join(str(tmp_path), "short.red")
    with open(red, "wb") as fh:
        fh.write(bytes(4096))
    io = stream.FileIO([[(path, 3000)]], [red], [0], 2048)
    with pytest.raises(_lib.RedsetHipError):
        stream.crc32_stream(2048, io, [(0, DATA, 0, 3000)], slice_bytes=512)
    io.close()
