"""Redundancy sets on disk, in one process: write every member's redundancy
file (header + parity chunks) and rebuild lost members from whatever
redundancy files survive, learning the set from their headers.

This is the file-level job of redset_apply over a whole set
(src/redset_reedsolomon.c:405-566, src/redset_xor.c:298-439) and of the
single-process rebuild redset_rebuild_rs / redset_rebuild_xor
(src/redset_reedsolomon_serial.c:345-693, src/redset_xor_serial.c:277-622),
with the byte work done by the HIP streaming pipeline (redset_amd.stream:
files -> pinned host buffers -> HBM -> gf_mac / xor kernels -> files).
Headers: redset_amd.header (tree content pinned by the reference's documented
examples; KVTree's byte layout unpinned)."""
from __future__ import annotations

import json
import os
from typing import Dict, List, Optional, Sequence

from . import header as H
from . import stream


def _codec(scheme: str, ranks: int, encoding: int):
    if scheme == "RS":
        from .codec import RSCodec

        return RSCodec(ranks, encoding)
    return None


SIDECAR_SUFFIX = ".crc"


def _checksum_table(files, reds, hsize, chunk: int, k: int, slice_bytes: int = 0, members=None) -> Dict[int, Dict]:
    """CRC-32 of every data file and of the redundancy payload (the k parity
    chunks after the header) of the listed members (default: all), in one
    crc32_stream pass over the files: {member: {"files": [[name, size, crc],
    ...], "payload": crc}}. A file's span is its own bytes in the member's
    logical file, so the zero padding after the last file is in no CRC."""
    members = list(range(len(files))) if members is None else list(members)
    spans, where = [], []
    for r in members:
        pos = 0
        for i, (_, size) in enumerate(files[r]):
            spans.append((r, 0, pos, size))
            where.append((r, i))
            pos += size
        spans.append((r, 1, 0, k * chunk))
        where.append((r, None))
    io = stream.FileIO(files, reds, hsize, chunk)
    try:
        crcs = stream.crc32_stream(chunk, io, spans, slice_bytes=slice_bytes)["crcs"]
    finally:
        io.close()
    table = {r: {"files": [[path, size, None] for path, size in files[r]], "payload": None} for r in members}
    for (r, i), crc in zip(where, crcs):
        if i is None:
            table[r]["payload"] = crc
        else:
            table[r]["files"][i][2] = crc
    return table


def _write_sidecars(reds, members, scheme: str, chunk: int, k: int, table: Dict[int, Dict]) -> None:
    """The whole set's table beside the redundancy file of every member of
    ``members``: any loss the set survives leaves a copy, as every header
    carries every member's descriptor."""
    doc = {"format": 1, "checksum": "crc32", "scheme": scheme, "ranks": len(reds), "encoding": k, "chunk": chunk,
           "members": [{"rank": r, "files": table[r]["files"], "payload": table[r]["payload"]}
                       for r in sorted(table)]}
    text = json.dumps(doc, indent=1, sort_keys=True) + "\n"
    for r in members:
        tmp = reds[r] + SIDECAR_SUFFIX + ".tmp"
        with open(tmp, "w") as fh:
            fh.write(text)
        os.replace(tmp, reds[r] + SIDECAR_SUFFIX)


def _read_sidecar(reds, p: int, chunk: int) -> Dict[int, Dict]:
    """The table of the first readable sidecar that describes this set."""
    for red in reds:
        try:
            with open(red + SIDECAR_SUFFIX) as fh:
                doc = json.load(fh)
            if doc["checksum"] != "crc32" or doc["ranks"] != p or doc["chunk"] != chunk:
                continue
            table = {int(m["rank"]): {"files": m["files"], "payload": m["payload"]} for m in doc["members"]}
            if sorted(table) == list(range(p)):
                return table
        except (OSError, ValueError, KeyError, TypeError):
            continue
    raise ValueError("no readable checksum sidecar (" + SIDECAR_SUFFIX + ") beside any redundancy file of the set")


def _checksum_diff(stored: Dict[int, Dict], now: Dict[int, Dict], reds) -> List[Dict]:
    """What differs: [{"member", "kind": "data" | "parity", "file"}]."""
    bad = []
    for r in sorted(now):
        for i, (path, size, crc) in enumerate(now[r]["files"]):
            old = stored[r]["files"][i] if i < len(stored[r]["files"]) else None
            if old is None or old[1] != size or old[2] != crc:
                bad.append({"member": r, "kind": "data", "file": path})
        if stored[r]["payload"] != now[r]["payload"]:
            bad.append({"member": r, "kind": "parity", "file": reds[r]})
    return bad


def apply_set(scheme: str, member_files: Sequence[Sequence[str]], prefix: str, encoding: int = 1,
              world_ranks: Optional[Sequence[int]] = None, world_size: Optional[int] = None,
              group_id: int = 0, groups: int = 1, slice_bytes: int = 0, checksums: bool = False) -> Dict:
    """Encode a set whose members' data files are ``member_files[r]``: write
    member r's redundancy file ``redundancy_filename(prefix, ...)`` with its
    header and its parity chunks. Returns the file names, CHUNK and the
    pipeline statistics. ``checksums``: also write, beside every redundancy
    file, a sidecar ``<redundancy file>.crc`` with the CRC-32 of every
    member's data files and redundancy payload (one more pass over the set,
    on the GPU; the redundancy files themselves are unchanged), for
    verify_set / rebuild_set(checksums=True); the result gains
    ``"checksums"``."""
    scheme = scheme.upper()
    if scheme not in ("RS", "XOR"):
        raise ValueError(f"unknown scheme {scheme!r}")
    p = len(member_files)
    k = encoding if scheme == "RS" else 1
    wr = list(world_ranks) if world_ranks is not None else list(range(p))
    ws = world_size if world_size is not None else max(wr) + 1
    metas = [[H.FileMeta.stat(f) for f in fl] for fl in member_files]
    members = [H.member_hash(H.Descriptor(scheme, r, p, wr[r], ws, group_id, groups, k), metas[r])
               for r in range(p)]
    chunk = H.chunk_size(scheme, max(sum(m.size for m in ms) for ms in metas), p, k)
    reds, hsize = [], []
    for r in range(p):
        red = H.redundancy_filename(scheme, prefix, wr[r], group_id, groups, r, p)
        fd = os.open(red, os.O_WRONLY | os.O_CREAT | os.O_TRUNC, 0o600)
        try:
            hsize.append(H.write_header(fd, H.header_tree(scheme, r, members, wr, chunk, k)))
        finally:
            os.close(fd)
        reds.append(red)
    io = stream.FileIO([[(m.path, m.size) for m in ms] for ms in metas], reds, hsize, chunk)
    try:
        if scheme == "RS":
            st = stream.rs_encode_stream(_codec(scheme, p, k), chunk, io, slice_bytes=slice_bytes)
        else:
            st = stream.xor_encode_stream(p, chunk, io, slice_bytes=slice_bytes)
    finally:
        io.close()
    out = {"redundancy": reds, "chunk": chunk, "header_bytes": hsize, "stats": st}
    if checksums:
        files = [[(m.path, m.size) for m in ms] for ms in metas]
        out["checksums"] = _checksum_table(files, reds, hsize, chunk, k, slice_bytes)
        _write_sidecars(reds, range(p), scheme, chunk, k, out["checksums"])
    return out


def _files_ok(files) -> bool:
    """redset_lofi_check_mapped: every data file exists with its recorded
    size (src/redset_lofi.c:219-297)."""
    for path, size in files:
        try:
            if os.stat(path).st_size != size:
                return False
        except OSError:
            return False
    return True


def _apply_meta(path: str, meta: H.Tree) -> List[str]:
    """redset_meta_apply (src/redset_util.c:292-380): mode, owner, size check,
    access / modification times. Returns the failures (the reference logs
    them and reports failure)."""
    errs = []
    try:
        os.chmod(path, H.get_int(meta, "MODE") & 0o7777)
    except OSError as e:
        errs.append(f"chmod({path}): {e}")
    try:
        uid, gid = H.get_int(meta, "UID"), H.get_int(meta, "GID")
        st = os.stat(path)
        if (st.st_uid, st.st_gid) != (uid, gid):
            os.chown(path, uid, gid)
    except OSError as e:
        errs.append(f"chown({path}): {e}")
    if os.stat(path).st_size != H.get_int(meta, "SIZE"):
        errs.append(f"{path}: size {os.stat(path).st_size} expected {H.get_int(meta, 'SIZE')}")
    ns = lambda s, n: H.get_int(meta, s) * 1_000_000_000 + H.get_int(meta, n)  # noqa: E731
    os.utime(path, ns=(ns("ATIME_SECS", "ATIME_NSECS"), ns("MTIME_SECS", "MTIME_NSECS")))
    return errs


def _read_set(redundancy_files: Sequence[str]):
    """The set as its readable redundancy files' headers describe it: the
    facts, every member's redundancy file name and data files, and the lost
    members (redundancy file unreadable or shorter than header + k chunks, or
    a data file absent or the wrong size)."""
    heads, paths = [], {}
    for path in redundancy_files:
        try:
            t, n = H.read_header(path)
        except (OSError, ValueError):
            continue
        heads.append((t, n))
        paths[H.get_int(t, "RANK")] = path
    f = H.set_facts(heads)
    p, k = f.ranks, f.encoding
    # every member's redundancy file name, from a survivor's name and the descriptors
    any_rank, any_path = next(iter(paths.items()))
    d0 = f.descriptor(any_rank)
    g, gs = H.get_int(d0, "GROUP"), H.get_int(d0, "GROUPS")
    tail = H.redundancy_filename(f.scheme, "", f.world_ranks[any_rank], g, gs, any_rank, p)
    if not any_path.endswith(tail):
        raise ValueError(f"{any_path}: name does not follow the redundancy file pattern")
    prefix = any_path[:len(any_path) - len(tail)]
    reds = [paths.get(r) or H.redundancy_filename(f.scheme, prefix, f.world_ranks[r], g, gs, r, p)
            for r in range(p)]
    files = [f.files(r) for r in range(p)]

    def parity_ok(r: int) -> bool:  # header + k chunks present
        try:
            return os.stat(reds[r]).st_size >= f.header_size[r] + k * f.chunk
        except OSError:
            return False

    lost = [r for r in range(p) if not f.have_header[r] or not parity_ok(r) or not _files_ok(files[r])]
    return f, reds, files, lost


def rebuild_set(redundancy_files: Sequence[str], slice_bytes: int = 0, checksums: bool = False,
                check_survivors: bool = False, fix_survivors: bool = False) -> Dict:
    """Rebuild the lost members of one set from the redundancy files that can
    still be read (``redundancy_files`` may name lost ones too). A member is
    lost when its redundancy file is unreadable or shorter than header + k
    chunks, or one of its data files is absent or the wrong size. More lost
    members than the scheme tolerates is an error
    (src/redset_reedsolomon_serial.c:496-519). Lost members get
    their data files, file metadata and redundancy file (header regenerated
    from the set facts, so it matches what apply_set wrote) back.
    ``checksums``: with a surviving checksum sidecar (apply_set(checksums=
    True)), every rebuilt data file and redundancy payload is checked against
    it after the rebuild -- a silently damaged survivor gives a wrong rebuild,
    reported in ``errors`` (``ok`` false) -- and the lost members' sidecars
    are written again. No sidecar: a ValueError before anything is written.

    ``check_survivors``: rebuild through the checked rebuild
    (redset_amd.stream.rs_rebuild_checked_stream) instead, for an RS set with
    fewer lost members than parity rows, e <= 4: the parity rows the rebuild
    does not need check the survivors of every byte column, and one wrong
    survivor byte per column is located and kept out of the rebuilt files
    (two spare rows or more; one spare row only detects). The result gains
    ``survivor_corrections`` -- [{"member", "stripe", "bytes",
    "first_offset"}] --, ``unlocated_columns``, ``unlocated_stripes`` and
    ``trusted`` (false when any column is unlocated: its rebuilt bytes are
    the plain rebuild's). XOR sets, as many lost members as parity rows and
    e > 4 are a ValueError, never a silent plain rebuild. Survivors' data
    files are opened read-only; with ``fix_survivors`` (which needs
    check_survivors) a second pass opens for writing only the members the
    first located corrections in, and writes the corrected bytes back."""
    f, reds, files, lost = _read_set(redundancy_files)
    p, k = f.ranks, f.encoding
    out = {"scheme": f.scheme, "ranks": p, "encoding": k, "chunk": f.chunk, "missing": lost,
           "redundancy": reds, "errors": []}
    if fix_survivors and not check_survivors:
        raise ValueError("fix_survivors needs check_survivors=True")
    if not lost:
        return out
    if len(lost) > k:
        raise ValueError(f"{len(lost)} members lost but {f.scheme} tolerates {k}")
    if check_survivors:
        if f.scheme != "RS":
            raise ValueError(f"check_survivors: an {f.scheme} set has one parity row and the rebuild needs it; "
                             "nothing is left to check the survivors with")
        if k > 4:
            raise ValueError(f"check_survivors: RS set with {k} parity rows: the checked rebuild is built for 2..4")
        if len(lost) == k:
            raise ValueError(f"check_survivors: {len(lost)} members lost of {k} parity rows: the rebuild needs every "
                             "row, nothing is left to check the survivors with")
    stored = _read_sidecar(reds, p, f.chunk) if checksums else None
    hsize = [f.header_size.get(r, 0) for r in range(p)]
    for r in lost:
        for path, _ in files[r]:
            d = os.path.dirname(path)
            if d:
                os.makedirs(d, exist_ok=True)
            os.close(os.open(path, os.O_WRONLY | os.O_CREAT | os.O_TRUNC, 0o600))
        fd = os.open(reds[r], os.O_WRONLY | os.O_CREAT | os.O_TRUNC, 0o600)
        try:
            hsize[r] = H.write_header(fd, H.header_tree(f.scheme, r, f.members, f.world_ranks, f.chunk, k))
        finally:
            os.close(fd)
    if check_survivors:
        codec = _codec("RS", p, k)

        def run(writable, fix):
            cio = stream.FileIO(files, reds, hsize, f.chunk, writable=writable)
            try:
                return stream.rs_rebuild_checked_stream(codec, lost, f.chunk, cio, slice_bytes=slice_bytes,
                                                        fix_survivors=fix)
            finally:
                cio.close()

        res = run([r in lost for r in range(p)], False)
        if fix_survivors and res["corrected"].any():
            # members with a correction in one of their data cells
            data_fix = [r in lost or any(res["corrected"][c, r] and codec.encoding_id(r, c) < p for c in range(p))
                        for r in range(p)]
            res = run(data_fix, True)
        out["stats"] = res["stats"]
        out["survivor_corrections"] = [
            {"member": m, "stripe": c, "bytes": int(res["corrected"][c, m]), "first_offset": int(res["first"][c, m])}
            for c in range(p) for m in range(p) if res["corrected"][c, m]]
        out["unlocated_columns"] = int(res["unlocated_columns"])
        out["unlocated_stripes"] = [c for c in range(p) if res["unlocated"][c]]
        out["trusted"] = out["unlocated_columns"] == 0
    else:
        io = stream.FileIO(files, reds, hsize, f.chunk, writable=[r in lost for r in range(p)])
        try:
            if f.scheme == "RS":
                out["stats"] = stream.rs_rebuild_stream(_codec("RS", p, k), lost, f.chunk, io, slice_bytes=slice_bytes)
            else:
                out["stats"] = stream.xor_rebuild_stream(p, lost[0], f.chunk, io, slice_bytes=slice_bytes)
        finally:
            io.close()
    for r in lost:
        for i, (path, _) in enumerate(files[r]):
            (_, meta), = f.members[r]["FILE"][str(i)].items()
            out["errors"] += _apply_meta(path, meta)
    if stored is not None:
        now = _checksum_table(files, reds, hsize, f.chunk, k, slice_bytes, members=lost)
        out["checksum_damaged"] = _checksum_diff(stored, now, reds)
        for d in out["checksum_damaged"]:
            out["errors"].append(f"{d['file']}: rebuilt {d['kind']} of member {d['member']} does not match its "
                                 "recorded CRC-32 (a surviving member is damaged)")
        _write_sidecars(reds, lost, f.scheme, f.chunk, k, stored)
    out["ok"] = not out["errors"]
    return out


def repair_set(redundancy_files: Sequence[str], slice_bytes: int = 0, apply: bool = True,
               checksums: bool = False) -> Dict:
    """Scrub one RS set on disk (2 <= e <= 4) and correct, in place, every
    byte column with one wrong byte (redset_amd.stream.rs_repair_stream):
    only the wrong bytes' cell slices are rewritten, and members each damaged
    at different offsets are repaired even when they are more than a rebuild
    has erasures for. Driven by the headers as verify_set is. Lost members
    are rebuild_set's job and a ValueError here, as are XOR sets and e = 1
    (one parity row locates nothing: rebuild the member the checksum sidecar
    names) and e > 4.

    A dry run comes first and says which members need corrections; with
    ``apply`` only those members' data files are then opened for writing
    (redundancy files are opened as every streaming call opens them and
    written only where their payload is corrected; headers are never
    touched). Files of members with nothing to correct keep their size,
    modification time and inode. ``apply=False`` stops after the dry run.

    Returns the scheme, the summary (``verify_mismatch_bytes``,
    ``corrected_bytes``, ``unlocated_columns``, ``remaining_mismatch_bytes``,
    ``damaged_stripes``, ``repair_units``, ``cells_written``) and ``damaged``:
    per damaged stripe its number, ``members`` -- [{"member", "kind": "data" |
    "parity", "corrected_bytes", "first_offset"}] -- and
    ``unlocated_columns``. ``repaired`` is true iff nothing mismatches after
    the call and no column was unlocated.
    ``checksums``: afterwards recompute every member's CRC-32s (one
    crc32_stream pass) and compare them with the stored sidecar (apply_set(
    checksums=True); none readable: ValueError before anything is written).
    ``checksum_damaged`` lists what differs; any entry makes ``repaired``
    false -- the guard against e = 2's miscorrection of a column with two
    wrong bytes into a third member. Sidecars are not rewritten: a correct
    repair restores the recorded bytes."""
    f, reds, files, lost = _read_set(redundancy_files)
    p, k = f.ranks, f.encoding
    if lost:
        raise ValueError(f"members {lost} are lost: rebuild_set them, repair_set corrects bytes of members that are there")
    if f.scheme != "RS" or k < 2:
        raise ValueError(f"{f.scheme} set with {k} parity row(s): one row locates nothing; the tool here is a "
                         "rebuild (rebuild_set) of the member that the checksum sidecar names "
                         "(verify_set(checksums=True))")
    if k > 4:
        raise ValueError(f"RS set with {k} parity rows: repair is built for 2..4; rebuild_set the located member")
    stored = _read_sidecar(reds, p, f.chunk) if checksums else None
    hsize = [f.header_size[r] for r in range(p)]
    codec = _codec("RS", p, k)

    def run(writable, do_apply):
        io = stream.FileIO(files, reds, hsize, f.chunk, writable=writable)
        try:
            return stream.rs_repair_stream(codec, f.chunk, io, slice_bytes=slice_bytes, apply=do_apply)
        finally:
            io.close()

    res = run(None, False)
    if apply and res["corrected"].any():
        # members with a correction in one of their data cells
        data_fix = [any(res["corrected"][c, m] and codec.encoding_id(m, c) < p for c in range(p)) for m in range(p)]
        res = run(data_fix, True)
    out = {"scheme": f.scheme, "ranks": p, "encoding": k, "chunk": f.chunk, "applied": bool(apply), "damaged": [],
           "stats": res["stats"]}
    for key in ("verify_mismatch_bytes", "corrected_bytes", "unlocated_columns", "remaining_mismatch_bytes",
                "damaged_stripes", "repair_units", "cells_written"):
        out[key] = int(res[key])
    for c in range(p):
        if not res["corrected"][c].any() and not res["unlocated"][c]:
            continue
        members = [{"member": m, "kind": "data" if codec.encoding_id(m, c) < p else "parity",
                    "corrected_bytes": int(res["corrected"][c, m]), "first_offset": int(res["first"][c, m])}
                   for m in range(p) if res["corrected"][c, m]]
        out["damaged"].append({"stripe": c, "members": members, "unlocated_columns": int(res["unlocated"][c])})
    out["repaired"] = out["remaining_mismatch_bytes"] == 0 and out["unlocated_columns"] == 0
    if stored is not None:
        now = _checksum_table(files, reds, hsize, f.chunk, k, slice_bytes)
        out["checksum_damaged"] = _checksum_diff(stored, now, reds)
        out["repaired"] = out["repaired"] and not out["checksum_damaged"]
    return out


def _gf_mul(a: int, b: int) -> int:
    """GF(2^8) / 0x11D product (the codec's field)."""
    r = 0
    while b:
        if b & 1:
            r ^= a
        b >>= 1
        a <<= 1
        if a & 0x100:
            a ^= 0x11D
    return r


def _cell_byte(files, red: str, header: int, chunk: int, kind_data: bool, index: int, off: int) -> int:
    """One byte of a member's cell: logical-file offset index*chunk + off over
    its data files (zeros past the last), or its redundancy file's slot."""
    if not kind_data:
        with open(red, "rb") as fh:
            fh.seek(header + index * chunk + off)
            return fh.read(1)[0]
    pos = index * chunk + off
    for path, size in files:
        if pos < size:
            with open(path, "rb") as fh:
                fh.seek(pos)
                return fh.read(1)[0]
        pos -= size
    return 0


def _cell_range(scheme: str, codec, p: int, member: int, stripe: int, chunk: int):
    """Member's cell of a stripe: ("data", first byte in its logical file) or
    ("parity", first byte in its redundancy payload)."""
    if scheme == "RS":
        enc = codec.encoding_id(member, stripe)
        if enc < p:
            return "data", codec.data_id(member, stripe) * chunk
        return "parity", (enc - p) * chunk
    if member == stripe:
        return "parity", 0
    return "data", (stripe if stripe < member else stripe - 1) * chunk


def verify_set(redundancy_files: Sequence[str], slice_bytes: int = 0, checksums: bool = False) -> Dict:
    """Scrub one set on disk: stream every member's data files and parity
    chunks through the check kernels (redset_amd.stream.*_verify_stream;
    nothing is written) and report whether the stored parity still matches
    the stored data. Driven by the headers as rebuild_set is; every member
    must be present (a lost member is rebuild_set's job, and a ValueError
    here). Returns the scheme, ``clean``, ``mismatch_bytes`` (summed over the
    parity rows) and ``damaged``: per damaged stripe its number, the first
    differing cell ``offset``, the located ``member`` (None for XOR sets or
    when no single member explains the column) and whether that member's
    wrong cell is ``"data"`` or ``"parity"``. Damage is repaired in place by
    repair_set (RS sets with 2 <= e <= 4: every byte column with one wrong
    byte), or by removing a located member's files and calling rebuild_set.
    ``checksums``: also recompute every member's CRC-32s (one crc32_stream
    pass) and compare them with the set's checksum sidecar (apply_set(
    checksums=True); none readable: ValueError). ``checksum_damaged`` lists
    what differs as {"member", "kind": "data" | "parity", "file"}; any entry
    makes ``clean`` false. A damaged stripe whose ``member`` the syndrome
    cannot name (XOR sets; columns no single member explains) takes it from
    there when exactly one member's differing file covers its cell of that
    stripe; where the syndrome did name one, ``member`` stays the syndrome's
    answer and the CRC's stands beside it."""
    f, reds, files, lost = _read_set(redundancy_files)
    p, k = f.ranks, f.encoding
    if lost:
        raise ValueError(f"members {lost} are lost: rebuild_set them before verifying")
    hsize = [f.header_size[r] for r in range(p)]
    codec = _codec(f.scheme, p, k)
    io = stream.FileIO(files, reds, hsize, f.chunk)
    try:
        if f.scheme == "RS":
            res = stream.rs_verify_stream(codec, f.chunk, io, slice_bytes=slice_bytes)
        else:
            res = stream.xor_verify_stream(p, f.chunk, io, slice_bytes=slice_bytes)
    finally:
        io.close()
    mism, first = res["mismatch"], res["first"]
    out = {"scheme": f.scheme, "ranks": p, "encoding": k, "chunk": f.chunk, "clean": bool(res["clean"]),
           "mismatch_bytes": int(mism.sum()), "damaged": [], "stats": res["stats"]}
    mat = codec.matrix() if codec is not None else None
    for c in range(p):
        if not mism[c].any():
            continue
        off = int(min(int(first[c, i]) for i in range(mism.shape[1]) if mism[c, i]))
        entry = {"stripe": c, "offset": off, "member": None, "kind": None}
        if codec is not None:
            syn = [0] * k
            for s in range(p):
                enc = codec.encoding_id(s, c)
                if enc < p:
                    b = _cell_byte(files[s], reds[s], hsize[s], f.chunk, True, codec.data_id(s, c), off)
                    for j in range(k):
                        syn[j] ^= _gf_mul(int(mat[p + j, s]), b)
                else:
                    syn[enc - p] ^= _cell_byte(files[s], reds[s], hsize[s], f.chunk, False, enc - p, off)
            m = codec.locate_syndrome(c, syn)
            if m >= 0:
                entry["member"] = m
                entry["kind"] = "data" if codec.encoding_id(m, c) < p else "parity"
        out["damaged"].append(entry)
    if checksums:
        stored = _read_sidecar(reds, p, f.chunk)
        now = _checksum_table(files, reds, hsize, f.chunk, k, slice_bytes)
        bad = _checksum_diff(stored, now, reds)
        out["checksum_damaged"] = bad
        out["clean"] = out["clean"] and not bad
        for entry in out["damaged"]:
            if entry["member"] is not None:
                continue
            hits = set()
            for d in bad:
                kind, lo = _cell_range(f.scheme, codec, p, d["member"], entry["stripe"], f.chunk)
                if kind != d["kind"]:
                    continue
                if kind == "data":  # the file's bytes in the logical file against the cell's
                    pos = 0
                    for path, size in files[d["member"]]:
                        if path == d["file"] and pos < lo + f.chunk and pos + size > lo:
                            hits.add((d["member"], kind))
                        pos += size
                else:
                    hits.add((d["member"], kind))
            if len(hits) == 1:
                (entry["member"], entry["kind"]), = hits
    return out
