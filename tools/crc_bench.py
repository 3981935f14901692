#!/usr/bin/env python
"""Time the CRC-32 plan and the streamed CRC pass beside set verification.

One process, the RS(8+3) set of BASELINE configs[2]: 11 members, 64 MiB
cells, 121 cells, the padded layout bench.py uses (redset_hip_cell_stride).

Device-resident: a CRC plan of one range per cell and the RS verify plan over
the same encoded set take turns, 5 warm-up and 20 event-timed executes each;
GB/s = the plan's bytes_read / median time, and its fraction of the 8 TB/s
HBM roofline. zlib.crc32 on one host thread over 256 MiB gives the CPU's rate.

Streamed: the set copied to page-locked host memory in the same layout;
crc32_stream (one span per member's logical file and one per payload: every
cell once) and rs_verify_stream take turns, 1 warm-up and 5 timed calls each,
GB/s = bytes_read / wall time of the call.

    python tools/crc_bench.py [--chunk-mib 64] [--out profiles/crc_bench.json]
"""
import argparse
import json
import os
import statistics
import sys
import time
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK_GBS = 8000.0      # MI355X HBM3E
HOST_LINK_GBS = 69.2   # zero-copy host reads, DESIGN.md section 5.3


def time_plans(torch, plans, warmup, steps):
    """sorted ms of every plan, the plans taking turns step by step"""
    for _ in range(warmup):
        for p in plans.values():
            p.execute()
    torch.cuda.synchronize()
    ms = {k: [] for k in plans}
    for _ in range(steps):
        for k, p in plans.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            p.execute()
            e1.record()
            e1.synchronize()
            ms[k].append(e0.elapsed_time(e1))
    return {k: sorted(v) for k, v in ms.items()}


def rate(nbytes, ms):
    return nbytes / (ms * 1e-3) / 1e9


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--chunk-mib", type=int, default=64)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "crc_bench.json"))
    args = ap.parse_args()
    import torch

    import redset_amd
    from redset_amd import stream

    assert torch.cuda.is_available(), "crc_bench needs a GPU"
    p, e = 11, 3
    d = p - e
    chunk = args.chunk_mib << 20
    pad = redset_amd.cell_stride(chunk) - -(-chunk // 256) * 256
    lay = redset_amd.SetLayout.allocate(p, d, e, chunk, pad=pad)
    lay.storage.random_(0, 256)
    codec = redset_amd.RSCodec(p, e)
    codec.plan_encode(lay.lofi_ptrs(), lay.parity_ptrs(), chunk, lay.cell_stride).execute()
    torch.cuda.synchronize()
    cells = [lay.data_cell(r, s) for r in range(p) for s in range(d)] + \
            [lay.parity_cell(r, i) for r in range(p) for i in range(e)]
    crc = redset_amd.Crc32Plan([(c, chunk) for c in cells], keepalive=lay)
    ver = codec.plan_verify(lay.lofi_ptrs(), lay.parity_ptrs(), chunk, lay.cell_stride)
    runs = time_plans(torch, {"crc32": crc, "rs_verify": ver}, args.warmup, args.steps)
    assert ver.clean, "the set it just encoded does not verify"
    # the kernels against zlib on one cell, and zlib's own rate
    one = cells[0][:min(chunk, 256 << 20)].cpu().numpy().tobytes()
    t0 = time.perf_counter()
    want = zlib.crc32(one)
    zlib_s = time.perf_counter() - t0
    got = redset_amd.Crc32Plan([(cells[0], len(one))], keepalive=lay)
    got.execute()
    assert got.report()[0] == want, "the CRC kernels disagree with zlib"
    res = {"device": torch.cuda.get_device_name(0), "ranks": p, "encoding": e, "chunk_bytes": chunk,
           "cell_stride_bytes": lay.cell_stride, "cells": len(cells), "warmup": args.warmup, "steps": args.steps,
           "device_resident": {}, "streamed": {}}
    for k, plan_bytes in (("crc32", crc.info()["bytes_read"]), ("rs_verify", ver.bytes_read)):
        med = statistics.median(runs[k])
        gbs = rate(plan_bytes, med)
        res["device_resident"][k] = {"bytes_read": plan_bytes, "median_ms": round(med, 4), "gb_per_s": round(gbs, 1),
                                     "fraction_of_8tbs": round(gbs / PEAK_GBS, 4),
                                     "sorted_ms": [round(x, 4) for x in runs[k]]}
    res["device_resident"]["crc32"]["launches"] = crc.info()["launches"]
    res["device_resident"]["zlib_one_thread"] = {"bytes": len(one), "gb_per_s": round(len(one) / zlib_s / 1e9, 3)}
    res["device_resident"]["crc32_over_host_link"] = round(res["device_resident"]["crc32"]["gb_per_s"] / HOST_LINK_GBS, 2)
    print("device-resident:", json.dumps({k: v.get("gb_per_s") if isinstance(v, dict) else v
                                          for k, v in res["device_resident"].items()}), flush=True)

    # the same set in page-locked host memory, same layout
    host = torch.empty(lay.storage.numel(), dtype=torch.uint8, pin_memory=True)
    host.copy_(lay.storage)
    torch.cuda.synchronize()
    del crc, ver, got, cells
    base, member = host.data_ptr(), lay.member_bytes
    io = stream.HostIO(p, [base + r * member for r in range(p)],
                       [base + r * member + d * lay.cell_stride for r in range(p)], lay.cell_stride,
                       keepalive=host, pinned=True)
    spans = [(r, 0, 0, d * chunk) for r in range(p)] + [(r, 1, 0, e * chunk) for r in range(p)]
    calls = {"crc32_stream": lambda: stream.crc32_stream(chunk, io, spans),
             "rs_verify_stream": lambda: stream.rs_verify_stream(codec, chunk, io)}
    first = {k: f() for k, f in calls.items()}  # warm-up; also the answers
    assert first["rs_verify_stream"]["clean"]
    got = first["crc32_stream"]["crcs"]
    cell_crcs = redset_amd.Crc32Plan([(lay.data_cell(0, s), chunk) for s in range(d)], keepalive=lay)
    cell_crcs.execute()
    joined = 0
    for c in cell_crcs.report():
        joined = redset_amd.crc32_combine(joined, c, chunk)
    assert got[0] == joined, "the streamed CRC of member 0 differs from its cells' CRCs joined"
    del cell_crcs
    times = {k: [] for k in calls}
    stats = {}
    for _ in range(args.repeats):
        for k, f in calls.items():
            stats[k] = f()["stats"]
            times[k].append(stats[k]["seconds"])
    for k in calls:
        nbytes = stats[k]["bytes_read"]
        rates = sorted(nbytes / t / 1e9 for t in times[k])
        res["streamed"][k] = {"bytes_read": nbytes, "seconds": [round(t, 5) for t in times[k]],
                              "gb_per_s_sorted": [round(x, 2) for x in rates],
                              "gb_per_s_median": round(statistics.median(rates), 2),
                              "gpu_seconds_last": round(stats[k]["gpu_seconds"], 5)}
    lo, hi = res["streamed"]["rs_verify_stream"]["gb_per_s_sorted"][0], res["streamed"]["rs_verify_stream"]["gb_per_s_sorted"][-1]
    med = res["streamed"]["crc32_stream"]["gb_per_s_median"]
    res["streamed"]["crc_within_verify_spread"] = bool(lo <= med <= hi)
    res["streamed"]["crc_median_over_verify_median"] = round(med / res["streamed"]["rs_verify_stream"]["gb_per_s_median"], 3)
    res["ring_faults"], res["hang_faults"] = redset_amd.ring_faults(), redset_amd.hang_faults()
    io.close()
    print("streamed:", json.dumps({k: (v["gb_per_s_sorted"] if isinstance(v, dict) else v)
                                   for k, v in res["streamed"].items()}), flush=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
