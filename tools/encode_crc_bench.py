#!/usr/bin/env python
"""Time the fused encode + CRC-32 plan against the two plans it replaces.

One process, the RS(8+3) set of BASELINE configs[2]: 11 members, 64 MiB
cells, 121 cells, the padded layout bench.py uses (redset_hip_cell_stride).

Three plans over the same set take turns, 5 warm-up and 20 event-timed
executes each, `--repeats` times over: (a) the plain encode plan, (b) a CRC
plan of one range per cell, (c) the fused plan. Before timing, (c)'s parity
must equal (a)'s byte for byte and its 121 CRCs (b)'s; after timing the
ring-fault and hang-fault counts must be 0. GB/s = the algorithmic bytes,
(d + e) * chunk a stripe, over the median time; ratio = c / (a + b), the
medians of the same repeat.

    python tools/encode_crc_bench.py [--chunk-mib 64] [--out profiles/encode_crc_bench.json]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK_GBS = 8000.0  # MI355X HBM3E


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


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--chunk-mib", type=int, default=64)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "encode_crc_bench.json"))
    args = ap.parse_args()
    import numpy as np
    import torch

    import redset_amd

    assert torch.cuda.is_available(), "encode_crc_bench needs a GPU"
    p, e = 11, 3
    d = p - e
    chunk = args.chunk_mib << 20
    pad = redset_amd.cell_stride(chunk) - -(-chunk // 256) * 256
    lay = redset_amd.SetLayout.allocate(p, d, e, chunk, pad=pad)
    lay.storage.random_(0, 256)
    codec = redset_amd.RSCodec(p, e)
    ptrs = (lay.lofi_ptrs(), lay.parity_ptrs(), chunk, lay.cell_stride)
    # member r's cells in report order: data cells, then parity slots
    cells = [c for r in range(p) for c in [lay.data_cell(r, s) for s in range(d)] + [lay.parity_cell(r, i) for i in range(e)]]
    plans = {"encode": codec.plan_encode(*ptrs), "crc32": redset_amd.Crc32Plan([(c, chunk) for c in cells], keepalive=lay),
             "encode_crc32": codec.plan_encode_crc32(*ptrs)}
    parity = lambda: torch.cat([lay.parity_cell(r, i) for r in range(p) for i in range(e)])  # noqa: E731
    plans["encode"].execute()
    plans["crc32"].execute()
    torch.cuda.synchronize()
    want_parity, want_crcs = parity().clone(), np.array(plans["crc32"].report(), dtype=np.uint32)
    for r in range(p):
        for i in range(e):
            lay.parity_cell(r, i).zero_()
    plans["encode_crc32"].execute()
    torch.cuda.synchronize()
    assert torch.equal(parity(), want_parity), "the fused plan's parity differs from the encode plan's"
    assert np.array_equal(plans["encode_crc32"].report().reshape(-1), want_crcs), "the fused plan's CRCs differ from the CRC plan's"

    nbytes = p * (d + e) * chunk
    res = {"device": torch.cuda.get_device_name(0), "ranks": p, "encoding": e, "chunk_bytes": chunk,
           "cell_stride_bytes": lay.cell_stride, "cells": len(cells), "warmup": args.warmup, "steps": args.steps,
           "algorithmic_bytes": nbytes, "launches": {k: int(v.info.launches) if k != "crc32" else v.info()["launches"]
                                                     for k, v in plans.items()},
           "repeats": []}
    for _ in range(args.repeats):
        runs = time_plans(torch, plans, args.warmup, args.steps)
        rep = {k: {"median_ms": round(statistics.median(v), 4), "min_ms": round(v[0], 4), "max_ms": round(v[-1], 4)}
               for k, v in runs.items()}
        rep["ratio_c_over_a_plus_b"] = round(rep["encode_crc32"]["median_ms"] /
                                             (rep["encode"]["median_ms"] + rep["crc32"]["median_ms"]), 4)
        res["repeats"].append(rep)
        print(json.dumps(rep), flush=True)
    res["summary"] = {}
    for k in plans:
        meds = sorted(r[k]["median_ms"] for r in res["repeats"])
        med = statistics.median(meds)
        gbs = nbytes / (med * 1e-3) / 1e9
        res["summary"][k] = {"median_ms": round(med, 4), "medians_range_ms": [meds[0], meds[-1]],
                             "gb_per_s": round(gbs, 1), "fraction_of_8tbs": round(gbs / PEAK_GBS, 4)}
    ratios = sorted(r["ratio_c_over_a_plus_b"] for r in res["repeats"])
    res["summary"]["ratio_c_over_a_plus_b"] = {"median": round(statistics.median(ratios), 4), "range": [ratios[0], ratios[-1]]}
    res["ring_faults"], res["hang_faults"] = redset_amd.ring_faults(), redset_amd.hang_faults()
    assert (res["ring_faults"], res["hang_faults"]) == (0, 0), "a fault counter moved"
    print("summary:", json.dumps(res["summary"]), flush=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
