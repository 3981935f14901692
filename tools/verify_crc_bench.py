#!/usr/bin/env python
"""Time the fused verify + CRC-32 plan against the two plans it replaces.

One process, the RS(8+3) set of BASELINE configs[2]: 11 members, 64 MiB
cells, 121 cells, the padded layout bench.py uses (redset_hip_cell_stride).

Three plans over the same encoded set take turns, 5 warm-up and 20 event-timed
executes each, `--repeats` times over: (a) the verify plan, (b) a CRC plan of
one range per cell, (c) the fused plan. Before timing, on the clean set and
again with bytes of three cells flipped, (c)'s report rows must equal (a)'s
and its 121 CRCs (b)'s; the set is clean while timed. After timing the
ring-fault and hang-fault counts must be 0. GB/s = the algorithmic bytes,
(d + e) * chunk a stripe, over the median time; ratio = c / (a + b), the
medians of the same repeat.

    python tools/verify_crc_bench.py [--chunk-mib 64] [--out profiles/verify_crc_bench.json]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from encode_crc_bench import PEAK_GBS, time_plans  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--chunk-mib", type=int, default=64)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "verify_crc_bench.json"))
    args = ap.parse_args()
    import numpy as np
    import torch

    import redset_amd

    assert torch.cuda.is_available(), "verify_crc_bench needs a GPU"
    p, e = 11, 3
    d = p - e
    chunk = args.chunk_mib << 20
    pad = redset_amd.cell_stride(chunk) - -(-chunk // 256) * 256
    lay = redset_amd.SetLayout.allocate(p, d, e, chunk, pad=pad)
    lay.storage.random_(0, 256)
    codec = redset_amd.RSCodec(p, e)
    ptrs = (lay.lofi_ptrs(), lay.parity_ptrs(), chunk, lay.cell_stride)
    codec.plan_encode(*ptrs).execute()
    # member r's cells in report order: data cells, then parity slots
    cells = [c for r in range(p) for c in [lay.data_cell(r, s) for s in range(d)] + [lay.parity_cell(r, i) for i in range(e)]]
    plans = {"verify": codec.plan_verify(*ptrs), "crc32": redset_amd.Crc32Plan([(c, chunk) for c in cells], keepalive=lay),
             "verify_crc32": codec.plan_verify_crc32(*ptrs)}

    def agree(what, clean):
        for plan in plans.values():
            plan.execute()
        torch.cuda.synchronize()
        rows, fused = plans["verify"].report(), plans["verify_crc32"].report()
        assert all(np.array_equal(a, b) for a, b in zip(rows, fused)), f"{what}: the fused plan's rows differ from the verify plan's"
        assert np.array_equal(plans["verify_crc32"].crcs().reshape(-1), np.array(plans["crc32"].report(), dtype=np.uint32)), \
            f"{what}: the fused plan's CRCs differ from the CRC plan's"
        assert plans["verify_crc32"].clean == clean, what
        return int(rows[0].sum())

    agree("clean set", True)
    hits = [(lay.data_cell(0, 0), 0), (lay.data_cell(3, 5), chunk // 2 + 5), (lay.parity_cell(7, 1), chunk - 1)]
    for cell, off in hits:
        cell[off] ^= 0x5A
    differing = agree("damaged set", False)
    for cell, off in hits:
        cell[off] ^= 0x5A
    agree("set restored", True)

    nbytes = p * (d + e) * chunk
    res = {"device": torch.cuda.get_device_name(0), "ranks": p, "encoding": e, "chunk_bytes": chunk,
           "cell_stride_bytes": lay.cell_stride, "cells": len(cells), "warmup": args.warmup, "steps": args.steps,
           "algorithmic_bytes": nbytes, "differing_bytes_in_the_damaged_check": differing,
           "launches": {k: int(v.info.launches) if k != "crc32" else v.info()["launches"] for k, v in plans.items()},
           "repeats": []}
    for _ in range(args.repeats):
        runs = time_plans(torch, plans, args.warmup, args.steps)
        rep = {k: {"median_ms": round(statistics.median(v), 4), "min_ms": round(v[0], 4), "max_ms": round(v[-1], 4)}
               for k, v in runs.items()}
        rep["ratio_c_over_a_plus_b"] = round(rep["verify_crc32"]["median_ms"] /
                                             (rep["verify"]["median_ms"] + rep["crc32"]["median_ms"]), 4)
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
    res["summary"]["ratio_c_over_a_plus_b"] = {"median": round(statistics.median(ratios), 4), "range": [ratios[0], ratios[-1]],
                                               "below_1_in_every_repeat": ratios[-1] < 1.0}
    agree("after timing", True)
    res["ring_faults"], res["hang_faults"] = redset_amd.ring_faults(), redset_amd.hang_faults()
    assert (res["ring_faults"], res["hang_faults"]) == (0, 0), "a fault counter moved"
    print("summary:", json.dumps(res["summary"]), flush=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
