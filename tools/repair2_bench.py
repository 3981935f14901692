#!/usr/bin/env python
"""Time the two-error repair kernel beside the single-error one on the same set.

One process, device-resident, the RS(16+4) set of BASELINE configs[4] at
64 MiB cells, the padded layout bench.py uses (redset_hip_cell_stride). The
set is encoded once, then three plans take turns, 5 warm-up and 20 event-timed
steps each:

  repair_dry    the unchanged gf_repair_kernel<4>, a dry run over all 20
                stripes of the clean set: the yardstick (p*(d+e)*C bytes)
  repair2_dry   gf_repair2_kernel, the same dry run on the same clean set
  repair2_pair  gf_repair2_kernel applying to ONE stripe with a 4 KiB run
                damaged in two members at the same offsets; the damage is put
                back before every step, outside the timed window ((d+e)*C bytes)

    python tools/repair2_bench.py [--chunk-mib 64] [--out profiles/repair2_bench.json]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK_GBS = 8000.0  # MI355X HBM3E


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--chunk-mib", type=int, default=64)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "repair2_bench.json"))
    args = ap.parse_args()
    import torch

    import redset_amd

    assert torch.cuda.is_available(), "repair2_bench needs a GPU"
    p, e, chunk = 20, 4, args.chunk_mib << 20
    d = p - e
    pad = redset_amd.cell_stride(chunk) - -(-chunk // 256) * 256
    lay = redset_amd.SetLayout.allocate(p, d, e, chunk, pad=pad)
    lay.storage.random_(0, 256)
    codec = redset_amd.RSCodec(p, e)
    args_ = (lay.lofi_ptrs(), lay.parity_ptrs(), chunk, lay.cell_stride)
    codec.plan_encode(*args_).execute()
    torch.cuda.synchronize()
    stripe = 7
    plans = {"repair_dry": codec.plan_repair(*args_, apply=False),
             "repair2_dry": codec.plan_repair(*args_, apply=False, max_errors=2),
             "repair2_pair": codec.plan_repair(*args_, stripes=[stripe], apply=True, max_errors=2)}
    nbytes = {"repair_dry": p * p * chunk, "repair2_dry": p * p * chunk, "repair2_pair": p * chunk}
    # the damage: the same 4 KiB of columns in the data cells members 0 and 1 hold in that stripe
    lo = chunk // 2 + 5
    cells = []
    for m, x in ((0, 0x5A), (1, 0xC3)):
        assert codec.encoding_id(m, stripe) < p
        cell = lay.data_cell(m, codec.data_id(m, stripe))
        good = cell[lo:lo + 4096].clone()
        cells.append((cell, good, good ^ x))

    def step(name, timed):
        if name == "repair2_pair":
            for cell, _, bad in cells:
                cell[lo:lo + 4096].copy_(bad)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        plans[name].execute()
        e1.record()
        e1.synchronize()
        if timed is not None:
            timed[name].append(e0.elapsed_time(e1))

    for _ in range(args.warmup):
        for name in plans:
            step(name, None)
    ms = {k: [] for k in plans}
    for _ in range(args.steps):
        for name in plans:
            step(name, ms)
    torch.cuda.synchronize()
    # the last steps' reports: a clean set, and the run corrected as pairs
    for name in ("repair_dry", "repair2_dry"):
        rep = plans[name].report()
        assert not rep[0].any() and not rep[2].any(), name
    one = plans["repair2_pair"].report()
    assert int(one[0][0, 0]) == 4096 and int(one[0][0, 1]) == 4096 and int(one[4][0]) == 4096 and not one[2].any()
    for cell, good, _ in cells:
        assert torch.equal(cell[lo:lo + 4096], good)
    res = {"device": torch.cuda.get_device_name(0), "warmup": args.warmup, "steps": args.steps, "scheme": "RS",
           "ranks": p, "encoding": e, "chunk_bytes": chunk, "cell_stride_bytes": lay.cell_stride,
           "ring_faults": redset_amd.ring_faults(), "hang_faults": redset_amd.hang_faults()}
    for k in plans:
        med = statistics.median(ms[k])
        gbs = nbytes[k] / (med * 1e-3) / 1e9
        res[k] = {"median_ms": round(med, 4), "min_ms": round(min(ms[k]), 4), "max_ms": round(max(ms[k]), 4),
                  "bytes_per_step": nbytes[k], "gb_per_s": round(gbs, 1), "fraction_of_8tbs": round(gbs / PEAK_GBS, 4),
                  "launches": plans[k].launches, "sorted_ms": [round(x, 4) for x in sorted(ms[k])]}
        print(f"{k}: {res[k]['median_ms']} ms ({res[k]['min_ms']}-{res[k]['max_ms']}), {res[k]['gb_per_s']} GB/s",
              flush=True)
    res["repair2_dry_rate_over_repair_dry_rate"] = round(res["repair2_dry"]["gb_per_s"] / res["repair_dry"]["gb_per_s"], 4)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps({"repair2_dry_rate_over_repair_dry_rate": res["repair2_dry_rate_over_repair_dry_rate"]}))


if __name__ == "__main__":
    main()
