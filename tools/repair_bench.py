#!/usr/bin/env python
"""Time the repair plans beside the verify plan of the same set.

One process, device-resident, BASELINE configs[2]: RS(8+3), 64 MiB cells, the
padded layout bench.py uses (redset_hip_cell_stride). The set is encoded once,
then three plans take turns, 5 warm-up and 20 event-timed steps each, and
their medians are reported:

  verify        the verify plan: the unchanged check kernels, the yardstick
  repair_dry    a dry-run repair plan over all 11 stripes of the clean set
                (what a repair costs where nothing is wrong: the ring-less
                read kernel at full width; both read p*(d+e)*C bytes)
  repair_one    an applying repair plan over ONE stripe with one 4 KiB run
                damaged in one cell; the damage is put back before every
                step, outside the timed window ((d+e)*C bytes read)

    python tools/repair_bench.py [--chunk-mib 64] [--out profiles/repair_bench.json]
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "repair_bench.json"))
    args = ap.parse_args()
    import torch

    import redset_amd

    assert torch.cuda.is_available(), "repair_bench needs a GPU"
    p, e, chunk = 11, 3, args.chunk_mib << 20
    d = p - e
    pad = redset_amd.cell_stride(chunk) - -(-chunk // 256) * 256
    lay = redset_amd.SetLayout.allocate(p, d, e, chunk, pad=pad)
    lay.storage.random_(0, 256)
    codec = redset_amd.RSCodec(p, e)
    args_ = (lay.lofi_ptrs(), lay.parity_ptrs(), chunk, lay.cell_stride)
    codec.plan_encode(*args_).execute()
    torch.cuda.synchronize()
    stripe = 5
    plans = {"verify": codec.plan_verify(*args_), "repair_dry": codec.plan_repair(*args_, apply=False),
             "repair_one": codec.plan_repair(*args_, stripes=[stripe], apply=True)}
    nbytes = {"verify": p * p * chunk, "repair_dry": p * p * chunk, "repair_one": p * chunk}
    # the damage: a 4 KiB run in the data cell member 0 holds in that stripe
    assert codec.encoding_id(0, stripe) < p
    cell = lay.data_cell(0, codec.data_id(0, stripe))
    lo = chunk // 2 + 5
    good = cell[lo:lo + 4096].clone()
    bad = good ^ 0x5A

    def step(name, timed):
        if name == "repair_one":
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
    # the last steps' reports: a clean set, and the run corrected
    assert plans["verify"].clean
    dry = plans["repair_dry"].report()
    assert not dry[0].any() and not dry[2].any()
    one = plans["repair_one"].report()
    assert int(one[0].sum()) == 4096 and int(one[0][0, 0]) == 4096 and not one[2].any()
    assert torch.equal(cell[lo:lo + 4096], good)
    res = {"device": torch.cuda.get_device_name(0), "warmup": args.warmup, "steps": args.steps, "scheme": "RS",
           "ranks": p, "encoding": e, "chunk_bytes": chunk, "cell_stride_bytes": lay.cell_stride,
           "ring_faults": redset_amd.ring_faults(), "hang_faults": redset_amd.hang_faults()}
    for k in plans:
        med = statistics.median(ms[k])
        gbs = nbytes[k] / (med * 1e-3) / 1e9
        res[k] = {"median_ms": round(med, 4), "bytes_per_step": nbytes[k], "gb_per_s": round(gbs, 1),
                  "fraction_of_8tbs": round(gbs / PEAK_GBS, 4), "launches": plans[k].launches,
                  "sorted_ms": [round(x, 4) for x in sorted(ms[k])]}
        print(f"{k}: {res[k]['median_ms']} ms, {res[k]['gb_per_s']} GB/s", flush=True)
    res["repair_dry_rate_over_verify_rate"] = round(res["repair_dry"]["gb_per_s"] / res["verify"]["gb_per_s"], 4)
    res["repair_one_rate_over_verify_rate"] = round(res["repair_one"]["gb_per_s"] / res["verify"]["gb_per_s"], 4)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps({k: res[k] for k in ("repair_dry_rate_over_verify_rate", "repair_one_rate_over_verify_rate")}))


if __name__ == "__main__":
    main()
