#!/usr/bin/env python
"""Time the wide repair kernel beside this tree's verify plan and gf_repair_kernel<4>.

One process, device-resident, an RS(16+8) set at 64 MiB cells in the padded
layout bench.py uses (redset_hip_cell_stride), and an RS(16+4) set of the same
cells for the e = 4 yardstick. Both are encoded once, then four plans take
turns, 5 warm-up and 20 event-timed steps each:

  verify        the unchanged verify plan over the clean RS(16+8) set
  wide_dry      gf_repair_wide_kernel<8>, a dry run over all 24 stripes of
                the clean set (p*(d+e)*C bytes)
  wide_run      gf_repair_wide_kernel<8> applying to ONE stripe with a 4 KiB
                run damaged in t = 4 members at the same offsets; the damage
                is put back before every step, outside the timed window
                ((d+e)*C bytes)
  repair4_dry   the unchanged gf_repair_kernel<4>, a dry run over the clean
                RS(16+4) set

    python tools/repair_wide_bench.py [--chunk-mib 64] [--out profiles/repair_wide_bench.json]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK_GBS = 8000.0  # MI355X HBM3E


def make_set(redset_amd, torch, p, e, chunk):
    pad = redset_amd.cell_stride(chunk) - -(-chunk // 256) * 256
    lay = redset_amd.SetLayout.allocate(p, p - e, e, chunk, pad=pad)
    lay.storage.random_(0, 256)
    codec = redset_amd.RSCodec(p, e)
    args = (lay.lofi_ptrs(), lay.parity_ptrs(), chunk, lay.cell_stride)
    codec.plan_encode(*args).execute()
    torch.cuda.synchronize()
    return lay, codec, args


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--chunk-mib", type=int, default=64)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "repair_wide_bench.json"))
    args = ap.parse_args()
    import torch

    import redset_amd

    assert torch.cuda.is_available(), "repair_wide_bench needs a GPU"
    chunk = args.chunk_mib << 20
    p, e = 24, 8
    t = e // 2
    lay, codec, set8 = make_set(redset_amd, torch, p, e, chunk)
    _, codec4, set4 = make_set(redset_amd, torch, 20, 4, chunk)
    stripe = 9
    plans = {"verify": codec.plan_verify(*set8),
             "wide_dry": codec.plan_repair_wide(*set8, apply=False),
             "wide_run": codec.plan_repair_wide(*set8, stripes=[stripe], apply=True),
             "repair4_dry": codec4.plan_repair(*set4, apply=False)}
    nbytes = {"verify": p * p * chunk, "wide_dry": p * p * chunk, "wide_run": p * chunk, "repair4_dry": 20 * 20 * chunk}
    # the damage: the same 4 KiB of columns in the first t data cells of that stripe
    lo = chunk // 2 + 5
    members = [m for m in range(p) if codec.encoding_id(m, stripe) < p][:t]
    cells = []
    for m, x in zip(members, (0x5A, 0xC3, 0x17, 0xE1)):
        cell = lay.data_cell(m, codec.data_id(m, stripe))
        good = cell[lo:lo + 4096].clone()
        cells.append((cell, good, good ^ x))

    def step(name, timed):
        if name == "wide_run":
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
    # the last steps' reports: clean sets, and the run corrected t bytes a column
    assert plans["verify"].clean
    for name in ("wide_dry", "repair4_dry"):
        rep = plans[name].report()
        assert not rep[0].any() and not rep[2].any(), name
    one = plans["wide_run"].report()
    assert all(int(one[0][0, m]) == 4096 for m in members) and int(one[4][0, t - 2]) == 4096 and not one[2].any()
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
    res["wide_dry_rate_over_verify_rate"] = round(res["wide_dry"]["gb_per_s"] / res["verify"]["gb_per_s"], 4)
    res["wide_dry_rate_over_repair4_dry_rate"] = round(res["wide_dry"]["gb_per_s"] / res["repair4_dry"]["gb_per_s"], 4)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps({k: res[k] for k in ("wide_dry_rate_over_verify_rate", "wide_dry_rate_over_repair4_dry_rate",
                                          "ring_faults", "hang_faults")}))


if __name__ == "__main__":
    main()
