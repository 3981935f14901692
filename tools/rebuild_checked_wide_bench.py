#!/usr/bin/env python
"""Time the wide checked rebuild beside the unchanged plans of the same set.

One process, device-resident: RS(16+8), 64 MiB cells, the padded layout
bench.py uses (redset_hip_cell_stride). The set is encoded once, then five
plans take turns, 5 warm-up and 20 event-timed executes each:

  rebuild_k1 / rebuild_k2   the plain rebuild plan for 1 / 2 lost members:
                            the unchanged kernels, the yardstick
  checked_k1 / checked_k2   the wide checked rebuild plan for the same members
  repair_wide_dry           the unchanged gf_repair_wide_kernel<8> dry run

Rates are GB/s of bytes_read + bytes_written of each plan's own plan info.

Then one apply line: a 4 KiB run wrong in three survivors of one stripe,
rebuilt by checked_k1 (s = 7, three wrong bytes per column), 1 warm-up and 5
timed executes from the same damaged start.

    python tools/rebuild_checked_wide_bench.py [--chunk-mib 64] [--out profiles/rebuild_checked_wide_bench.json]
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rebuild_checked_wide_bench.json"))
    args = ap.parse_args()
    import torch

    import redset_amd

    assert torch.cuda.is_available(), "rebuild_checked_wide_bench needs a GPU"
    p, e, chunk = 24, 8, args.chunk_mib << 20
    d = p - e
    pad = redset_amd.cell_stride(chunk) - -(-chunk // 256) * 256
    lay = redset_amd.SetLayout.allocate(p, d, e, chunk, pad=pad)
    lay.storage.random_(0, 256)
    codec = redset_amd.RSCodec(p, e)
    args_ = (lay.lofi_ptrs(), lay.parity_ptrs(), chunk, lay.cell_stride)
    codec.plan_encode(*args_).execute()
    torch.cuda.synchronize()
    truth = {r: (lay.lofi(r).clone(), lay.parity(r).clone()) for r in (1, 2)}
    lost = {1: [1], 2: [1, 2]}
    plans = {}
    for k in (1, 2):
        plans[f"rebuild_k{k}"] = codec.plan_rebuild(lost[k], *args_)
        plans[f"checked_k{k}"] = codec.plan_rebuild_checked_wide(lost[k], *args_)
    plans["repair_wide_dry"] = codec.plan_repair_wide(*args_, apply=False)
    nbytes = {k: pl.bytes_read + pl.bytes_written for k, pl in plans.items()}

    def step(name, timed):
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
    # the last executes' reports and bytes: a clean set, rebuilt right
    for k in (1, 2):
        rep = plans[f"checked_k{k}"].report()
        assert not rep[0].any() and not rep[2].any()
    assert not plans["repair_wide_dry"].report()[0].any()
    for r, (lo, pa) in truth.items():
        assert torch.equal(lay.lofi(r), lo) and torch.equal(lay.parity(r), pa)
    res = {"device": torch.cuda.get_device_name(0), "warmup": args.warmup, "steps": args.steps, "scheme": "RS",
           "ranks": p, "encoding": e, "chunk_bytes": chunk, "cell_stride_bytes": lay.cell_stride}
    for k in plans:
        med = statistics.median(ms[k])
        gbs = nbytes[k] / (med * 1e-3) / 1e9
        res[k] = {"median_ms": round(med, 4), "min_ms": round(min(ms[k]), 4), "max_ms": round(max(ms[k]), 4),
                  "bytes_per_step": nbytes[k], "gb_per_s": round(gbs, 1), "fraction_of_8tbs": round(gbs / PEAK_GBS, 4),
                  "launches": plans[k].launches, "sorted_ms": [round(x, 4) for x in sorted(ms[k])]}
        print(f"{k}: {res[k]['median_ms']} ms ({res[k]['min_ms']}-{res[k]['max_ms']}), {res[k]['gb_per_s']} GB/s",
              flush=True)
    for k in (1, 2):
        res[f"checked_k{k}_rate_over_rebuild_k{k}_rate"] = round(
            res[f"checked_k{k}"]["gb_per_s"] / res[f"rebuild_k{k}"]["gb_per_s"], 4)
        res[f"checked_k{k}_rate_over_repair_wide_dry_rate"] = round(
            res[f"checked_k{k}"]["gb_per_s"] / res["repair_wide_dry"]["gb_per_s"], 4)

    # the slow case: 4 KiB of columns with three wrong survivors in stripe 3
    c, run, at = 3, 4096, 1 << 20
    surv = [m for m in range(p) if m != 1][:3]
    cells = [lay.data_cell(m, codec.data_id(m, c)) if codec.encoding_id(m, c) < p
             else lay.parity_cell(m, codec.encoding_id(m, c) - p) for m in surv]
    good = [x[at:at + run].clone() for x in cells]
    apply_ms = []
    pl = codec.plan_rebuild_checked_wide([1], *args_, fix_survivors=True)
    for it in range(6):
        for x in cells:
            x[at:at + run] ^= 0x5A
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        pl.execute()
        e1.record()
        e1.synchronize()
        if it:
            apply_ms.append(e0.elapsed_time(e1))
        rep = pl.report()
        assert int(rep[0].sum()) == 3 * run and not rep[2].any() and int(rep[4][c, 1]) == run
        assert all(torch.equal(x[at:at + run], g) for x, g in zip(cells, good))
    assert torch.equal(lay.lofi(1), truth[1][0]) and torch.equal(lay.parity(1), truth[1][1])
    res["apply_4k_run_3_wrong"] = {"median_ms": round(statistics.median(apply_ms), 4), "min_ms": round(min(apply_ms), 4),
                                   "max_ms": round(max(apply_ms), 4), "columns": run, "wrong_per_column": 3}
    print(f"apply_4k_run_3_wrong: {res['apply_4k_run_3_wrong']['median_ms']} ms", flush=True)
    res["ring_faults"] = redset_amd.ring_faults()
    res["hang_faults"] = redset_amd.hang_faults()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps({k: v for k, v in res.items() if k.endswith("_rate")}))


if __name__ == "__main__":
    main()
