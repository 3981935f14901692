#!/usr/bin/env python
"""Time the checked rebuild beside the unchanged plans of the same set.

One process, device-resident, BASELINE configs[2]: RS(8+3), 64 MiB cells, the
padded layout bench.py uses (redset_hip_cell_stride). The set is encoded once,
then six plans take turns, 5 warm-up and 20 event-timed executes each:

  rebuild_k1 / rebuild_k2   the plain rebuild plan for 1 / 2 lost members:
                            the unchanged kernels, the yardstick
  checked_k1 / checked_k2   the checked rebuild plan for the same lost members
  verify                    the verify plan (reads p*(d+e)*C bytes)
  repair_dry                a dry-run repair plan over all stripes

Rates are GB/s of bytes_read + bytes_written of each plan's own plan info.

Then the host-resident form on the same set in page-locked host memory:
rs_rebuild_stream and rs_rebuild_checked_stream for one lost member, 1 warm-up
and 5 timed calls each, taking turns (wall time of the call).

    python tools/rebuild_checked_bench.py [--chunk-mib 64] [--out profiles/rebuild_checked_bench.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK_GBS = 8000.0  # MI355X HBM3E


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--chunk-mib", type=int, default=64)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--stream-steps", type=int, default=5, help="0 skips the host-resident part")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rebuild_checked_bench.json"))
    args = ap.parse_args()
    import torch

    import redset_amd

    assert torch.cuda.is_available(), "rebuild_checked_bench needs a GPU"
    p, e, chunk = 11, 3, args.chunk_mib << 20
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
        plans[f"checked_k{k}"] = codec.plan_rebuild_checked(lost[k], *args_)
    plans["verify"] = codec.plan_verify(*args_)
    plans["repair_dry"] = codec.plan_repair(*args_, apply=False)
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
    assert plans["verify"].clean
    for k in (1, 2):
        rep = plans[f"checked_k{k}"].report()
        assert not rep[0].any() and not rep[2].any()
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
        res[f"checked_k{k}_rate_over_verify_rate"] = round(res[f"checked_k{k}"]["gb_per_s"] / res["verify"]["gb_per_s"], 4)
    res["repair_dry_rate_over_verify_rate"] = round(res["repair_dry"]["gb_per_s"] / res["verify"]["gb_per_s"], 4)

    if args.stream_steps > 0:
        # the same set in page-locked host memory, the device set's layout
        host = torch.empty(lay.storage.numel(), dtype=torch.uint8, pin_memory=True)
        host.copy_(lay.storage)
        torch.cuda.synchronize()
        base, per = host.data_ptr(), lay.member_bytes
        lofi = [base + r * per for r in range(p)]
        parity = [x + d * lay.cell_stride for x in lofi]
        io = redset_amd.stream.HostIO(p, lofi, parity, lay.cell_stride, keepalive=(host,), pinned=True)
        calls = {"rebuild_stream": lambda: redset_amd.stream.rs_rebuild_stream(codec, [1], chunk, io),
                 "checked_stream": lambda: redset_amd.rs_rebuild_checked_stream(codec, [1], chunk, io)}
        secs = {k: [] for k in calls}
        last = {}
        for it in range(1 + args.stream_steps):
            for name, fn in calls.items():
                t0 = time.perf_counter()
                last[name] = fn()
                if it > 0:
                    secs[name].append(time.perf_counter() - t0)
        io.close()
        assert last["checked_stream"]["corrected_bytes"] == 0 and last["checked_stream"]["unlocated_columns"] == 0
        assert torch.equal(host.cuda(), lay.storage)
        for name in calls:
            stt = last[name].get("stats", last[name])
            moved = int(stt["bytes_read"]) + int(stt["bytes_written"])
            med = statistics.median(secs[name])
            res[name] = {"median_s": round(med, 4), "min_s": round(min(secs[name]), 4), "max_s": round(max(secs[name]), 4),
                         "bytes_per_call": moved, "gb_per_s": round(moved / med / 1e9, 2),
                         "read_s": round(stt["read_seconds"], 4), "gpu_s": round(stt["gpu_seconds"], 4),
                         "write_s": round(stt["write_seconds"], 4)}
            print(f"{name}: {res[name]['median_s']} s ({res[name]['min_s']}-{res[name]['max_s']}), "
                  f"{res[name]['gb_per_s']} GB/s", flush=True)
        res["checked_stream_rate_over_rebuild_stream_rate"] = round(
            res["checked_stream"]["gb_per_s"] / res["rebuild_stream"]["gb_per_s"], 4)
    res["ring_faults"] = redset_amd.ring_faults()
    res["hang_faults"] = redset_amd.hang_faults()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps({k: v for k, v in res.items() if k.endswith("_rate")}))


if __name__ == "__main__":
    main()
