#!/usr/bin/env python
"""Time the verify (scrub) plans beside the encode plans of the same set.

One process, the padded layout bench.py uses (redset_hip_cell_stride), 64 MiB
cells: RS(8+3), XOR p = 8 and, for the record, RS(16+4). Per set: encode once
(so the stored parity is right and verify runs its fast path), then 5 warm-up
and 20 event-timed steps of each plan, alternating, and their medians. Both
plans move (d+e)*C bytes per stripe -- the encode reads d*C and writes e*C,
the verify reads all of it -- so the encode, unchanged code, is the yardstick:
GB/s = p*(d+e)*C / median, and the verify / encode time ratio.

    python tools/verify_bench.py [--chunk-mib 64] [--out profiles/verify_bench.json]
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
    """median ms of every plan, the plans taking turns step by step"""
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
    return {k: statistics.median(v) for k, v in ms.items()}, {k: [round(x, 4) for x in sorted(v)] for k, v in ms.items()}


def one(torch, redset_amd, scheme, p, e, chunk, warmup, steps):
    d = p - e
    pad = redset_amd.cell_stride(chunk) - -(-chunk // 256) * 256
    lay = redset_amd.SetLayout.allocate(p, d, e, chunk, pad=pad)
    lay.storage.random_(0, 256)
    if scheme == "RS":
        codec = redset_amd.RSCodec(p, e)
        enc = codec.plan_encode(lay.lofi_ptrs(), lay.parity_ptrs(), chunk, lay.cell_stride)
        ver = codec.plan_verify(lay.lofi_ptrs(), lay.parity_ptrs(), chunk, lay.cell_stride)
    else:
        enc = redset_amd.xor_plan_encode(p, lay.lofi_ptrs(), lay.parity_ptrs(), chunk, lay.cell_stride)
        ver = redset_amd.xor_plan_verify(p, lay.lofi_ptrs(), lay.parity_ptrs(), chunk, lay.cell_stride)
    enc.execute()
    torch.cuda.synchronize()
    med, runs = time_plans(torch, {"encode": enc, "verify": ver}, warmup, steps)
    assert ver.clean, "the set it just encoded does not verify"
    nbytes = p * (d + e) * chunk
    out = {"scheme": scheme, "ranks": p, "encoding": e, "chunk_bytes": chunk, "cell_stride_bytes": lay.cell_stride,
           "bytes_per_step": nbytes, "verify_launches": ver.launches, "encode_launches": enc.launches,
           "verify_over_encode": round(med["verify"] / med["encode"], 4), "ring_faults": redset_amd.ring_faults(),
           "hang_faults": redset_amd.hang_faults()}
    for k in ("encode", "verify"):
        gbs = nbytes / (med[k] * 1e-3) / 1e9
        out[k] = {"median_ms": round(med[k], 4), "gb_per_s": round(gbs, 1), "fraction_of_8tbs": round(gbs / PEAK_GBS, 4),
                  "sorted_ms": runs[k]}
    del enc, ver, lay
    torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--chunk-mib", type=int, default=64)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "verify_bench.json"))
    args = ap.parse_args()
    import torch

    import redset_amd

    chunk = args.chunk_mib << 20
    res = {"device": torch.cuda.get_device_name(0), "warmup": args.warmup, "steps": args.steps, "configs": {}}
    for name, scheme, p, e in (("rs_8p3", "RS", 11, 3), ("xor_p8", "XOR", 8, 1), ("rs_16p4", "RS", 20, 4)):
        res["configs"][name] = one(torch, redset_amd, scheme, p, e, chunk, args.warmup, args.steps)
        c = res["configs"][name]
        print(f"{name}: encode {c['encode']['median_ms']} ms ({c['encode']['gb_per_s']} GB/s), "
              f"verify {c['verify']['median_ms']} ms ({c['verify']['gb_per_s']} GB/s), "
              f"verify/encode {c['verify_over_encode']}", flush=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps({k: v["verify_over_encode"] for k, v in res["configs"].items()}))


if __name__ == "__main__":
    main()
