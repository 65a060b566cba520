"""Times the value layer's parameter gradients on bf16-stored rows (ops.value_proj_backward on bf16 operands:
dsmil_value_backward_bf16, k_value_tn_b16) and, on the same device in the same run, the route a user had before it: widen the
bf16 rows and the bf16 V with .float() and call dsmil_value_backward (k_value_tn) on the copies.
  10 000 x 512 x 512 (one bag) and 640 000 x 512 x 512 (the 64-bag batch, one call over the concatenated rows):
      ops.value_proj_backward(x_bf16, V_bf16, g)   vs   ops.value_proj_backward(x_bf16.float(), V_bf16.float(), g)
  plus the fp32 kernel alone on operands widened once outside the window (what the widening itself costs), the GB/s the
  native time implies (x and V read once at 2 bytes, g_vals at 4) and its share of the bf16 MFMA peak (three plane products).
Device-event times; every shape is warmed up first; a timed window repeats its call until it is >= --window seconds long; the
sides alternate inside this one process, --repeats windows each (>= 5), so that the spread (max - min of a side's windows) is
known.  Asserts no time.  Writes every median and spread to profiles/value_bwd_b16/times.json (--out) and prints the JSON.

    python tools/value_bwd_b16_time.py [--repeats 5] [--window 0.3] [--only-kernels]
`--only-kernels`: run the two routes a few times and exit (for a `rocprofv3 --kernel-trace --stats` run of its own)."""
import argparse
import json
import os
import statistics

import _path  # noqa: F401
import torch

import dsmil  # noqa: F401  (registers the dsmil_wsi_amd package)
from dsmil_wsi_amd import ops
from dsmil_wsi_amd.synthetic import make_bag
from value_proj_time import window

PEAK_BF16_DENSE = 2.5e15   # MI355X bf16 MFMA, FLOP/s
COPY_CEILING = 6.29e12     # MI355X achievable HBM copy rate, bytes/s (a float4 copy kernel; 8.0e12 is the data sheet's)


def abc(sides, repeats, min_s):
    """sides: {name: fn}.  Warm-up, then `repeats` rounds of one window per side in turn."""
    for fn in sides.values():   # warm-up: code objects, workspaces, the allocator's blocks for the widened copies
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    t = {k: [] for k in sides}
    for _ in range(repeats):
        for k, fn in sides.items():
            t[k].append(window(fn, min_s))
    return {k: {"median_us": statistics.median(v) * 1e6, "spread_us": (max(v) - min(v)) * 1e6,
                "windows_us": [round(u * 1e6, 2) for u in v]} for k, v in t.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.3)
    ap.add_argument("--only-kernels", action="store_true", help="run the two routes a few times and exit (for a kernel trace)")
    ap.add_argument("--out", default=os.path.join(_path.ROOT, "profiles", "value_bwd_b16", "times.json"))
    args = ap.parse_args()
    if args.repeats < 5:
        ap.error("--repeats must be at least 5")
    K, N = 512, 10000
    torch.manual_seed(0)
    v_w = torch.nn.init.orthogonal_(torch.empty(K, K)).cuda()
    v_b = (0.05 * torch.randn(K)).cuda()
    x1 = torch.from_numpy(make_bag(1, N, K)).cuda().to(torch.bfloat16)
    x64 = torch.cat([torch.from_numpy(make_bag(100 + i, N, K)) for i in range(64)]).cuda().to(torch.bfloat16)
    res = {"device": torch.cuda.get_device_name(0), "repeats": args.repeats, "window_s": args.window, "K": K, "Kv": K}
    with torch.no_grad():
        for key, x in (("tn_10000x512x512", x1), ("tn_640000x512x512", x64)):
            rows = x.shape[0]
            V = ops.value_proj(x, v_w, v_b)                      # the bf16 forward's own V
            g = torch.randn(rows, K, device="cuda")
            native = lambda: ops.value_proj_backward(x, V, g)
            parent = lambda: ops.value_proj_backward(x.float(), V.float(), g)
            if args.only_kernels:
                for _ in range(5):
                    native()
                    parent()
                torch.cuda.synchronize()
                continue
            x32, V32 = x.float(), V.float()
            r = abc({"native": native, "parent": parent, "fp32_kernel_alone": lambda: ops.value_proj_backward(x32, V32, g)},
                    args.repeats, args.window)
            del x32, V32
            t = r["native"]["median_us"] * 1e-6
            r["not_slower_than_parent_beyond_its_spread"] = \
                r["native"]["median_us"] <= r["parent"]["median_us"] + r["parent"]["spread_us"]
            r["speedup_over_parent"] = r["parent"]["median_us"] / r["native"]["median_us"]
            r["bytes"] = rows * (K * 2 + K * 2 + K * 4)
            r["GB_per_s"] = r["bytes"] / t / 1e9
            r["share_of_copy_ceiling"] = r["bytes"] / t / COPY_CEILING
            r["share_of_bf16_mfma_peak"] = 3 * 2.0 * rows * K * K / t / PEAK_BF16_DENSE
            res[key] = r
    if args.only_kernels:
        return
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
