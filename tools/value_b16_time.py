"""Times the native value stream on bf16-stored rows (ops.value_proj on bf16 rows: dsmil_value_forward_bf16, k_value_proj_b16)
and, on the same device in the same run, the route it replaces: nn.Linear + ReLU of a module after .bfloat16().
  (a) the projection alone, 1 x 10 000 x 512 and 64 x 10 000 x 512 rows:  ops.value_proj  vs  bc.v(x)
      with the GB/s the native time implies (every row read once, every value row written once: rows (K + Kv) 2 bytes) and
      its share of the bf16 MFMA peak;
  (b) the bf16 forward of the same rows through MILNet(passing_v=True) — one 10 000-row bag (net(x)), 64 bags
      (net.forward_bags) — and the projection's share of it.
Device-event times; every shape is warmed up first; a timed window repeats its call until it is >= --window seconds long; the
two sides of (a) alternate inside this one process, --repeats windows each (>= 5), so that the spread (max - min of a side's
windows) is known.  A window of one launch per call includes the launch gap; at 64 x 10 000 rows that is a fraction of a
percent.  Asserts no time.  Writes every median and spread to profiles/value_b16/times.json (--out) and prints the JSON.

    python tools/value_b16_time.py [--repeats 5] [--window 0.3] [--only-proj]
`--only-proj`: run the two projections a few times and exit (for a `rocprofv3 --kernel-trace --stats` run of its own)."""
import argparse
import copy
import json
import os
import statistics

import _path  # noqa: F401
import torch

import dsmil  # noqa: F401  (registers the dsmil_wsi_amd package)
from dsmil_wsi_amd import modules as M
from dsmil_wsi_amd import ops
from dsmil_wsi_amd.synthetic import make_bag
from value_proj_time import window

PEAK_BF16_DENSE = 2.5e15   # MI355X bf16 MFMA, FLOP/s
COPY_CEILING = 6.29e12     # MI355X achievable HBM copy rate, bytes/s (a float4 copy kernel; 8.0e12 is the data sheet's)


def ab(native, parent, repeats, min_s):
    for fn in (native, parent):   # warm-up: code objects, packed weights, the GEMM library's algorithm choice
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    tn, tp = [], []
    for _ in range(repeats):
        tn.append(window(native, min_s))
        tp.append(window(parent, min_s))
    side = lambda t: {"median_us": statistics.median(t) * 1e6, "spread_us": (max(t) - min(t)) * 1e6,
                      "windows_us": [round(v * 1e6, 2) for v in t]}
    return {"native": side(tn), "parent": side(tp)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.3)
    ap.add_argument("--only-proj", action="store_true", help="run the two projections a few times and exit (for a kernel trace)")
    ap.add_argument("--out", default=os.path.join(_path.ROOT, "profiles", "value_b16", "times.json"))
    args = ap.parse_args()
    if args.repeats < 5:
        ap.error("--repeats must be at least 5")
    K, C, N = 512, 2, 10000
    torch.manual_seed(0)
    net = M.MILNet(M.FCLayer(K, C), M.BClassifier(K, C, dropout_v=0.0, nonlinear=True, passing_v=True)).eval().cuda()
    bc = net.b_classifier
    v_w, v_b = bc.v[1].weight.detach(), bc.v[1].bias.detach()
    x1 = torch.from_numpy(make_bag(1, N, K)).cuda().to(torch.bfloat16)
    x64 = torch.cat([torch.from_numpy(make_bag(100 + i, N, K)) for i in range(64)]).cuda().to(torch.bfloat16)
    bags = list(x64.split(N))
    v_b16 = copy.deepcopy(bc.v).to(torch.bfloat16).eval()   # the parent route: torch's nn.Linear + ReLU on bf16 parameters
    res = {"device": torch.cuda.get_device_name(0), "repeats": args.repeats, "window_s": args.window, "K": K, "C": C}
    with torch.no_grad():
        if args.only_proj:
            for _ in range(5):
                ops.value_proj(x1, v_w, v_b)
                ops.value_proj(x64, v_w, v_b)
            torch.cuda.synchronize()
            return
        res["proj_10000x512"] = ab(lambda: ops.value_proj(x1, v_w, v_b), lambda: v_b16(x1), args.repeats, args.window)
        res["proj_640000x512"] = ab(lambda: ops.value_proj(x64, v_w, v_b), lambda: v_b16(x64), args.repeats, args.window)
        for fn in (lambda: net(x1), lambda: net.forward_bags(bags)):
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        fwd1 = [window(lambda: net(x1), args.window) for _ in range(args.repeats)]
        fwd64 = [window(lambda: net.forward_bags(bags), args.window) for _ in range(args.repeats)]
    for key, rows, fwd in (("proj_10000x512", N, fwd1), ("proj_640000x512", 64 * N, fwd64)):
        r = res[key]
        t = r["native"]["median_us"] * 1e-6
        r["not_slower_than_parent"] = r["native"]["median_us"] <= r["parent"]["median_us"]
        r["bytes"] = rows * (K + K) * 2
        r["GB_per_s"] = r["bytes"] / t / 1e9
        r["share_of_copy_ceiling"] = r["bytes"] / t / COPY_CEILING
        r["share_of_bf16_mfma_peak"] = 2.0 * rows * K * K / t / PEAK_BF16_DENSE
        f = statistics.median(fwd)
        r["bf16_forward"] = {"median_us": f * 1e6, "spread_us": (max(fwd) - min(fwd)) * 1e6, "projection_share": t / f}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
