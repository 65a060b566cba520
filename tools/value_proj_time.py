"""Times the native value stream of BClassifier(passing_v=True) against the torch route it replaces (which stays callable):
  (a) the projection alone, 10 000 x 512 and 640 000 x 512:   ops.value_proj            vs  bc.v(x)  (nn.Linear + ReLU, rocBLAS)
  (b) MILNet.forward of one 10 000 x 512 passing_v bag:        net(x)                    vs  bc.v(x) + ops.agg_forward(vals=...)
  (c) forward_bags of 64 such bags:                            one projection + one call vs  the per-bag loop of (b)
Device-event times; every shape is warmed up first; a timed window repeats its call until it is >= --window seconds long; the
two sides alternate inside this one process, --repeats windows each (>= 5), so that the spread (max - min of a side's
windows) is known.  Writes every median and spread, and the projection's share of the fp16 MFMA peak, to
profiles/value_proj/times.json (--out) and prints the JSON.

    python tools/value_proj_time.py [--repeats 5] [--window 0.3] [--kernel-us-10k U --kernel-us-640k U]
`--kernel-us-*`: k_value_proj's kernel time from a separate `rocprofv3 --kernel-trace --stats -- python tools/value_proj_time.py
--only-proj` run; without it the share is computed from the event time of (a) (which includes the launch gap)."""
import argparse
import json
import os
import statistics

import _path  # noqa: F401
import torch

import dsmil  # noqa: F401  (registers the dsmil_wsi_amd package)
from dsmil_wsi_amd import modules as M
from dsmil_wsi_amd import ops
from dsmil_wsi_amd.synthetic import make_bag

PEAK_F16_DENSE = 2.5e15   # MI355X fp16 MFMA, FLOP/s


def window(fn, min_s):
    """One timed window: calls of fn between two device events until the window is at least min_s long -> seconds per call."""
    n = 1
    while True:
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(n):
            fn()
        b.record()
        b.synchronize()
        t = a.elapsed_time(b) * 1e-3
        if t >= min_s:
            return t / n
        n = max(n + 1, int(n * min(20.0, 1.3 * min_s / max(t, 1e-6))))


def ab(native, parent, repeats, min_s):
    for fn in (native, parent):   # warm-up: code objects, packed weights, rocBLAS's algorithm choice, workspaces
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
    ap.add_argument("--kernel-us-10k", type=float, default=None)
    ap.add_argument("--kernel-us-640k", type=float, default=None)
    ap.add_argument("--out", default=os.path.join(_path.ROOT, "profiles", "value_proj", "times.json"))
    args = ap.parse_args()
    if args.repeats < 5:
        ap.error("--repeats must be at least 5")
    K, C, N = 512, 2, 10000
    torch.manual_seed(0)
    net = M.MILNet(M.FCLayer(K, C), M.BClassifier(K, C, dropout_v=0.0, nonlinear=True, passing_v=True)).eval().cuda()
    bc, lin = net.b_classifier, net.i_classifier.fc[0]
    w = {k: (v.detach() if v is not None else None) for k, v in bc._weights().items()}
    w["fc_w"], w["fc_b"] = lin.weight.detach(), lin.bias.detach()
    v_w, v_b = bc.v[1].weight.detach(), bc.v[1].bias.detach()
    x1 = torch.from_numpy(make_bag(1, N, K)).cuda()
    x64 = torch.cat([torch.from_numpy(make_bag(100 + i, N, K)) for i in range(64)]).cuda()
    bags = list(x64.split(N))
    res = {"device": torch.cuda.get_device_name(0), "repeats": args.repeats, "window_s": args.window, "K": K, "C": C}
    with torch.no_grad():
        if args.only_proj:
            for _ in range(5):
                ops.value_proj(x1, v_w, v_b)
                ops.value_proj(x64, v_w, v_b)
            torch.cuda.synchronize()
            return

        def parent_forward(x):
            return ops.agg_forward(x, [x.shape[0]], w, vals=bc.v(x))
        res["proj_10000x512"] = ab(lambda: ops.value_proj(x1, v_w, v_b), lambda: bc.v(x1), args.repeats, args.window)
        res["proj_640000x512"] = ab(lambda: ops.value_proj(x64, v_w, v_b), lambda: bc.v(x64), args.repeats, args.window)
        res["forward_10000x512"] = ab(lambda: net(x1), lambda: parent_forward(x1), args.repeats, args.window)
        res["forward_bags_64x10000x512"] = ab(lambda: net.forward_bags(bags), lambda: [parent_forward(b) for b in bags],
                                               args.repeats, args.window)
    # the conditions of the change: (a) not slower than the parent route by more than its spread, (c) faster by more than it
    for key in ("proj_10000x512", "proj_640000x512"):
        r = res[key]
        r["not_slower"] = r["native"]["median_us"] <= r["parent"]["median_us"] + r["parent"]["spread_us"]
    r = res["forward_bags_64x10000x512"]
    r["faster"] = r["native"]["median_us"] < r["parent"]["median_us"] - r["parent"]["spread_us"]
    # share of the fp16 MFMA peak: three executed plane products per MAC, and the algorithmic one beside it
    for key, rows, kus in (("proj_10000x512", N, args.kernel_us_10k), ("proj_640000x512", 64 * N, args.kernel_us_640k)):
        t = (kus if kus is not None else res[key]["native"]["median_us"]) * 1e-6
        algo = 2.0 * rows * K * K
        res[key]["peak_share"] = {"time_us": t * 1e6, "time_from": "rocprofv3 kernel trace" if kus is not None else "device events",
                                  "executed_3_products": 3 * algo / t / PEAK_F16_DENSE, "algorithmic": algo / t / PEAK_F16_DENSE}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
