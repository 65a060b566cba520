"""Times loss.backward() when the INPUT rows require a gradient (x.requires_grad_()), objective of train_tcga.py:67-71:
  (a) a 10 000 x 512 tcga bag, v = Identity        MILNet(FCLayer, BClassifier)
  (b) the same with passing_v=True
  (c) a 300 x 1024 tree bag, v = Identity
and, where the library has them, the two row-gradient kernels alone (ops.value_proj_backward_rows = k_value_gx;
ops.agg_backward with and without want_g_feats, the difference = k_bwd_gx).  The script uses only the module API, so the
SAME file run in a checkout of the parent commit times the parent's route (torch dense backward / nn.Linear autograd):
    (parent checkout)  python tools/gx_time.py --out parent.json
    (this checkout)    python tools/gx_time.py --parent-json parent.json
The comparison is always against the parent commit's figures, never against this code itself.  Device-event times; every
case is warmed up first; a timed window repeats backward(retain_graph=True) on one recorded graph until it is >= --window
seconds long; --repeats windows (>= 5) per case, median and spread (max - min) reported.  One process.
`--kernel-us-bwd-gx U --kernel-us-value-gx U`: the kernels' times from a separate
`rocprofv3 --kernel-trace --stats -- python tools/gx_time.py --only-kernels` run; k_bwd_gx's achieved bytes/s against the
HBM roof for its algorithmic traffic and k_value_gx's share of the bf16 MFMA peak at six plane products per MAC are
computed from them (from the device-event times otherwise).  Writes profiles/gx/times.json (--out) and prints the JSON."""
import argparse
import json
import os
import statistics

import _path  # noqa: F401
import torch
import torch.nn.functional as F

import dsmil  # noqa: F401  (registers the dsmil_wsi_amd package)
from dsmil_wsi_amd import modules as M
from dsmil_wsi_amd import ops
from dsmil_wsi_amd.synthetic import make_bag

PEAK_BF16_DENSE = 2.5e15   # MI355X bf16 MFMA, FLOP/s
HBM_ROOF = 8.0e12          # MI355X HBM3E, B/s


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


def timed(fn, repeats, min_s):
    for _ in range(5):   # warm-up: code objects, packed weights, rocBLAS's algorithm choice, workspaces
        fn()
    torch.cuda.synchronize()
    t = [window(fn, min_s) for _ in range(repeats)]
    return {"median_us": statistics.median(t) * 1e6, "spread_us": (max(t) - min(t)) * 1e6,
            "windows_us": [round(v * 1e6, 2) for v in t]}


def make_net(K, C, passing_v):
    torch.manual_seed(0)
    return M.MILNet(M.FCLayer(K, C), M.BClassifier(K, C, dropout_v=0.0, nonlinear=True, passing_v=passing_v)).train().cuda()


def backward_case(K, N, passing_v, repeats, min_s):
    net = make_net(K, 2, passing_v)
    x = torch.from_numpy(make_bag(1, N, K)).cuda().requires_grad_(True)
    y = torch.tensor([[1.0, 0.0]], device="cuda")
    ins, bag, _, _ = net(x)
    mx, _ = torch.max(ins, 0)
    loss = 0.5 * F.binary_cross_entropy_with_logits(bag.view(1, -1), y) + 0.5 * F.binary_cross_entropy_with_logits(mx.view(1, -1), y)
    return timed(lambda: loss.backward(retain_graph=True), repeats, min_s)


def kernel_inputs(K, N):
    net = make_net(K, 2, True)
    bc, lin = net.b_classifier, net.i_classifier.fc[0]
    w = {k: (v.detach() if v is not None else None) for k, v in bc._weights().items()}
    w["fc_w"], w["fc_b"] = lin.weight.detach(), lin.bias.detach()
    x = torch.from_numpy(make_bag(1, N, K)).cuda()
    v_w = bc.v[1].weight.detach()
    V = ops.value_proj(x, v_w, bc.v[1].bias.detach())
    g = torch.randn(N, K, device="cuda")
    _, _, A, B, idx = ops.agg_forward(x, [N], w)
    gp, gm = torch.tensor([0.1, -0.2], device="cuda"), torch.tensor([0.3, 0.1], device="cuda")
    return x, w, V, g, v_w, A, B, idx, gp, gm


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.3)
    ap.add_argument("--only-kernels", action="store_true", help="run the two kernels a few times and exit (for a kernel trace)")
    ap.add_argument("--parent-json", default=None, help="the output of this script run in a checkout of the parent commit")
    ap.add_argument("--kernel-us-bwd-gx", type=float, default=None)
    ap.add_argument("--kernel-us-value-gx", type=float, default=None)
    ap.add_argument("--out", default=os.path.join(_path.ROOT, "profiles", "gx", "times.json"))
    args = ap.parse_args()
    if args.repeats < 5:
        ap.error("--repeats must be at least 5")
    K, N = 512, 10000
    have = hasattr(ops, "value_proj_backward_rows")
    res = {"device": torch.cuda.get_device_name(0), "repeats": args.repeats, "window_s": args.window,
           "native_row_gradients": have}
    if have:
        x, w, V, g, v_w, A, B, idx, gp, gm = kernel_inputs(K, N)
        rows = lambda want: ops.agg_backward(x, w, A, B, idx, gp, g_max=gm, want_g_feats=want)
        if args.only_kernels:
            for _ in range(5):
                ops.value_proj_backward_rows(V, g, v_w)
                rows(True)
            torch.cuda.synchronize()
            return
        out = torch.empty(N, K, device="cuda")
        res["k_value_gx_10000x512x512"] = timed(lambda: ops.value_proj_backward_rows(V, g, v_w, out=out), args.repeats, args.window)
        res["agg_backward_10000x512_with_g_feats"] = timed(lambda: rows(True), args.repeats, args.window)
        res["agg_backward_10000x512_without"] = timed(lambda: rows(False), args.repeats, args.window)
        d = res["agg_backward_10000x512_with_g_feats"]["median_us"] - res["agg_backward_10000x512_without"]["median_us"]
        tb = (args.kernel_us_bwd_gx if args.kernel_us_bwd_gx is not None else d) * 1e-6
        traffic = 4.0 * (N * K + N * 128 + 128 * K + 2 * N * 2 + 2 * 2 * K)   # g_x out; gH, W1, A, g_c-free tail, Wf / gB in
        res["k_bwd_gx_10000x512"] = {"time_us": tb * 1e6,
                                     "time_from": "rocprofv3 kernel trace" if args.kernel_us_bwd_gx is not None
                                     else "device events: backward with - without g_feats",
                                     "algorithmic_bytes": traffic, "bytes_per_s": traffic / tb, "hbm_roof_share": traffic / tb / HBM_ROOF}
        tv = (args.kernel_us_value_gx if args.kernel_us_value_gx is not None else res["k_value_gx_10000x512x512"]["median_us"]) * 1e-6
        algo = 2.0 * N * K * K
        res["k_value_gx_10000x512x512"]["peak_share"] = {
            "time_us": tv * 1e6, "time_from": "rocprofv3 kernel trace" if args.kernel_us_value_gx is not None else "device events",
            "executed_6_products": 6 * algo / tv / PEAK_BF16_DENSE, "algorithmic": algo / tv / PEAK_BF16_DENSE}
    elif args.only_kernels:
        return
    res["backward_rows_tcga_10000x512"] = backward_case(512, 10000, False, args.repeats, args.window)
    res["backward_rows_passing_v_10000x512"] = backward_case(512, 10000, True, args.repeats, args.window)
    res["backward_rows_tree_300x1024"] = backward_case(1024, 300, False, args.repeats, args.window)
    if args.parent_json:
        par = json.load(open(args.parent_json))
        res["parent"] = {k: par[k] for k in par if k.startswith("backward_rows_")}
        for k in list(res["parent"]):
            p, t = res["parent"][k], res[k]
            res[k]["parent_median_us"] = p["median_us"]
            res[k]["speedup_vs_parent"] = p["median_us"] / t["median_us"]
            res[k]["faster_than_parent"] = t["median_us"] < p["median_us"] - max(p["spread_us"], t["spread_us"])
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
