"""Times the aggregator backward over a batch of bags (ops.agg_backward_bags, csrc/agg_bwd_bags.h) against the route the
parent commit offers for the same bags and which stays callable: a loop of one ops.agg_backward call per bag, objective
of train_tcga.py:67-71 (g_pred + sparse g_max).  Shapes:
    64 x 10 000 x 512 with C = 1 and C = 2;  64 ragged bags (one of 60 000 rows, 63 of 64 rows) x 512;  64 x 300 x 1024.
Method of tools/gx_time.py: device events, both sides warmed up, then --repeats (>= 5) ALTERNATING windows (loop, batched,
loop, ...) of at least --window seconds per side in one process; median and spread (max - min) per side.
`--train`: bags/s of training.train at bags_per_step 1, 8 and 64 on cached 10 000 x 512 bags (a report, not a bar: one step
per 64 bags is a different optimisation schedule from one step per bag).  `--dtype bf16`: the cached rows are bf16-stored
(BagCache's dtype).  `--generic`: every cell a second time with args.fused_step = False, so one run prints the one-call step
and the generic loop side by side.  `--train-only`: skip the kernel shapes above.
`--only-step`: a few dsmil_agg_train_step_bags and dsmil_agg_train_step_bags_bf16 calls on 8 x 10 000 x 512 and exit (launch
counts per step from a `rocprofv3 --kernel-trace --stats` run).
`--only-kernels`: a few batched calls on the uniform C = 2 batch and exit (for a `rocprofv3 --kernel-trace --stats` run).
Writes profiles/bwd_bags/times.json (--out) and prints the JSON."""
import argparse
import json
import os
import statistics
import time
import types

import _path  # noqa: F401
import numpy as np
import torch

import dsmil  # noqa: F401  (registers the dsmil_wsi_amd package)
from dsmil_wsi_amd import modules as M
from dsmil_wsi_amd import ops, training
from dsmil_wsi_amd.synthetic import make_bag
from gx_time import window


def make_net(K, C):
    torch.manual_seed(0)
    return M.MILNet(M.FCLayer(K, C), M.BClassifier(K, C, dropout_v=0.0, nonlinear=True)).train().cuda()


def case(lengths, K, C):
    """(loop side, batched side) closures over one forward of the batch."""
    net = make_net(K, C)
    bc, lin = net.b_classifier, net.i_classifier.fc[0]
    w = {k: (v.detach() if v is not None else None) for k, v in bc._weights().items()}
    w["fc_w"], w["fc_b"] = lin.weight.detach(), lin.bias.detach()
    base = torch.from_numpy(make_bag(1, max(lengths), K)).cuda()
    x = torch.cat([base[:n] + 0.01 * b for b, n in enumerate(lengths)])
    classes, pred, A, B, idx = ops.agg_forward(x, lengths, w)
    labels = (torch.arange(len(lengths) * C, device="cuda").reshape(len(lengths), C) % 2).float()
    _, _, gp, gm = ops.agg_loss_head_bags(classes, lengths, pred, idx, labels)
    off = np.concatenate([[0], np.cumsum(lengths)])
    views = [(x[off[b]:off[b + 1]], A[off[b]:off[b + 1]], B[b:b + 1], idx[b:b + 1], gp[b], gm[b]) for b in range(len(lengths))]

    def loop():
        for xb, Ab, Bb, ib, gpb, gmb in views:
            ops.agg_backward(xb, w, Ab, Bb, ib, gpb, g_max=gmb)

    def batched():
        ops.agg_backward_bags(x, lengths, w, A, B, idx, gp, g_max=gm)
    return loop, batched


def alternating(loop, batched, repeats, min_s):
    for _ in range(3):
        loop(); batched()
    torch.cuda.synchronize()
    t = {"loop": [], "batched": []}
    for _ in range(repeats):
        t["loop"].append(window(loop, min_s))
        t["batched"].append(window(batched, min_s))
    out = {k: {"median_us": statistics.median(v) * 1e6, "spread_us": (max(v) - min(v)) * 1e6,
               "windows_us": [round(u * 1e6, 1) for u in v]} for k, v in t.items()}
    out["speedup"] = out["loop"]["median_us"] / out["batched"]["median_us"]
    out["batched_faster_by_more_than_both_spreads"] = bool(
        out["loop"]["median_us"] - out["batched"]["median_us"] > max(out["loop"]["spread_us"], out["batched"]["spread_us"]))
    return out


def train_rates(n_bags, rows, K, dtype=torch.float32, fused=True):
    bags = [(torch.from_numpy(make_bag(100 + i, rows, K)).cuda().to(dtype), torch.tensor([float(i % 2), float(1 - i % 2)], device="cuda"))
            for i in range(n_bags)]
    cache = types.SimpleNamespace(get=lambda item, feats_size=None: bags[item])
    crit = torch.nn.BCEWithLogitsLoss()
    res = {}
    for per_step in (1, 8, 64):
        net = make_net(K, 2)
        opt = torch.optim.Adam(net.parameters(), lr=1e-4, betas=(0.5, 0.9), weight_decay=1e-3)
        args = types.SimpleNamespace(feats_size=K, dropout_patch=0, bags_per_step=per_step, fused_step=fused)
        rates = []
        for epoch in range(4):   # the first epoch warms up
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            training.train(args, list(range(n_bags)), net, crit, opt, cache=cache, log=False)
            torch.cuda.synchronize()
            rates.append(n_bags / (time.perf_counter() - t0))
        res[f"bags_per_step_{per_step}"] = {"bags_per_s_median": statistics.median(rates[1:]),
                                            "bags_per_s_spread": max(rates[1:]) - min(rates[1:]),
                                            "epochs_bags_per_s": [round(r, 1) for r in rates]}
    return res


def only_step():
    """Five one-call steps per entry on 8 x 10 000 x 512 (fp32 rows, then bf16-stored rows)."""
    net = make_net(512, 2)
    opt = torch.optim.Adam(net.parameters(), lr=1e-4, betas=(0.5, 0.9), weight_decay=1e-3)
    fused = training.FusedTrainStep.create(net, torch.nn.BCEWithLogitsLoss(), opt)
    x = torch.cat([torch.from_numpy(make_bag(100 + i, 10000, 512)) for i in range(8)]).cuda()
    labels = (torch.arange(16, device="cuda").reshape(8, 2) % 2).float()
    for rows in (x, x.to(torch.bfloat16)):
        for _ in range(5):
            fused.step_bags(rows, [10000] * 8, labels)
    torch.cuda.synchronize()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.3)
    ap.add_argument("--train", action="store_true")
    ap.add_argument("--only-kernels", action="store_true")
    ap.add_argument("--only-step", action="store_true")
    ap.add_argument("--train-only", action="store_true")
    ap.add_argument("--dtype", choices=("fp32", "bf16"), default="fp32")
    ap.add_argument("--generic", action="store_true")
    ap.add_argument("--out", default=os.path.join(_path.ROOT, "profiles", "bwd_bags", "times.json"))
    args = ap.parse_args()
    if args.repeats < 5:
        ap.error("--repeats must be at least 5")
    if args.only_kernels:
        _, batched = case([10000] * 64, 512, 2)
        for _ in range(5):
            batched()
        torch.cuda.synchronize()
        return
    if args.only_step:
        only_step()
        return
    res = {"device": torch.cuda.get_device_name(0), "repeats": args.repeats, "window_s": args.window}
    shapes = {"64x10000x512_C1": ([10000] * 64, 512, 1), "64x10000x512_C2": ([10000] * 64, 512, 2),
              "ragged_60000_and_63x64_x512_C2": ([64] * 31 + [60000] + [64] * 32, 512, 2), "64x300x1024_C2": ([300] * 64, 1024, 2)}
    for name, (lengths, K, C) in ({} if args.train_only else shapes).items():
        res[name] = alternating(*case(lengths, K, C), args.repeats, args.window)
        res[name]["bags"] = len(lengths)
    if args.train or args.train_only:
        dtype = torch.bfloat16 if args.dtype == "bf16" else torch.float32
        tag = "" if args.dtype == "fp32" else "_bf16"
        res[f"train_10000x512{tag}_bags_per_s"] = train_rates(128, 10000, 512, dtype)
        if args.generic:
            res[f"train_10000x512{tag}_generic_bags_per_s"] = train_rates(128, 10000, 512, dtype, fused=False)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
