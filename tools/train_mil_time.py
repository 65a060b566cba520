#!/usr/bin/env python3
"""Seconds per epoch of train_mil.py's loop — training.mil_epoch_train + mil_epoch_test — on the synthetic stand-in for MUSK1
(training.write_synthetic_mil_file: 92 bags / 476 instances / 166 features), the model, criterion (BCEWithLogitsLoss with
the fold's pos_weight) and optimiser of train_mil.py:169-175: the native path (one dsmil_agg_train_step_bags_w per bag, one
batched forward + loss head per test pass) against the same loop with ``training.mil_fused_step`` off (the reference's
lines: an upload, autograd, torch.optim.Adam and a loss.item() per bag), from the same weights and the same seeds.
    python tools/train_mil_time.py [--epochs 20] [--warmup 3] [--json]
Prints the median and the fastest epoch of each path and the last epoch's losses of both (they follow each other to
rounding: tests/test_wbce_gpu.py)."""
import _path  # noqa: F401
import argparse
import copy
import json
import os
import tempfile
import time

import numpy as np
import torch
import torch.nn as nn

import dsmil as mil
from dsmil_wsi_amd import training as T


def run(native, bags, ys, train_idx, test_idx, start, epochs, warmup, device):
    T.mil_fused_step = native
    net = copy.deepcopy(start).to(device)
    pos = float(ys[train_idx].sum())
    crit = nn.BCEWithLogitsLoss(torch.tensor((len(train_idx) - pos) / max(pos, 1.0), device=device))
    opt = torch.optim.Adam(net.parameters(), lr=2e-4, betas=(0.5, 0.9), weight_decay=5e-3)
    np.random.seed(0)
    times, last = [], None
    for epoch in range(warmup + epochs):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        tr = T.mil_epoch_train(bags, ys, train_idx, net, crit, opt, device)
        te, _ = T.mil_epoch_test(bags, ys, test_idx, net, crit, device)
        torch.cuda.synchronize()
        if epoch >= warmup:
            times.append(time.perf_counter() - t0)
        last = (tr, te)
    return times, last


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--epochs", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--json", action="store_true")
    args = ap.parse_args()
    device = torch.device("cuda")
    with tempfile.TemporaryDirectory() as d:
        X, bag_ids, labels = T.parse_mil_file(T.write_synthetic_mil_file(os.path.join(d, "musk1_synthetic.svm")))
    bags, ys = T.group_bags(X, bag_ids, labels)
    order = np.random.default_rng(0).permutation(len(bags))
    test_idx, train_idx = order[:9], order[9:]          # one fold of train_mil.py's ten (train_mil.py:99-104)
    torch.manual_seed(0)
    start = mil.MILNet(mil.FCLayer(X.shape[1], 1), mil.BClassifier(input_size=X.shape[1], output_class=1))
    out = {"bags": len(bags), "train_bags": len(train_idx), "test_bags": len(test_idx), "epochs": args.epochs}
    for name, native in (("native", True), ("generic", False)):
        times, last = run(native, bags, ys, train_idx, test_idx, start, args.epochs, args.warmup, device)
        out[name] = {"median_s_per_epoch": float(np.median(times)), "min_s_per_epoch": float(np.min(times)),
                     "last_train_loss": last[0], "last_test_loss": last[1]}
    out["speedup_median"] = out["generic"]["median_s_per_epoch"] / out["native"]["median_s_per_epoch"]
    if args.json:
        print(json.dumps(out))
    else:
        for name in ("native", "generic"):
            r = out[name]
            print(f"{name:8s} median {r['median_s_per_epoch'] * 1e3:8.2f} ms / epoch   fastest {r['min_s_per_epoch'] * 1e3:8.2f} ms   "
                  f"last losses {r['last_train_loss']:.6f} / {r['last_test_loss']:.6f}")
        print(f"native is {out['speedup_median']:.2f}x the generic loop's epochs per second ({out['train_bags']} training bags, "
              f"{out['test_bags']} test bags per epoch)")


if __name__ == "__main__":
    main()
