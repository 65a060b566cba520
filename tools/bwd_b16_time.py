"""Times the aggregator backward on bf16-stored rows (ops.agg_backward_bags on bf16 rows: dsmil_agg_backward_bags_bf16) and,
on the same device in the same run, the route it replaces: feats.float() — an fp32 copy of every row in HBM — followed by
dsmil_agg_backward_bags on the copy.  Both sides get the same A, B, idx (the bf16 forward's) and the same bf16-rounded
weights, and compute the same gradient.
  shapes: 1 x 10 000 x 512 (the hidden-split tile) and 16 x 10 000 x 512 (the four-wave tile), C = 2, the training
  objective's upstream gradients (g_pred, sparse g_max).
Device-event times; every shape is warmed up first; a timed window repeats its call until it is >= --window seconds long; the
two sides alternate inside this one process, --repeats windows each (>= 5), so that the spread (max - min of a side's windows)
is known.  Asserts no time.  Writes every median and spread, and the bytes of row storage each side reads per row, to
profiles/bwd_b16/times.json (--out) and prints the JSON.

    python tools/bwd_b16_time.py [--repeats 5] [--window 0.3]"""
import argparse
import json
import os

import _path  # noqa: F401
import torch

import dsmil  # noqa: F401  (registers the dsmil_wsi_amd package)
from dsmil_wsi_amd import ops
from dsmil_wsi_amd.synthetic import load_weights, make_bag
from value_b16_time import ab


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.3)
    ap.add_argument("--out", default=os.path.join(_path.ROOT, "profiles", "bwd_b16", "times.json"))
    args = ap.parse_args()
    if args.repeats < 5:
        ap.error("--repeats must be at least 5")
    K, C, N = 512, 2, 10000
    w = {k: torch.from_numpy(v).cuda().to(torch.bfloat16).float() for k, v in load_weights("tcga").items()}
    res = {"device": torch.cuda.get_device_name(0), "repeats": args.repeats, "window_s": args.window, "K": K, "C": C}
    for n_bags in (1, 16):
        lengths = [N] * n_bags
        xb = torch.cat([torch.from_numpy(make_bag(300 + i, N, K)) for i in range(n_bags)]).cuda().to(torch.bfloat16)
        _, _, A, B, idx = ops.agg_forward(xb, lengths, w)
        g = torch.Generator().manual_seed(n_bags)
        g_pred, g_max = (torch.randn(n_bags, C, generator=g).cuda() for _ in range(2))
        native = lambda: ops.agg_backward_bags(xb, lengths, w, A, B, idx, g_pred, g_max=g_max)
        widen = lambda: ops.agg_backward_bags(xb.float(), lengths, w, A, B, idx, g_pred, g_max=g_max)
        r = ab(native, widen, args.repeats, args.window)
        r["not_slower_than_parent"] = r["native"]["median_us"] <= r["parent"]["median_us"]
        r["native_over_parent"] = r["native"]["median_us"] / r["parent"]["median_us"]
        # row storage read per row and pass (the widen route also reads the bf16 rows once and WRITES the fp32 copy once)
        r["row_bytes_per_pass"] = {"native": 2 * K, "parent": 4 * K}
        r["parent_copy_bytes_per_row"] = 2 * K + 4 * K
        res[f"{n_bags}x{N}x{K}"] = r
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
