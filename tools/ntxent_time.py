"""Times the NT-Xent loss, forward plus backward, on one GPU: the native path (csrc/ntxent.hip) against
  (a) the closed form from torch ops on the device (matmul + masked logsumexp under autograd), and
  (b) the reference-style broadcast cosine form (CosineSimilarity on [2N, 1, D] x [1, 2N, D], gather, cross-entropy),
      at N = 512 only by default: at N = 4096 its [2N, 2N, D] product is 64 GiB per copy; what happens is recorded.
hipEvents around one forward + backward, 5 warm-up runs, the median of 25 timed runs, 8 distinct input pairs in rotation (no run
re-reads the inputs of the run before it); torch.cuda.max_memory_allocated per method, reset before each.

    python tools/ntxent_time.py [--out profiles/ntxent/times.json] [--broadcast-at-4096]
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import dsmil  # noqa: E402,F401
from dsmil_wsi_amd.simclr import NTXentLoss, ntxent_composite  # noqa: E402


def broadcast_form(zis, zjs, T):
    """The reference's formulation (simclr/loss/nt_xent.py), restated: it materialises [2N, 2N, D]."""
    N = zis.shape[0]
    R = torch.cat([zjs, zis], 0)
    sim = torch.nn.functional.cosine_similarity(R.unsqueeze(1), R.unsqueeze(0), dim=-1)
    pos = torch.cat([torch.diag(sim, N), torch.diag(sim, -N)]).view(2 * N, 1)
    eye = torch.eye(2 * N, device=R.device, dtype=torch.bool)
    mask = ~(eye | torch.roll(eye, N, 1))
    logits = torch.cat((pos, sim[mask].view(2 * N, -1)), 1) / T
    labels = torch.zeros(2 * N, dtype=torch.long, device=R.device)
    return torch.nn.functional.cross_entropy(logits, labels, reduction="sum") / (2 * N)


def measure(fn, pairs, warmup=5, runs=25):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    times = []
    for i in range(warmup + runs):
        a, b = pairs[i % len(pairs)]
        a.grad = b.grad = None
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn(a, b).backward()
        e1.record()
        e1.synchronize()
        if i >= warmup:
            times.append(e0.elapsed_time(e1))
    times.sort()
    return {"median_ms": times[len(times) // 2], "min_ms": times[0], "max_ms": times[-1], "runs": runs,
            "peak_bytes_above_inputs": torch.cuda.max_memory_allocated() - base}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ntxent", "times.json"))
    ap.add_argument("--broadcast-at-4096", action="store_true")
    ap.add_argument("--sizes", type=int, nargs="*", default=[512, 4096])
    args = ap.parse_args()
    dev, D, T = "cuda:0", 256, 0.5
    out = {"device": torch.cuda.get_device_name(0), "D": D, "T": T, "method": __doc__.split("\n\n")[0], "sizes": {}}
    for N in args.sizes:
        g = torch.Generator(device="cpu").manual_seed(N)
        pairs = []
        for _ in range(8):
            a = torch.nn.functional.normalize(torch.randn(N, D, generator=g), dim=1)
            b = torch.nn.functional.normalize(0.9 * a + 0.44 * torch.nn.functional.normalize(torch.randn(N, D, generator=g), dim=1), dim=1)
            pairs.append((a.to(dev).requires_grad_(True), b.to(dev).requires_grad_(True)))
        crit = NTXentLoss(dev, N, T, True)
        res = {"input_bytes": 2 * N * D * 4}
        res["native"] = measure(crit, pairs)
        res["torch_closed_form"] = measure(lambda a, b: ntxent_composite(a, b, T, True), pairs)
        if N <= 512 or args.broadcast_at_4096:
            try:
                res["broadcast_form"] = measure(lambda a, b: broadcast_form(a, b, T), pairs, warmup=2, runs=20)
            except RuntimeError as e:      # out of memory is a result here, not a failure
                res["broadcast_form"] = {"error": str(e).split("\n")[0][:300]}
                torch.cuda.empty_cache()
        else:
            res["broadcast_form"] = {"skipped": "the [2N, 2N, D] fp32 product alone is %.0f GiB" % (4 * N * N * D * 4 / 2 ** 30)}
        la, lb = crit(*pairs[0]).item(), ntxent_composite(*pairs[0], T, True).item()
        res["loss_native"], res["loss_closed_form"] = la, lb
        out["sizes"][str(N)] = res
        print(N, json.dumps(res), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
