"""Times the native stem of the embedder's training path (csrc/stem_bwd.hip: ops.stem_pool_backward; ops.trunk32_stem_train;
simclr.use_native_stem) against the torch stem it replaces, at 224 x 224 (raw map 112^2 x 64, pooled 56^2 x 64), batch 64 and 256.

(a) The backward call alone: hipEvents around one ops.stem_pool_backward, 5 warm-up runs, the median of 25 timed runs, 3 distinct
input sets in rotation (no run re-reads the inputs of the run before it).  Two byte counts over the time, against the 6.29 TB/s
measured copy ceiling: the FLOOR (y read twice, g read once, gy written once) and what the call ACTUALLY asks for (y, g and the
winners each read in both passes, gy written once; neighbouring pixels share g and winner lines, so the cache serves most of the
repeats).  Beside it torch's three backward ops on the SAME y seen as a channels_last NCHW tensor: the backward of
max_pool2d(relu(instance_norm(y)), 3, 2, 1) with the forward graph built beforehand (retain_graph), so only the backward is
timed; ratio = native time / torch time (above 1: the native call loses).

(b) The stem alone, forward plus backward to conv1's weight gradient (loss = mean of the squared pooled map): the torch stem of
the training path so far (conv1 as NativeConv2d after use_native_convs — aten's forward, the native weight gradient — then
InstanceNorm2d, in-place ReLU, MaxPool2d) against the same model after use_native_stem.  Five runs of each, INTERLEAVED; a run is
the median of 10 steps after 3 warm-up steps; torch.cuda.max_memory_allocated over the timed steps, less what was resident.

(c) The whole ResNet-18 trunk step (fc = Identity, loss = mean of the squared features): use_native_blocks + use_native_convs
against the same plus use_native_stem, five interleaved runs of each as in (b).

    python tools/stem_bwd_time.py [--out-dir profiles/stem_bwd] [--batches 64 256] [--only-call] [--name times.json]

--only-call stops after (a): with an experiment build (build.py --variant expt -DDSMIL_EXPERIMENTS, DSMIL_NATIVE_LIB=
libdsmil_hip_expt.so) and DSMIL_STEM_BWD=recompute it times the form of the backward that recomputes the winners from y.
"""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import dsmil  # noqa: E402,F401
from dsmil_wsi_amd import ops, simclr  # noqa: E402
from dsmil_wsi_amd.resnet import resnet18  # noqa: E402

SETS, WARMUP, RUNS, REPEATS = 3, 5, 25, 5
COPY_CEILING = 6.29e12
HW_IN, H1, HP, C = 224, 112, 56, 64


def median_ms(fn, n_sets, warmup=WARMUP, runs=RUNS):
    times = []
    for i in range(warmup + runs):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn(i % n_sets)
        e1.record()
        e1.synchronize()
        if i >= warmup:
            times.append(e0.elapsed_time(e1))
    times.sort()
    return times[len(times) // 2]


def time_call(B, dev):
    gen = torch.Generator(device=dev).manual_seed(B)
    sets = []
    for _ in range(SETS):
        x = torch.rand(B, 3, HW_IN, HW_IN, device=dev, generator=gen)
        w = torch.randn(64, 3, 7, 7, device=dev, generator=gen) * (2.0 / (64 * 49)) ** 0.5
        pooled, y, stats, win = ops.trunk32_stem_train(x, w)
        g = torch.randn(B, HP, HP, C, device=dev, generator=gen) * 1e-5
        ty = y.permute(0, 3, 1, 2).requires_grad_(True)                                           # channels_last, no copy
        out = F.max_pool2d(torch.relu(F.instance_norm(ty)), 3, 2, 1)
        sets.append(dict(g=g, y=y, stats=stats, win=win, t_out=out, t_y=ty, t_g=g.permute(0, 3, 1, 2)))
        del x, pooled
    ws = torch.empty(ops._native.lib().dsmil_stem_pool_bwd_workspace_bytes(B, H1, H1, C), dtype=torch.uint8, device=dev)

    def native(i):
        s = sets[i]
        return ops.stem_pool_backward(s["g"], s["y"], s["stats"], s["win"], ws=ws)

    def torch_fn(i):
        s = sets[i]
        return torch.autograd.grad(s["t_out"], [s["t_y"]], s["t_g"], retain_graph=True)

    tn, tt = median_ms(native, SETS), median_ms(torch_fn, SETS)
    raw, pool = B * H1 * H1 * C, B * HP * HP * C
    floor = 4.0 * (3 * raw + pool)
    asked = 4.0 * (3 * raw + 2 * pool) + 2.0 * pool
    return {"native_ms": tn, "torch_ms": tt, "ratio_native_over_torch": tn / tt, "floor_bytes": floor, "asked_bytes": asked,
            "native_floor_bytes_per_s": floor / (tn * 1e-3), "native_floor_frac_of_copy_ceiling": floor / (tn * 1e-3) / COPY_CEILING,
            "native_asked_bytes_per_s": asked / (tn * 1e-3), "native_asked_frac_of_copy_ceiling": asked / (tn * 1e-3) / COPY_CEILING,
            "plan": ops.stem_pool_backward_plan(B, H1, H1, C)}


def make_model(dev, stem):
    torch.manual_seed(0)
    model = resnet18(norm_layer=torch.nn.InstanceNorm2d)
    model.fc = torch.nn.Identity()
    model = model.to(dev).train()
    assert simclr.use_native_blocks(model) == 8 and simclr.use_native_convs(model) == 20
    if stem:
        assert simclr.use_native_stem(model) == 1
    return model


def one_run(model, x, whole):
    """{"ms": the median step, "peak_bytes": the peak over the timed steps less what was resident before them}."""
    params = list(model.parameters()) if whole else [model.conv1.weight]
    forward = model if whole else (lambda t: simclr.stem_forward(model, t) if getattr(model, "_native_stem", False)
                                   else model.maxpool(model.relu(model.bn1(model.conv1(t)))))

    def step(_):
        for p in params:
            p.grad = None
        forward(x).square().mean().backward()

    step(0)
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    ms = median_ms(step, 1, warmup=3, runs=10)
    torch.cuda.synchronize()
    return {"ms": ms, "peak_bytes": torch.cuda.max_memory_allocated() - base}


def interleaved(B, dev, whole):
    x = torch.rand(B, 3, HW_IN, HW_IN, device=dev)
    models = {"torch_stem": make_model(dev, False), "native_stem": make_model(dev, True)}
    runs = {k: [] for k in models}
    for _ in range(REPEATS):
        for k, m in models.items():
            runs[k].append(one_run(m, x, whole))
            torch.cuda.empty_cache()
    res = {}
    for k, v in runs.items():
        ms = sorted(r["ms"] for r in v)
        res[k] = {"runs_ms": [r["ms"] for r in v], "median_ms": ms[len(ms) // 2], "fastest_ms": ms[0], "slowest_ms": ms[-1],
                  "peak_bytes": max(r["peak_bytes"] for r in v)}
    t, n = res["torch_stem"], res["native_stem"]
    res["ratio_native_over_torch"] = n["median_ms"] / t["median_ms"]
    res["torch_scatter_ms"] = t["slowest_ms"] - t["fastest_ms"]
    res["native_median_within_torch_scatter"] = n["median_ms"] <= t["median_ms"] + res["torch_scatter_ms"]
    res["native_median_not_above_torch_slowest"] = n["median_ms"] <= t["slowest_ms"]
    res["peak_ratio_native_over_torch"] = n["peak_bytes"] / t["peak_bytes"]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles", "stem_bwd"))
    ap.add_argument("--batches", type=int, nargs="*", default=[64, 256])
    ap.add_argument("--only-call", action="store_true")
    ap.add_argument("--name", default="times.json")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("stem_bwd_time.py measures on the GPU; none is visible")
    dev = "cuda:0"
    os.makedirs(args.out_dir, exist_ok=True)
    parts = __doc__.split("\n\n")
    out = {"device": torch.cuda.get_device_name(0), "copy_ceiling_bytes_per_s": COPY_CEILING, "input": HW_IN,
           "method": {"call": parts[1], "stem": parts[2], "step": parts[3]}, "batches": {},
           "library": os.path.basename(ops._native.LIB_PATH), "DSMIL_STEM_BWD": os.environ.get("DSMIL_STEM_BWD", "")}
    for B in args.batches:
        res = {"call": time_call(B, dev)}
        torch.cuda.empty_cache()
        print(B, "call", json.dumps({k: v for k, v in res["call"].items() if k != "plan"}), flush=True)
        for what, whole in () if args.only_call else (("stem", False), ("step", True)):
            res[what] = interleaved(B, dev, whole)
            torch.cuda.empty_cache()
            print(B, what, json.dumps(res[what]), flush=True)
        if not args.only_call:
            res["stem_share_of_step"] = {k: res["stem"][k]["median_ms"] / res["step"][k]["median_ms"] for k in ("torch_stem", "native_stem")}
        out["batches"][str(B)] = res
        with open(os.path.join(args.out_dir, args.name), "w") as f:
            json.dump(out, f, indent=1)
    print("wrote", os.path.join(args.out_dir, args.name))


if __name__ == "__main__":
    main()
