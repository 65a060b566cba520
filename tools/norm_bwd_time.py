"""Times the native InstanceNorm / ReLU / residual-add backward (csrc/norm_bwd.hip: ops.norm_backward) and the training step it
completes.

(a) Per kind ("relu", "add", "add_down") at the block shapes of ResNet-18 at 224 x 224 (56^2 x 64, 28^2 x 128, 14^2 x 256,
7^2 x 512), batch 64 and 256: hipEvents around one call, 5 warm-up runs, the median of 25 timed runs, 4 distinct input sets in
rotation (no run re-reads the inputs of the run before it).  Achieved bytes/s = the bytes the call MUST move (every operand read
once, every result written once: 3 maps for "relu", 5 for "add", 6 for "add_down", plus the statistics) over the time, against
the 6.29 TB/s measured copy ceiling.  Beside it the same chain through torch autograd on the SAME buffers seen as channels_last
NCHW tensors: the backward of relu(instance_norm(y) [+ idn | + instance_norm(yd)]) with the forward graph built beforehand
(retain_graph), so only the backward is timed; ratio = native time / torch time (above 1: the native call loses).

(b) Forward plus backward of the ResNet-18 InstanceNorm trunk (fc = Identity, loss = mean of the squared features) at 224 x 224,
batch 64 and 256: the plain torch model (NCHW, and channels_last) against the same model after use_native_blocks +
use_native_convs; the median of 10 steps after 3 warm-up steps, and torch.cuda.max_memory_allocated over the timed steps.

    python tools/norm_bwd_time.py [--out-dir profiles/norm_bwd] [--batches 64 256] [--skip-step]
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

SETS, WARMUP, RUNS = 4, 5, 25
COPY_CEILING = 6.29e12
SHAPES = [(56 * 56, 64), (28 * 28, 128), (14 * 14, 256), (7 * 7, 512)]
MAPS_MOVED = {"relu": 3, "add": 5, "add_down": 6}
STATS_MOVED = {"relu": 2, "add": 2, "add_down": 4}


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


def time_kind(kind, B, HW, C, dev):
    g = torch.Generator(device=dev).manual_seed(B * 1000 + HW + C)
    rnd = lambda *s: torch.randn(*s, device=dev, generator=g)
    side = int(HW ** 0.5)
    sets = []
    for _ in range(SETS):
        y, yd = rnd(B, HW, C) * 1.5 + 0.3, (rnd(B, HW, C) * 0.7 - 0.2 if kind == "add_down" else None)
        st = lambda t: (t.mean(1), (t.var(1, unbiased=False) + 1e-5).rsqrt())
        s = dict(g=rnd(B, HW, C) * 1e-5, y=y, stats=st(y))
        nchw = lambda t: t.view(B, side, side, C).permute(0, 3, 1, 2).requires_grad_(True)       # channels_last, no copy
        ty = nchw(y)
        if kind == "relu":
            out, wrt = torch.relu(F.instance_norm(ty)), [ty]
        elif kind == "add":
            tid = nchw(rnd(B, HW, C).relu_())
            out, wrt = torch.relu(F.instance_norm(ty) + tid), [ty, tid]
        else:
            tyd = nchw(yd)
            out, wrt = torch.relu(F.instance_norm(ty) + F.instance_norm(tyd)), [ty, tyd]
            s.update(down=(yd, st(yd)))
        if kind != "relu":
            s["out"] = out.detach().permute(0, 2, 3, 1).reshape(B, HW, C).contiguous()
        s.update(t_out=out, t_wrt=wrt, t_g=s["g"].view(B, side, side, C).permute(0, 3, 1, 2))
        sets.append(s)
    need = ops._native.lib().dsmil_norm_bwd_workspace_bytes(ops.NORM_BWD_KINDS[kind], B, HW, C)
    ws = torch.empty(need, dtype=torch.uint8, device=dev)

    def native(i):
        s = sets[i]
        return ops.norm_backward(kind, s["g"], s["y"], s["stats"], out=s.get("out"), down=s.get("down"), ws=ws)

    def torch_fn(i):
        s = sets[i]
        return torch.autograd.grad(s["t_out"], s["t_wrt"], s["t_g"], retain_graph=True)

    tn, tt = median_ms(native, SETS), median_ms(torch_fn, SETS)
    nbytes = 4.0 * (MAPS_MOVED[kind] * B * HW * C + STATS_MOVED[kind] * B * C)
    return {"native_ms": tn, "torch_ms": tt, "bytes_moved": nbytes, "native_bytes_per_s": nbytes / (tn * 1e-3),
            "native_frac_of_copy_ceiling": nbytes / (tn * 1e-3) / COPY_CEILING, "torch_bytes_per_s": nbytes / (tt * 1e-3),
            "ratio_native_over_torch": tn / tt, "plan": ops.norm_backward_plan(kind, B, HW, C)}


def time_step(B, dev, mode):
    torch.manual_seed(0)
    model = resnet18(norm_layer=torch.nn.InstanceNorm2d)
    model.fc = torch.nn.Identity()
    model = model.to(dev).train()
    x = torch.rand(B, 3, 224, 224, device=dev)
    if mode == "native":
        assert simclr.use_native_blocks(model) == 8 and simclr.use_native_convs(model) == 20
    elif mode == "torch_channels_last":
        model = model.to(memory_format=torch.channels_last)
        x = x.contiguous(memory_format=torch.channels_last)
    params = list(model.parameters())

    def step(_):
        for p in params:
            p.grad = None
        model(x).square().mean().backward()

    step(0)
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    ms = median_ms(step, 1, warmup=3, runs=10)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated()
    return {"step_ms": ms, "peak_bytes": peak, "resident_before_bytes": base}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles", "norm_bwd"))
    ap.add_argument("--batches", type=int, nargs="*", default=[64, 256])
    ap.add_argument("--skip-step", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("norm_bwd_time.py measures on the GPU; none is visible")
    dev = "cuda:0"
    os.makedirs(args.out_dir, exist_ok=True)
    out = {"device": torch.cuda.get_device_name(0), "method": __doc__.split("\n\n")[1], "copy_ceiling_bytes_per_s": COPY_CEILING,
           "batches": {}}
    for B in args.batches:
        per = {}
        for HW, C in SHAPES:
            for kind in ("relu", "add", "add_down"):
                r = time_kind(kind, B, HW, C, dev)
                per[f"{kind} {int(HW ** 0.5)}^2x{C}"] = r
                torch.cuda.empty_cache()
                print(B, kind, HW, C, json.dumps({k: v for k, v in r.items() if k != "plan"}), flush=True)
        tot = {s: sum(v[s] for v in per.values()) for s in ("native_ms", "torch_ms")}
        out["batches"][str(B)] = {"calls": per, "sum_over_the_12_calls_ms": tot}
    with open(os.path.join(args.out_dir, "times.json"), "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", os.path.join(args.out_dir, "times.json"))
    if args.skip_step:
        return
    step = {"device": out["device"], "method": __doc__.split("\n\n")[2], "input": 224, "batches": {}}
    for B in args.batches:
        res = {}
        for mode in ("torch_nchw", "torch_channels_last", "native"):
            res[mode] = time_step(B, dev, mode)
            torch.cuda.empty_cache()
            print(B, mode, json.dumps(res[mode]), flush=True)
        res["ratio_native_over_torch_nchw"] = res["native"]["step_ms"] / res["torch_nchw"]["step_ms"]
        res["peak_ratio_native_over_torch_nchw"] = res["native"]["peak_bytes"] / res["torch_nchw"]["peak_bytes"]
        step["batches"][str(B)] = res
    with open(os.path.join(args.out_dir, "step.json"), "w") as f:
        json.dump(step, f, indent=1)
    print("wrote", os.path.join(args.out_dir, "step.json"))


if __name__ == "__main__":
    main()
