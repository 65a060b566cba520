"""Times the native conv backward (csrc/conv_bwd.hip: ops.conv_backward_weight / conv_backward_data) on the 20 convs of the
ResNet-18 trunk at 224 x 224, batch 64 and 256, against torch.ops.aten.convolution_backward on the SAME tensors (the NHWC
buffers seen as channels_last NCHW) in the same run.  Per conv and direction: hipEvents around one call, 5 warm-up runs, the
median of 25 timed runs, 8 distinct input sets in rotation (no run re-reads the inputs of the run before it); algorithmic
TFLOP/s = 2 B Ho Wo Cout Cin ks^2 / time; ratio = native time / torch time (above 1: the native call loses).  Convs of one shape
are measured once and listed under every name.

    python tools/conv_bwd_time.py [--out profiles/conv_bwd/times.json] [--batches 64 256]
    python tools/conv_bwd_time.py --model-grad [--out profiles/conv_bwd/model_grad.json]
        the model-level check of tests/test_conv_bwd_gpu.py: per conv the norm-wise relative error of the weight gradient of
        the native run and of the fp32 CPU yardstick against the fp64 CPU model, and their ratio
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import dsmil  # noqa: E402,F401
from dsmil_wsi_amd import ops  # noqa: E402

SETS, WARMUP, RUNS = 8, 5, 25


def resnet18_convs(size=224):
    """[(name, Cin, Cout, ks, stride, pad, H, W)] in state_dict order."""
    out = [("conv1", 3, 64, 7, 2, 3, size, size)]
    hw, cin = size // 4, 64
    for li, planes in enumerate((64, 128, 256, 512), 1):
        stride = 1 if li == 1 else 2
        for b in range(2):
            s = stride if b == 0 else 1
            out.append((f"layer{li}.{b}.conv1", cin, planes, 3, s, 1, hw, hw))
            out.append((f"layer{li}.{b}.conv2", planes, planes, 3, 1, 1, hw // s, hw // s))
            if b == 0 and s == 2:
                out.append((f"layer{li}.0.downsample.0", cin, planes, 1, 2, 0, hw, hw))
            hw, cin = hw // s, planes
    return out


def median_ms(fn, n_sets):
    times = []
    for i in range(WARMUP + RUNS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn(i % n_sets)
        e1.record()
        e1.synchronize()
        if i >= WARMUP:
            times.append(e0.elapsed_time(e1))
    times.sort()
    return times[len(times) // 2]


def time_shape(B, Cin, Cout, ks, stride, pad, H, W, dev):
    Ho, Wo = (H + 2 * pad - ks) // stride + 1, (W + 2 * pad - ks) // stride + 1
    g = torch.Generator(device=dev).manual_seed(Cin * 1000 + Cout + ks + H)
    xs = [torch.randn(B, H, W, Cin, device=dev, generator=g).relu_() for _ in range(SETS)]
    dys = [torch.randn(B, Ho, Wo, Cout, device=dev, generator=g) * 1e-5 for _ in range(SETS)]
    w = torch.randn(Cout, Cin, ks, ks, device=dev, generator=g) * (2.0 / (Cout * ks * ks)) ** 0.5
    w_cl = w.contiguous(memory_format=torch.channels_last)
    flop = 2.0 * B * Ho * Wo * Cout * Cin * ks * ks
    res = {"flop": flop}

    def aten(i, mask):
        return torch.ops.aten.convolution_backward(dys[i].permute(0, 3, 1, 2), xs[i].permute(0, 3, 1, 2), w_cl, None, [stride, stride],
                                                   [pad, pad], [1, 1], False, [0, 0], 1, mask)

    legs = [("weight", lambda i: ops.conv_backward_weight(xs[i], dys[i], ks, stride, pad), lambda i: aten(i, [False, True, False]))]
    if Cin != 3:
        legs.append(("data", lambda i: ops.conv_backward_data(dys[i], w, H, W, stride, pad), lambda i: aten(i, [True, False, False])))
    for which, native, torch_fn in legs:
        tn, tt = median_ms(native, SETS), median_ms(torch_fn, SETS)
        res[which] = {"native_ms": tn, "torch_ms": tt, "native_tflops": flop / tn * 1e-9, "torch_tflops": flop / tt * 1e-9,
                      "ratio_native_over_torch": tn / tt}
    return res


def model_grad(out_path):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import conv_bwd_cases as cc
    g64 = cc.model_weight_grads(torch.float64)
    yard = cc.rel_errors(cc.model_weight_grads(torch.float32), g64)
    nat = cc.rel_errors(cc.model_weight_grads(torch.float32, device="cuda", native=True), g64)
    names = [c[0] for c in resnet18_convs()]
    out = {"device": torch.cuda.get_device_name(0), "seed": cc.MODEL_SEED, "batch": cc.MODEL_B, "input": cc.MODEL_HW,
           "margin": cc.MODEL_MARGIN, "quantity": "||g - g64|| / ||g64|| per conv weight gradient",
           "convs": {n: {"native": a, "yardstick_fp32_cpu": b, "ratio": a / b} for n, a, b in zip(names, nat, yard)}}
    out["max_ratio"] = max(v["ratio"] for v in out["convs"].values())
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out["convs"], indent=1))
    print("max ratio", out["max_ratio"], "wrote", out_path)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--batches", type=int, nargs="*", default=[64, 256])
    ap.add_argument("--model-grad", action="store_true")
    args = ap.parse_args()
    if args.model_grad:
        return model_grad(args.out or os.path.join(ROOT, "profiles", "conv_bwd", "model_grad.json"))
    out_path = args.out or os.path.join(ROOT, "profiles", "conv_bwd", "times.json")
    dev = "cuda:0"
    out = {"device": torch.cuda.get_device_name(0), "method": __doc__.split("\n\n")[0], "input": 224, "batches": {}}
    for B in args.batches:
        done, per = {}, {}
        for name, Cin, Cout, ks, stride, pad, H, W in resnet18_convs():
            key = (Cin, Cout, ks, stride, pad, H, W)
            if key not in done:
                done[key] = time_shape(B, Cin, Cout, ks, stride, pad, H, W, dev)
                torch.cuda.empty_cache()
            per[name] = dict(done[key], shape={"Cin": Cin, "Cout": Cout, "ks": ks, "stride": stride, "pad": pad, "H": H, "W": W})
            print(B, name, json.dumps({k: v for k, v in done[key].items() if k != "flop"}), flush=True)
        tot = {w: {s: sum(v[w][s] for v in per.values() if w in v) for s in ("native_ms", "torch_ms")} for w in ("weight", "data")}
        out["batches"][str(B)] = {"convs": per, "sum_over_the_20_convs_ms": tot}
        print(B, "sum", json.dumps(tot), flush=True)
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", out_path)


if __name__ == "__main__":
    main()
