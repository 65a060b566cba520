#!/usr/bin/env python
"""Checks that a change of the embedder's HOST code (csrc/resnet_fwd.hip: plan_conv / plan_stem and the launches that read
them) left sizes, launches, bits and time alone.  The library under test is the one DSMIL_NATIVE_LIB names (a file next to
dsmil-wsi_amd/_native.py), as everywhere.

    python tools/embed_plan_check.py sizes                      record tests/golden/resnet_sizes.json (CPU)
    python tools/embed_plan_check.py bits --out F.npz           the feature rows of the cases below (GPU); from the parent build
        they are the fixture of a bit-identity test of the launch plan and summation order
    python tools/embed_plan_check.py launches --out A.json      ordered (kernel, grid, workgroup, LDS bytes) of one forward per case
        below plus depth 18 at B=256, 224x224: one fresh process per case under
        `rocprofv3 --kernel-trace --stats` (no counters)
    python tools/embed_plan_check.py compare A.json B.json --out profiles/embed_plan/launches.json
    python tools/embed_plan_check.py time --libs libA.so libB.so --runs 5 --out profiles/embed_plan/times.json
        alternating fresh processes: ms per forward of bench.py's embedder batch (B=256, 224x224) and of a launch-bound call
        (B=1, 32x32), and the SHA-256 of the features of bench.py's first embedder batch
"""
import argparse
import csv
import glob
import hashlib
import json
import os
import re
import statistics
import subprocess
import sys
import tempfile
import time

import ctypes

import numpy as np

import _path  # noqa: F401
import dsmil  # noqa: F401  (registers the dsmil_wsi_amd package)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
# The smallest shapes that still take every plan kind of the product library:
#   depth 18 InstanceNorm, B=3, 64x70, fp32 and u8 input: fused stem, the two-wave unit on layer 1, w1 on layers 2-4, direct
#       tiles 42 / 22 / 24
#   depth 18 frozen BatchNorm, B=2, 33x47: unfused stem, fill_stats
#   depth 50 InstanceNorm, B=2, 64x64: Bottleneck blocks, 1x1 convs up to 2048 channels
#   depth 18, precision 1, 2 and 3, B=3, 64x70: the one-plane form and the bf16 / fp16 activation trunks
# Weights and images come from numpy's seeded PCG64 on the CPU.
#        name           depth B  H   W   u8     bn     precision
CASES = [("d18_in_f32", 18, 3, 64, 70, False, False, 0),
         ("d18_in_u8", 18, 3, 64, 70, True, False, 0),
         ("d18_bn", 18, 2, 33, 47, False, True, 0),
         ("d50_in", 50, 2, 64, 64, False, False, 0),
         ("d18_p1", 18, 3, 64, 70, False, False, 1),
         ("d18_p2", 18, 3, 64, 70, False, False, 2),
         ("d18_p3", 18, 3, 64, 70, False, False, 3)]


def make_inputs(depth, B, H, W, u8, bn):
    """(conv weights, images, bn_m, bn_r) as numpy arrays: kaiming-normal(fan_out) weights, images in [0, 1) (or their uint8
    NHWC rounding), and for the frozen-BatchNorm case per-channel (m, r) with r of either sign."""
    from dsmil_wsi_amd.ops import resnet_conv_shapes
    rng = np.random.default_rng(1000 + depth)
    convs = [(rng.standard_normal(s, dtype=np.float32) * np.float32((2.0 / (s[0] * s[2] * s[3])) ** 0.5)) for s in resnet_conv_shapes(depth)]
    x = np.random.default_rng(7 * B + H + W).random((B, 3, H, W), dtype=np.float32)
    if u8:
        x = np.ascontiguousarray(np.rint(x * 255).astype(np.uint8).transpose(0, 2, 3, 1))
    bn_m = bn_r = None
    if bn:
        n = sum(s[0] for s in resnet_conv_shapes(depth))
        r2 = np.random.default_rng(5)
        bn_m = (r2.standard_normal(n) * 0.1).astype(np.float32)
        bn_r = (r2.uniform(0.6, 1.0, n) * np.where(r2.random(n) < 0.1, -1.0, 1.0)).astype(np.float32)
    return convs, x, bn_m, bn_r


def run_case(depth, B, H, W, u8, bn, precision):
    """One dsmil_resnet_forward_ex on the inputs of make_inputs; the feature rows as a numpy array."""
    import torch
    import dsmil_wsi_amd._native as nat
    from dsmil_wsi_amd import ops
    L = nat.lib()
    dev = torch.device("cuda:0")
    convs, x, bn_m, bn_r = make_inputs(depth, B, H, W, u8, bn)
    convs = [torch.from_numpy(w).to(dev) for w in convs]
    x = torch.from_numpy(x).to(dev)
    bn_m = torch.from_numpy(bn_m).to(dev) if bn else None
    bn_r = torch.from_numpy(bn_r).to(dev) if bn else None
    packed = ops._packed_resnet_weights(convs, depth, precision)
    nbytes = L.dsmil_resnet_workspace_bytes(depth, B, H, W)
    assert nbytes > 0
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    feats = torch.full((B, L.dsmil_resnet_feature_dim(depth)), float("nan"), dtype=torch.float32, device=dev)
    p = ops._ptr
    rc = L.dsmil_resnet_forward_ex(depth, p(x), 1 if u8 else 0, B, H, W, p(convs[0]), p(packed), p(bn_m), p(bn_r), p(None), p(None),
                                   0, p(feats), p(None), p(ws), ctypes.c_size_t(nbytes), precision, ops._stream(dev))
    nat.check(rc, "dsmil_resnet_forward_ex")
    torch.cuda.synchronize()
    return feats.cpu().numpy()
BIG = ("d18_in_b256", 18, 256, 224, 224, False, False, 0)


def cases():
    return list(CASES) + [BIG]


def trace_case(name, timeout):
    with tempfile.TemporaryDirectory() as d:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "-f", "csv", "-d", d, "--", sys.executable, os.path.abspath(__file__),
               "case", name]
        subprocess.run(cmd, check=True, timeout=timeout, stdout=subprocess.DEVNULL)
        rows = []
        for f in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
            rows += list(csv.DictReader(open(f)))
    rows.sort(key=lambda r: int(r.get("Dispatch_Id") or r.get("Start_Timestamp")))
    out = []
    for r in rows:
        m = re.search(r"(?:^|[\s:])(k_[a-z0-9_]+(?:<.*>)?)", r["Kernel_Name"])
        if not m:
            continue   # the framework's own kernels (tensor fills, casts)
        dims = lambda stem: [int(r[k]) for k in (stem + "_X", stem + "_Y", stem + "_Z") if k in r] or [int(r[stem])]  # noqa: E731
        out.append({"kernel": re.sub(r"\(.*$", "", m.group(1)), "grid": dims("Grid_Size"), "workgroup": dims("Workgroup_Size"),
                    "lds": int(r.get("LDS_Block_Size", r.get("LDS_Block_Size_v", 0)))})
    return out


def time_one():
    """In a fresh process: the figures of one run as a JSON line."""
    import torch
    import torch.nn as nn
    import dsmil
    from dsmil_wsi_amd.resnet import resnet18
    from dsmil_wsi_amd.synthetic import make_resnet18_weights
    res = resnet18(norm_layer=nn.InstanceNorm2d)
    res.fc = nn.Identity()
    res.load_state_dict(make_resnet18_weights(seed=11), strict=True)
    ic = dsmil.IClassifier(res, 512, output_class=2).eval().cuda()
    g = torch.Generator(device="cuda").manual_seed(7)
    x = torch.rand((256, 3, 224, 224), generator=g, device="cuda", dtype=torch.float32)   # bench.py's first embedder batch
    xs = torch.rand((1, 3, 32, 32), generator=g, device="cuda", dtype=torch.float32)
    res = {}
    with torch.no_grad():
        f, _ = ic(x)
        res["bench_feats_sha256"] = hashlib.sha256(f.cpu().numpy().tobytes()).hexdigest()
        for key, inp, warm, n in (("ms_b256_224", x, 3, 20), ("ms_b1_32", xs, 50, 1000)):
            for _ in range(warm):
                ic(inp)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(n):
                ic(inp)
            torch.cuda.synchronize()
            res[key] = (time.perf_counter() - t0) / n * 1e3
    print("TIME " + json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=("sizes", "bits", "launches", "case", "compare", "time", "time-one"))
    ap.add_argument("args", nargs="*")
    ap.add_argument("--out")
    ap.add_argument("--libs", nargs=2)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--timeout", type=int, default=150, help="seconds per child process")
    a = ap.parse_args()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    if a.mode == "sizes":
        import dsmil  # noqa: F401
        import test_resnet_sizes_cabi as t
        json.dump(t.query(), open(a.out or t.GOLDEN, "w"), indent=0, sort_keys=True)
    elif a.mode == "bits":
        rows = {c[0]: run_case(*c[1:]) for c in CASES}
        assert all(np.isfinite(v).all() for v in rows.values())
        np.savez_compressed(a.out, **rows)
    elif a.mode == "case":
        run_case(*[c for c in cases() if c[0] == a.args[0]][0][1:])
    elif a.mode == "time-one":
        time_one()
    elif a.mode == "launches":
        res = {}
        for c in cases():   # a case that fails ends the run: nothing more is started on the device
            res[c[0]] = trace_case(c[0], a.timeout)
            print(c[0], len(res[c[0]]), "launches", flush=True)
        json.dump(res, open(a.out, "w"), indent=1)
    elif a.mode == "compare":
        A, B = (json.load(open(f)) for f in a.args)
        res = {"a": a.args[0], "b": a.args[1], "cases": {}}
        for name in A:
            res["cases"][name] = {"equal": A[name] == B.get(name), "launches": A[name]}
            if A[name] != B.get(name):
                res["cases"][name]["launches_b"] = B.get(name)
        res["all_equal"] = set(A) == set(B) and all(c["equal"] and c["launches"] for c in res["cases"].values())
        json.dump(res, open(a.out, "w"), indent=1)
        print("all_equal:", res["all_equal"])
        return 0 if res["all_equal"] else 1
    elif a.mode == "time":
        runs = {lib: [] for lib in a.libs}
        for i in range(a.runs):
            for lib in a.libs:   # alternating; a child that fails ends the run
                e = dict(os.environ, DSMIL_NATIVE_LIB=lib)
                r = subprocess.run([sys.executable, os.path.abspath(__file__), "time-one"], env=e, capture_output=True, text=True,
                                   timeout=a.timeout)
                if r.returncode != 0:
                    print(r.stdout[-2000:], r.stderr[-4000:])
                    return 1
                runs[lib].append(json.loads([l for l in r.stdout.splitlines() if l.startswith("TIME ")][0][5:]))
                print(i, lib, runs[lib][-1], flush=True)
        res = {"libs": a.libs, "runs": runs, "summary": {}}
        base, new = a.libs
        for k in ("ms_b256_224", "ms_b1_32"):
            b, n = [r[k] for r in runs[base]], [r[k] for r in runs[new]]
            res["summary"][k] = {"base_min": min(b), "base_max": max(b), "base_median": statistics.median(b),
                                 "new_median": statistics.median(n), "new_median_within_base_range": min(b) <= statistics.median(n) <= max(b),
                                 "new_median_not_slower_than_base_max": statistics.median(n) <= max(b)}
        res["summary"]["bench_feats_bit_identical"] = len({r["bench_feats_sha256"] for rs in runs.values() for r in rs}) == 1
        json.dump(res, open(a.out, "w"), indent=1)
        print(json.dumps(res["summary"], indent=1))
    return 0


if __name__ == "__main__":
    sys.exit(main())
