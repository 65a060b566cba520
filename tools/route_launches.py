#!/usr/bin/env python
"""Which kernels the aggregator forward launches, call by call: the ordered list of (kernel, grid, workgroup, LDS bytes) for a
handful of calls that between them take every route of tests/test_route_cabi.py — to compare two builds of the library
(a change of the host code that claims "same launches" shows two equal lists).

    python tools/route_launches.py --lib dsmil-wsi_amd/libdsmil_hip.so --out /tmp/launches_new.json
        one fresh process per case under `rocprofv3 --kernel-trace --stats` (no counters), through the C-ABI only, so that
        an older build of the library (one without dsmil_agg_forward_route) runs under the same script
    python tools/route_launches.py --compare A.json B.json --out profiles/route_refactor/launches.json
    python tools/route_launches.py --lib ... --case NAME        (what the driver runs under the profiler)
"""
import argparse
import csv
import ctypes
import glob
import itertools
import json
import os
import re
import subprocess
import sys
import tempfile

import _path  # noqa: F401

CASES = ("f3_uniform", "f3_ragged_caller_images", "f2_c3", "f2_batch_form1", "split128_batch_form0", "split128_vals", "k166_batch",
         "hs_inline", "hs_inline_rowmap", "hs_qmax_launch", "hs_no_inline_knob", "given_classes", "k166_lone", "bf16_res",
         "bf16_res_ragged_pipe", "bf16_dma_k1024", "bf16_ring", "shard_two_phases")
RENAMED = {"k_set_offsets2": "k_set_offsets"}   # the same one-thread kernel, once per translation unit before


def run_case(lib_path, name):
    import torch
    import dsmil  # noqa: F401
    import dsmil_wsi_amd._native as nat
    L = ctypes.CDLL(os.path.abspath(lib_path))
    for sym, (res, args) in nat.SIGNATURES.items():
        if hasattr(L, sym):
            getattr(L, sym).restype, getattr(L, sym).argtypes = res, args
    dev = torch.device("cuda:0")
    g = torch.Generator(device="cpu").manual_seed(5)

    def rnd(*shape, scale=1.0):
        return (torch.randn(*shape, generator=g) * scale).to(dev)

    def ptr(t):
        return None if t is None else ctypes.c_void_p(t.data_ptr())

    def forward(lengths, K=512, Kv=None, C=2, nonlinear=1, bf16=False, given=False, rowmap=False, images=False, phase=0):
        Kv = K if Kv is None else Kv
        total, nb = sum(lengths), len(lengths)
        feats = rnd(total, K)
        vals = feats if Kv == K else rnd(total, Kv)
        w = dict(fc_w=rnd(C, K, scale=0.05), fc_b=rnd(C), q0_w=rnd(128, K, scale=0.05), q0_b=rnd(128), q2_w=rnd(128, 128, scale=0.1),
                 q2_b=rnd(128), fcc_w=rnd(C, C, Kv, scale=0.05), fcc_b=rnd(C))
        p = nat.AggParams(*[w[k].data_ptr() for k in ("fc_w", "fc_b", "q0_w", "q0_b", "q2_w", "q2_b", "fcc_w", "fcc_b")], K, Kv, C,
                          nonlinear)
        off = torch.tensor([0] + list(itertools.accumulate(lengths)), dtype=torch.int64, device=dev)
        classes = rnd(total, C) if given else torch.empty(total, C, device=dev)
        A, B = torch.empty(total, C, device=dev), torch.empty(nb, C, Kv, device=dev)
        pred, idx = torch.empty(nb, C, device=dev), torch.empty(nb, C, dtype=torch.int64, device=dev)
        ws = torch.empty(L.dsmil_agg_workspace_bytes(nb, total, K, Kv, C) + 256, dtype=torch.uint8, device=dev)
        wsp = ctypes.c_void_p((ws.data_ptr() + 255) // 256 * 256)
        st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        q2 = ptr(w["q2_w"]) if nonlinear else None
        if phase:
            best, crit, ml = torch.empty(C, device=dev), rnd(C, K), torch.empty(C, 2, device=dev)
            rc = L.dsmil_agg_shard_argmax(ptr(feats), total, ctypes.byref(p), ptr(classes), ptr(best), ptr(idx), wsp, ws.numel() - 256, st)
            assert rc == 0, rc
            rc = L.dsmil_agg_shard_attend(ptr(feats), None, total, ctypes.byref(p), ptr(crit), ptr(A), ptr(ml), ptr(B), wsp,
                                          ws.numel() - 256, st)
        elif bf16:
            packed = torch.empty(L.dsmil_agg_packed_bf16_bytes(K), dtype=torch.uint8, device=dev)
            assert L.dsmil_agg_pack_bf16(ptr(w["q0_w"]), q2, K, ptr(packed), st) == 0
            fb = feats.to(torch.bfloat16)
            rc = L.dsmil_agg_forward_bf16(ptr(fb), ptr(fb if Kv == K else vals.to(torch.bfloat16)), ptr(off), nb, total, max(lengths),
                                          ctypes.byref(p), ptr(packed), None, ptr(classes), ptr(A), ptr(B), ptr(pred), ptr(idx), wsp,
                                          ws.numel() - 256, st)
        else:
            keep = []
            opts = nat.AggOpts(0, 0, 0)
            if images:
                sp = torch.empty(L.dsmil_agg_packed_split_bytes(K, nonlinear), dtype=torch.uint8, device=dev)
                f2 = torch.empty(L.dsmil_agg_packed_f2_bytes(K), dtype=torch.uint8, device=dev)
                assert L.dsmil_agg_pack_split(ptr(w["q0_w"]), q2, K, ptr(sp), st) == 0
                assert L.dsmil_agg_pack_f2(ptr(w["q0_w"]), q2, K, ptr(f2), st) == 0
                opts.packed_split, opts.packed_f2 = sp.data_ptr(), f2.data_ptr()
                keep += [sp, f2]
            if rowmap:
                rm = torch.randperm(total, generator=g).to(dev)
                opts.row_map = rm.data_ptr()
                keep.append(rm)
            rc = L.dsmil_agg_forward_ex(ptr(feats), ptr(vals if Kv != K else None), ptr(off), nb, total, max(lengths), ctypes.byref(p),
                                        ctypes.byref(opts), ptr(classes) if given else None, None if given else ptr(classes), ptr(A),
                                        ptr(B), ptr(pred), ptr(idx), wsp, ws.numel() - 256, st)
        assert rc == 0, f"{name}: rc {rc}"
        torch.cuda.synchronize()

    batch = [1024] * 64
    ragged = [700 + 11 * i for i in range(64)] + [20000]
    if name == "f3_uniform": forward(batch)
    elif name == "f3_ragged_caller_images": forward(ragged, images=True)
    elif name == "f2_c3": forward(ragged, K=256, C=3)
    elif name == "f2_batch_form1": L.dsmil_agg_batch_form(1); forward(batch, C=1)
    elif name == "split128_batch_form0": L.dsmil_agg_batch_form(0); forward(ragged, images=True)
    elif name == "split128_vals": forward(batch, Kv=384)
    elif name == "k166_batch": forward(batch, K=166, C=1)
    elif name == "hs_inline": forward([1500])
    elif name == "hs_inline_rowmap": forward([900, 1500, 33], C=5, rowmap=True, images=True)
    elif name == "hs_qmax_launch": forward([5000] * 8)
    elif name == "hs_no_inline_knob": L.dsmil_agg_inline_query(0); forward([1500], nonlinear=0)
    elif name == "given_classes": forward([1500], given=True)
    elif name == "k166_lone": forward([476], K=166, C=1)
    elif name == "bf16_res": forward(batch, bf16=True)
    elif name == "bf16_res_ragged_pipe": L.dsmil_agg_logits_form(2); forward(ragged, bf16=True)
    elif name == "bf16_dma_k1024": forward(ragged, K=1024, bf16=True)
    elif name == "bf16_ring": forward([1500], bf16=True, C=1)
    elif name == "shard_two_phases": forward([3000], phase=1)
    else: raise SystemExit(f"unknown case {name}")


def trace_case(lib_path, name, timeout):
    with tempfile.TemporaryDirectory() as d:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "-f", "csv", "-d", d, "--", sys.executable, os.path.abspath(__file__),
               "--lib", lib_path, "--case", name]
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
        kname = re.sub(r"\(.*$", "", m.group(1))
        out.append({"kernel": RENAMED.get(kname, kname), "grid": dims("Grid_Size"), "workgroup": dims("Workgroup_Size"),
                    "lds": int(r.get("LDS_Block_Size", r.get("LDS_Block_Size_v", 0)))})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "dsmil-wsi_amd", "libdsmil_hip.so"))
    ap.add_argument("--case")
    ap.add_argument("--out")
    ap.add_argument("--timeout", type=int, default=120, help="seconds per traced case")
    ap.add_argument("--compare", nargs=2, metavar=("A.json", "B.json"))
    a = ap.parse_args()
    if a.case:
        return run_case(a.lib, a.case)
    if a.compare:
        A, B = (json.load(open(f)) for f in a.compare)
        res = {"a": a.compare[0], "b": a.compare[1], "renamed": RENAMED, "cases": {}}
        for name in CASES:
            res["cases"][name] = {"equal": A[name] == B[name], "launches": A[name]}
            if A[name] != B[name]:
                res["cases"][name]["launches_b"] = B[name]
        res["all_equal"] = all(c["equal"] and c["launches"] for c in res["cases"].values())
    else:
        res = {}
        for name in CASES:   # a case that fails ends the run: nothing more is started on the device
            res[name] = trace_case(a.lib, name, a.timeout)
            print(name, len(res[name]), "launches", flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        json.dump(res, open(a.out, "w"), indent=1)
    if a.compare:
        print("all_equal:", res["all_equal"])
        return 0 if res["all_equal"] else 1


if __name__ == "__main__":
    sys.exit(main())
