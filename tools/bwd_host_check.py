#!/usr/bin/env python
"""One-off checks that a change of the aggregator backward's HOST code (csrc/agg_bwd.hip, csrc/agg_bwd_bags.h) left sizes,
bits, launches and time alone: two builds of the library, the parent commit's and the new one, driven through the C-ABI only.

    python tools/bwd_host_check.py sizes                         record tests/golden/bwd_sizes.json (CPU; the library
                                                                 DSMIL_NATIVE_LIB names, as everywhere)
    python tools/bwd_host_check.py bits --lib L.so --dump DIR    every case below in ONE process: identical inputs from a
        fixed seed, the workspace and every output filled with a NaN pattern before each call; every output tensor (the
        step entries: the updated parameters, exp_avg, exp_avg_sq and the losses after three steps) as DIR/<case>/<t>.npy.
        The process ends at the first non-zero return code or HIP error and starts nothing after it.
    python tools/bwd_host_check.py compare-bits DIR_A DIR_B --out profiles/bwd_host/bits.json     byte equality per tensor
    python tools/bwd_host_check.py launches --lib L.so --out A.json
        one fresh process per case under `rocprofv3 --kernel-trace --stats` (no counters): the ordered list of
        (kernel, grid, workgroup, LDS bytes) of the library's kernels
    python tools/bwd_host_check.py compare-launches A.json B.json --out profiles/bwd_host/launches.json
    python tools/bwd_host_check.py time --names libdsmil_hip_parent.so libdsmil_hip.so --repeats 3 --out profiles/bwd_host/times.json
        bench.py --full --workload train and tools/bwd_bags_time.py --train-only (fp32, bf16), alternating between the two
        libraries (file names next to dsmil-wsi_amd/_native.py); the new library's median against the parent's min-max
    python tools/bwd_host_check.py case --lib L.so --case NAME   (what `launches` runs under the profiler)
"""
import argparse
import csv
import ctypes
import glob
import hashlib
import itertools
import json
import os
import re
import statistics
import subprocess
import sys
import tempfile

import _path  # noqa: F401

QD = 128
SMALL, BIG = (33, 900, 1), (40000, 25000, 600)


def _cases():
    """name -> (kind, keyword arguments): the smallest shapes that reach each branch of the host code."""
    c = {}
    for nl in (1, 0):
        c[f"backward_n33_k64_kv96_c5_{'nonlinear' if nl else 'linear'}"] = ("backward", dict(
            entry="dsmil_agg_backward", lengths=(33,), K=64, Kv=96, C=5, nonlinear=nl, g_classes=True, g_A=True, g_B=True, g_vals=True))
    c["ex_n65_k64_c1_gmax_rowmap"] = ("backward", dict(entry="dsmil_agg_backward_ex", lengths=(65,), K=64, C=1, g_max=True, rowmap=True))
    for n in (1, 1500):
        c[f"rows_n{n}_k512_c2_gfeats"] = ("backward", dict(entry="dsmil_agg_backward_rows", lengths=(n,), K=512, C=2, g_max=True, g_feats=True))
    c["rows_n476_k166_c1"] = ("backward", dict(entry="dsmil_agg_backward_rows", lengths=(476,), K=166, C=1, g_max=True, g_feats=True))
    c["rows_n65536_k64_aligned"] = ("backward", dict(entry="dsmil_agg_backward_rows", lengths=(65536,), K=64, C=2, g_max=True, g_feats=True))
    c["rows_n65536_k64_base_plus_4_bytes"] = ("backward", dict(entry="dsmil_agg_backward_rows", lengths=(65536,), K=64, C=2, g_max=True,
                                                                g_feats=True, misalign=1))
    c["bags_small_k64_c5_all"] = ("backward", dict(entry="dsmil_agg_backward_bags", lengths=SMALL, K=64, C=5, g_classes=True, g_max=True,
                                                   g_vals=True, g_feats=True, rowmap=True))
    c["bags_big_k64_four_wave"] = ("backward", dict(entry="dsmil_agg_backward_bags", lengths=BIG, K=64, C=2, g_max=True, g_vals=True, g_feats=True))
    c["bags_big_k166_one_wave_slots"] = ("backward", dict(entry="dsmil_agg_backward_bags", lengths=BIG, K=166, C=2, g_max=True, g_vals=True,
                                                         g_feats=True))
    c["bags_one_bag"] = ("backward", dict(entry="dsmil_agg_backward_bags", lengths=(900,), K=64, C=2, g_max=True, g_feats=True))
    for tag, lengths in (("small", SMALL), ("big", BIG)):
        c[f"bags_bf16_{tag}_k64"] = ("backward", dict(entry="dsmil_agg_backward_bags_bf16", lengths=lengths, K=64, C=2, g_max=True, g_vals=True))
        c[f"bags_bf16_{tag}_k64_vals"] = ("backward", dict(entry="dsmil_agg_backward_bags_bf16", lengths=lengths, K=64, Kv=64, C=2, g_max=True,
                                                          g_vals=True, separate_vals=True))
    c["loss_head_bags"] = ("loss_head", dict(weighted=False))
    c["loss_head_bags_w"] = ("loss_head", dict(weighted=True))
    c["adam_step_eight_tensors_one_empty"] = ("adam", {})
    c["step_n1500_k512_c2_ga_in_prep"] = ("step", dict(N=1500, K=512, C=2))            # C K <= FC_ROLE_MAX; the forward carries the prologue
    c["step_n1500_k512_c5_ga_own_launch"] = ("step", dict(N=1500, K=512, C=5))
    c["step_n476_k166_c1_own_prologue"] = ("step", dict(N=476, K=166, C=1))            # the forward cannot carry the prologue
    c["step_n1500_k512_c2_rowmap"] = ("step", dict(N=1500, K=512, C=2, rowmap=True))
    c["step_n1500_k512_c2_linear"] = ("step", dict(N=1500, K=512, C=2, nonlinear=0))
    for e in ("dsmil_agg_train_step_bags", "dsmil_agg_train_step_bags_w", "dsmil_agg_train_step_bags_bf16", "dsmil_agg_train_step_bags_bf16_w"):
        c[e.replace("dsmil_agg_train_", "")] = ("step_bags", dict(entry=e))
    return c


CASES = _cases()


class Driver:
    """One library, one device, one seed per case."""

    def __init__(self, lib_path, dump=None):
        import torch
        import dsmil  # noqa: F401  (registers the dsmil_wsi_amd package)
        import dsmil_wsi_amd._native as nat
        self.torch, self.nat, self.dump_dir = torch, nat, dump
        self.L = ctypes.CDLL(os.path.abspath(lib_path))
        for sym, (res, args) in nat.SIGNATURES.items():
            if hasattr(self.L, sym):
                getattr(self.L, sym).restype, getattr(self.L, sym).argtypes = res, args
        self.dev = torch.device("cuda:0")
        self.st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    # ---- inputs and outputs
    def seed(self, name):
        self.g = self.torch.Generator(device="cpu").manual_seed(int(hashlib.sha256(name.encode()).hexdigest()[:8], 16))
        self.case, self.keep = name, []

    def rnd(self, *shape, scale=1.0):
        return (self.torch.randn(*shape, generator=self.g) * scale).to(self.dev)

    def uni(self, *shape):
        return self.torch.rand(*shape, generator=self.g).to(self.dev)

    def nan(self, *shape):
        return self.torch.full(shape, float("nan"), device=self.dev)

    def workspace(self, nbytes):
        assert nbytes > 0
        ws = self.torch.full((nbytes + 256,), 0xFF, dtype=self.torch.uint8, device=self.dev)   # all ones: a NaN in every float
        self.keep.append(ws)
        return ctypes.c_void_p((ws.data_ptr() + 255) // 256 * 256), nbytes

    @staticmethod
    def ptr(t):
        return None if t is None else ctypes.c_void_p(t.data_ptr())

    def call(self, entry, *args):
        rc = getattr(self.L, entry)(*args)
        if rc != 0:
            raise SystemExit(f"{self.case}: {entry} returned {rc}")
        self.torch.cuda.synchronize()    # a HIP error raises here and ends the process

    def out(self, name, t):
        if self.dump_dir is None or t is None:
            return
        import numpy as np
        d = os.path.join(self.dump_dir, self.case)
        os.makedirs(d, exist_ok=True)
        np.save(os.path.join(d, name + ".npy"), t.detach().cpu().numpy())

    def weights(self, K, Kv, C, nonlinear):
        w = dict(fc_w=self.rnd(C, K, scale=0.05), fc_b=self.rnd(C), q0_w=self.rnd(QD, K, scale=0.05), q0_b=self.rnd(QD),
                 q2_w=self.rnd(QD, QD, scale=0.1), q2_b=self.rnd(QD), fcc_w=self.rnd(C, C, Kv, scale=0.05), fcc_b=self.rnd(C))
        if not nonlinear:
            w["q2_w"] = w["q2_b"] = None
        return w

    def params(self, w, K, Kv, C, nonlinear):
        return self.nat.AggParams(*[(w[k].data_ptr() if w[k] is not None else None) for k in W_KEYS], K, Kv, C, nonlinear)

    # ---- the cases
    def backward(self, entry, lengths, K, C, Kv=None, nonlinear=1, g_classes=False, g_max=False, g_A=False, g_B=False,
                 g_vals=False, g_feats=False, rowmap=False, misalign=0, separate_vals=False):
        torch, ptr = self.torch, self.ptr
        Kv = K if Kv is None else Kv
        T, nb, b16 = sum(lengths), len(lengths), entry.endswith("bf16")
        buf = self.rnd(T * K + 4)
        feats = buf[misalign:misalign + T * K].view(T, K)          # misalign: the base pointer moved by 4 bytes per unit
        vals = self.rnd(T, Kv) if (Kv != K or separate_vals) else None
        if b16:
            feats, vals = feats.to(torch.bfloat16), (vals.to(torch.bfloat16) if vals is not None else None)
        w = self.weights(K, Kv, C, nonlinear)
        p = self.params(w, K, Kv, C, nonlinear)
        A, Bm = self.uni(T, C) / max(lengths), self.rnd(nb, C, Kv)
        idx = torch.stack([torch.randint(0, n, (C,), generator=self.g) for n in lengths]).to(self.dev)
        off = torch.tensor([0] + list(itertools.accumulate(lengths)), dtype=torch.int64, device=self.dev)
        gc = self.rnd(T, C, scale=0.01) if g_classes else None
        gm = self.rnd(nb, C, scale=0.1) if g_max else None
        gp, gA = self.rnd(nb, C, scale=0.1), (self.rnd(T, C, scale=0.01) if g_A else None)
        gB = self.rnd(nb, C, Kv, scale=0.01) if g_B else None
        rm = torch.randperm(T, generator=self.g).to(self.dev) if rowmap else None
        grads = {k: (self.nan(*w[k].shape) if w[k] is not None else None) for k in W_KEYS}
        g = self.nat.AggGrads(*[(grads[k].data_ptr() if grads[k] is not None else None) for k in W_KEYS])
        gv, gf = (self.nan(T, Kv) if g_vals else None), (self.nan(T, K) if g_feats else None)
        head = (ptr(feats), ptr(vals))
        mid = (ctypes.byref(p), ptr(A), ptr(Bm), ptr(idx), ptr(gc))
        if entry == "dsmil_agg_backward":
            ws = self.workspace(self.L.dsmil_agg_backward_workspace_bytes(T, K, Kv, C))
            self.call(entry, *head, T, *mid, ptr(gp), ptr(gA), ptr(gB), ctypes.byref(g), ptr(gv), *ws, self.st)
        elif entry == "dsmil_agg_backward_ex":
            ws = self.workspace(self.L.dsmil_agg_backward_workspace_bytes(T, K, Kv, C))
            self.call(entry, *head, T, *mid, ptr(gm), ptr(gp), ptr(gA), ptr(gB), ctypes.byref(g), ptr(gv), ptr(rm), *ws, self.st)
        elif entry == "dsmil_agg_backward_rows":
            ws = self.workspace(self.L.dsmil_agg_backward_rows_workspace_bytes(T, K, Kv, C))
            self.call(entry, *head, T, *mid, ptr(gm), ptr(gp), ptr(gA), ptr(gB), ctypes.byref(g), ptr(gv), ptr(rm), *ws, self.st, ptr(gf))
        elif entry == "dsmil_agg_backward_bags":
            ws = self.workspace(self.L.dsmil_agg_backward_bags_workspace_bytes(nb, T, K, Kv, C))
            self.call(entry, *head, ptr(off), nb, T, max(lengths), *mid, ptr(gm), ptr(gp), ptr(gA), ptr(gB), ctypes.byref(g), ptr(gv),
                      ptr(rm), *ws, self.st, ptr(gf))
        else:
            ws = self.workspace(self.L.dsmil_agg_backward_bags_bf16_workspace_bytes(nb, T, K, Kv, C))
            self.call(entry, *head, ptr(off), nb, T, max(lengths), *mid, ptr(gm), ptr(gp), ptr(gA), ptr(gB), ctypes.byref(g), ptr(gv),
                      *ws, self.st)
        for k in W_KEYS:
            self.out("g_" + k, grads[k])
        self.out("g_vals", gv)
        self.out("g_feats", gf)

    def loss_head(self, weighted, lengths=SMALL, C=5):
        torch, ptr = self.torch, self.ptr
        T, nb = sum(lengths), len(lengths)
        classes, pred = self.rnd(T, C), self.rnd(nb, C)
        idx = torch.stack([torch.randint(0, n, (C,), generator=self.g) for n in lengths]).to(self.dev)
        off = torch.tensor([0] + list(itertools.accumulate(lengths)), dtype=torch.int64, device=self.dev)
        labels = (self.uni(nb, C) > 0.5).float()
        outs = {k: self.nan(nb, C) for k in ("max_pred", "g_pred", "g_max")}
        outs["loss"] = self.nan(nb)
        args = [ptr(classes), ptr(off), ptr(pred), ptr(idx), ptr(labels), nb, C, ptr(outs["loss"]), ptr(outs["max_pred"]),
                ptr(outs["g_pred"]), ptr(outs["g_max"])]
        if weighted:
            pw, wt = self.uni(C) + 0.5, self.uni(C) + 0.5
            bw = self.nat.BceWeights(pw.data_ptr(), wt.data_ptr())
            self.call("dsmil_agg_loss_head_bags_w", *args, ctypes.byref(bw), self.st)
        else:
            self.call("dsmil_agg_loss_head_bags", *args, self.st)
        for k, t in outs.items():
            self.out(k, t)

    def adam(self):
        numel = [700, 5, 128 * 64, 128, 0, 128, 2 * 2 * 64, 2]
        P = [self.rnd(max(n, 1)) for n in numel]
        G, M = [self.rnd(max(n, 1), scale=0.1) for n in numel], [self.rnd(max(n, 1), scale=0.01) for n in numel]
        V = [self.uni(max(n, 1)) * 1e-3 for n in numel]
        arr = lambda ts: (ctypes.c_void_p * 8)(*[t.data_ptr() for t in ts])   # noqa: E731
        for step in (1, 2, 3):
            self.call("dsmil_adam_step", 8, arr(P), arr(G), arr(M), arr(V), (ctypes.c_int64 * 8)(*numel), step, 1e-4, 0.5, 0.9, 1e-8, 1e-3,
                      self.st)
        for i in range(8):
            self.out(f"param{i}", P[i]); self.out(f"exp_avg{i}", M[i]); self.out(f"exp_avg_sq{i}", V[i])

    def _adam_state(self, w, step):
        nat = self.nat
        m = {k: (self.rnd(*w[k].shape, scale=0.01) if w[k] is not None else None) for k in W_KEYS}
        v = {k: (self.uni(*w[k].shape) * 1e-3 if w[k] is not None else None) for k in W_KEYS}
        arr = lambda d: (ctypes.c_void_p * 8)(*[(d[k].data_ptr() if d[k] is not None else None) for k in W_KEYS])   # noqa: E731
        ma, va = arr(m), arr(v)
        self.keep += [ma, va]
        opt = nat.AdamState(ctypes.cast(ma, ctypes.POINTER(ctypes.c_void_p)), ctypes.cast(va, ctypes.POINTER(ctypes.c_void_p)), step,
                            1e-4, 0.5, 0.9, 1e-8, 1e-3)
        return m, v, opt

    def _step_outputs(self, w, m, v, losses):
        for k in W_KEYS:
            self.out("param_" + k, w[k]); self.out("exp_avg_" + k, m[k]); self.out("exp_avg_sq_" + k, v[k])
        for name, ts in losses.items():
            self.out(name, self.torch.stack(ts))

    def step(self, N, K, C, nonlinear=1, rowmap=False):
        torch, ptr = self.torch, self.ptr
        feats = self.rnd(N, K)
        w = self.weights(K, K, C, nonlinear)
        p = self.params(w, K, K, C, nonlinear)
        m, v, opt = self._adam_state(w, 1)
        label = (self.uni(C) > 0.5).float()
        rm = torch.randperm(N, generator=self.g).to(self.dev) if rowmap else None
        losses = []
        for step in (1, 2, 3):
            opt.step = step
            loss = self.nan(1)
            ws = self.workspace(self.L.dsmil_agg_train_step_workspace_bytes(N, K, C, nonlinear))
            self.call("dsmil_agg_train_step", ptr(feats), N, ptr(rm), ptr(label), ctypes.byref(p), ctypes.byref(opt), ptr(loss), *ws, self.st)
            losses.append(loss)
        self._step_outputs(w, m, v, {"loss": losses})

    def step_bags(self, entry, lengths=SMALL, K=64, C=2):
        torch, ptr = self.torch, self.ptr
        T, nb, b16, weighted = sum(lengths), len(lengths), "bf16" in entry, entry.endswith("_w")
        feats = self.rnd(T, K)
        if b16:
            feats = feats.to(torch.bfloat16)
        w = self.weights(K, K, C, 1)
        p = self.params(w, K, K, C, 1)
        m, v, opt = self._adam_state(w, 1)
        labels = (self.uni(nb, C) > 0.5).float()
        off = torch.tensor([0] + list(itertools.accumulate(lengths)), dtype=torch.int64, device=self.dev)
        pw, wt = self.uni(C) + 0.5, self.uni(C) + 0.5
        bw = self.nat.BceWeights(pw.data_ptr(), wt.data_ptr())
        size = self.L.dsmil_agg_train_step_bags_bf16_workspace_bytes if b16 else self.L.dsmil_agg_train_step_bags_workspace_bytes
        each, mean = [], []
        for step in (1, 2, 3):
            opt.step = step
            le, lo = self.nan(nb), self.nan(1)
            ws = self.workspace(size(nb, T, K, C, 1))
            args = [ptr(feats), ptr(off), nb, T, max(lengths)] + ([] if b16 else [None]) + \
                   [ptr(labels), ctypes.byref(p), ctypes.byref(opt), ptr(le), ptr(lo), *ws] + ([ctypes.byref(bw)] if weighted else [])
            self.call(entry, *args, self.st)
            each.append(le); mean.append(lo)
        self._step_outputs(w, m, v, {"loss_each": each, "loss": mean})

    def run(self, name):
        kind, kw = CASES[name]
        self.seed(name)
        getattr(self, kind)(**kw)
        self.keep = []


W_KEYS = ("fc_w", "fc_b", "q0_w", "q0_b", "q2_w", "q2_b", "fcc_w", "fcc_b")


def trace_case(lib_path, name, timeout, script=os.path.abspath(__file__)):
    with tempfile.TemporaryDirectory() as d:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "-f", "csv", "-d", d, "--", sys.executable, script,
               "case", "--lib", lib_path, "--case", name]
        subprocess.run(cmd, check=True, timeout=timeout, stdout=subprocess.DEVNULL)
        rows = []
        for f in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
            rows += list(csv.DictReader(open(f)))
    rows.sort(key=lambda r: int(r.get("Dispatch_Id") or r.get("Start_Timestamp")))
    out = []
    for r in rows:
        # (a name the profiler leaves mangled, as k_pack_value's with its _Float16 argument, has its length in front)
        m = re.search(r"(?:^|[\s:\d])(k_[a-z0-9_]+(?:<.*>)?)", r["Kernel_Name"])
        if not m:
            continue   # the framework's own kernels (tensor fills, casts)
        dims = lambda stem: [int(r[k]) for k in (stem + "_X", stem + "_Y", stem + "_Z") if k in r] or [int(r[stem])]  # noqa: E731
        out.append({"kernel": re.sub(r"\(.*$", "", m.group(1)), "grid": dims("Grid_Size"), "workgroup": dims("Workgroup_Size"),
                    "lds": int(r.get("LDS_Block_Size", r.get("LDS_Block_Size_v", 0)))})
    return out


def compare_bits(dir_a, dir_b, cases=None):
    import numpy as np
    res = {"a": os.path.basename(os.path.normpath(dir_a)), "b": os.path.basename(os.path.normpath(dir_b)), "cases": {}}
    for name in (CASES if cases is None else cases):
        fa = sorted(os.listdir(os.path.join(dir_a, name))) if os.path.isdir(os.path.join(dir_a, name)) else []
        fb = sorted(os.listdir(os.path.join(dir_b, name))) if os.path.isdir(os.path.join(dir_b, name)) else []
        tensors = {}
        for f in sorted(set(fa) | set(fb)):
            a = open(os.path.join(dir_a, name, f), "rb").read() if f in fa else None
            b = open(os.path.join(dir_b, name, f), "rb").read() if f in fb else None
            arr = np.load(os.path.join(dir_a, name, f)) if f in fa else None
            tensors[f[:-4]] = {"equal": a is not None and a == b, "bytes": len(a) if a is not None else None,
                               "sha256": hashlib.sha256(a).hexdigest() if a is not None else None,
                               # (an output the call does not write keeps the NaN fill: g_fc_* without g_max / g_classes)
                               "nan_values": int(np.isnan(arr).sum()) if arr is not None and arr.dtype.kind == "f" else 0}
        res["cases"][name] = {"equal": bool(tensors) and fa == fb and all(t["equal"] for t in tensors.values()), "tensors": tensors}
    res["all_equal"] = all(c["equal"] for c in res["cases"].values())
    return res


def bench_legs(lib_name, timeout):
    """One run of every timed leg with the library `lib_name` (a file next to _native.py): {leg: bags/s}."""
    env = dict(os.environ, DSMIL_NATIVE_LIB=lib_name)
    root = _path.ROOT
    legs = {}
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--steps", "20", "--warmup", "3", "--full",
                        "--workload", "train"], env=env, capture_output=True, text=True, timeout=timeout)
    if r.returncode != 0:
        raise SystemExit("bench.py failed:\n" + r.stdout[-2000:] + r.stderr[-4000:])
    line = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])

    # (without the headline leg bench.py promotes the first leg, train_c1, to the line itself)
    assert "trained" in line["metric"] and line["config"]["classes"] == 1 and line["train_c2"]["config"]["classes"] == 2, line["metric"]
    legs["train_c1"], legs["train_c2"] = line["value"], line["train_c2"]["value"]
    for dtype in ("fp32", "bf16"):
        with tempfile.TemporaryDirectory() as d:
            out = os.path.join(d, "t.json")
            r = subprocess.run([sys.executable, os.path.join(root, "tools", "bwd_bags_time.py"), "--train", "--train-only", "--dtype", dtype,
                                "--out", out], env=env, capture_output=True, text=True, timeout=timeout)
            if r.returncode != 0:
                raise SystemExit("bwd_bags_time.py failed:\n" + r.stdout[-2000:] + r.stderr[-4000:])
            res = json.load(open(out))
        key = [k for k in res if k.startswith("train_")][0]
        for per_step, v in res[key].items():
            legs[f"bags_train_{dtype}_{per_step}"] = v["bags_per_s_median"]
    return legs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=("sizes", "bits", "compare-bits", "launches", "compare-launches", "time", "case"))
    ap.add_argument("paths", nargs="*")
    ap.add_argument("--lib")
    ap.add_argument("--case")
    ap.add_argument("--dump")
    ap.add_argument("--out")
    ap.add_argument("--names", nargs=2, metavar=("PARENT.so", "NEW.so"))
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--timeout", type=int, default=180, help="seconds per child process")
    a = ap.parse_args()
    res = None
    if a.mode == "sizes":
        import dsmil  # noqa: F401
        import test_bwd_sizes_cabi as t
        a.out = a.out or t.GOLDEN
        res = t.query()
    elif a.mode == "case":
        Driver(a.lib).run(a.case)
        return 0
    elif a.mode == "bits":
        d = Driver(a.lib, dump=a.dump)
        for name in CASES:     # a case that fails ends the process: nothing more is started on the device
            d.run(name)
            print(name, "ok", flush=True)
        return 0
    elif a.mode == "compare-bits":
        res = compare_bits(*a.paths)
        print("all_equal:", res["all_equal"], [n for n, c in res["cases"].items() if not c["equal"]])
    elif a.mode == "launches":
        res = {}
        for name in CASES:     # a case that fails ends the run: nothing more is started on the device
            res[name] = trace_case(a.lib, name, a.timeout)
            print(name, len(res[name]), "launches", flush=True)
    elif a.mode == "compare-launches":
        A, B = (json.load(open(f)) for f in a.paths)
        res = {"a": os.path.basename(a.paths[0]), "b": os.path.basename(a.paths[1]), "cases": {}}
        for name in CASES:
            res["cases"][name] = {"equal": A.get(name) == B.get(name), "launches": A.get(name)}
            if A.get(name) != B.get(name):
                res["cases"][name]["launches_b"] = B.get(name)
        res["all_equal"] = all(c["equal"] and c["launches"] for c in res["cases"].values())
        print("all_equal:", res["all_equal"], [n for n, c in res["cases"].items() if not (c["equal"] and c["launches"])])
    elif a.mode == "time":
        runs = {n: [] for n in a.names}
        for i in range(a.repeats):
            for n in a.names:      # alternating; a failed child ends the run
                runs[n].append(bench_legs(n, a.timeout))
                print(i, n, json.dumps(runs[n][-1]), flush=True)
        parent, new = a.names
        res = {"parent": parent, "new": new, "unit": "bags/s", "runs": runs, "legs": {}}
        for leg in runs[parent][0]:
            pv, nv = [r[leg] for r in runs[parent]], [r[leg] for r in runs[new]]
            res["legs"][leg] = {"parent_median": statistics.median(pv), "parent_min": min(pv), "parent_max": max(pv),
                                "new_median": statistics.median(nv), "new_min": min(nv), "new_max": max(nv),
                                "new_median_inside_parent_range": min(pv) <= statistics.median(nv) <= max(pv)}
        res["all_inside"] = all(v["new_median_inside_parent_range"] for v in res["legs"].values())
        print(json.dumps(res["legs"], indent=1))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        json.dump(res, open(a.out, "w"), indent=1)
    if a.mode.startswith("compare"):
        return 0 if res["all_equal"] else 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
