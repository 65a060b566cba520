#!/usr/bin/env python
"""One-off checks that moving the value layer's HOST code into csrc/agg_value.hip left bits, launches and time alone: two
builds of the library, the parent commit's and the new one, driven through the C-ABI only (bwd_host_check.py's driver).

    python tools/value_host_check.py bits --lib L.so --dump DIR      every case in ONE process, inputs from a fixed seed, the
        workspace and every output NaN-filled before each call; every output tensor as DIR/<case>/<t>.npy.  The process ends
        at the first non-zero return code or HIP error and starts nothing after it.
    python tools/value_host_check.py compare-bits DIR_A DIR_B --out profiles/value_host/bits.json
    python tools/value_host_check.py launches --lib L.so --out A.json     the same cases in one process under ONE
        `rocprofv3 --kernel-trace --stats` run (no counters): the ordered (kernel, grid, workgroup, LDS bytes) of the library
    python tools/value_host_check.py compare-launches A.json B.json --out profiles/value_host/launches.json
    python tools/value_host_check.py time --names libdsmil_hip_parent.so libdsmil_hip.so --out profiles/value_host/times.json
        tools/value_proj_time.py, value_b16_time.py, value_bwd_b16_time.py and gx_time.py as they are, alternating between
        the two libraries (file names next to dsmil-wsi_amd/_native.py); the new median against the parent's min-max
"""
import argparse
import ctypes
import json
import os
import statistics
import subprocess
import sys
import tempfile

import _path  # noqa: F401
import bwd_host_check as base

FWD = [(1, 64, 64), (70, 166, 166), (200, 512, 512), (130, 1024, 256), (40, 1056, 64)]
FWD_B16 = [(1, 64, 64), (70, 72, 68), (200, 512, 512), (40, 1056, 64)]
BWD = [(200, 64, 64), (1000, 512, 512), (70, 72, 68)]
ROWS = [(70, 166, 166), (200, 512, 512)]


def _cases():
    c = {}
    for n, K, Kv in FWD:
        for rowmap in (False, True):
            for image in ("caller", "cut"):
                c[f"fwd_{n}x{K}x{Kv}_{'rowmap' if rowmap else 'plain'}_{image}"] = ("fwd", dict(n=n, K=K, Kv=Kv, rowmap=rowmap, image=image))
    for n, K, Kv in FWD_B16:
        for image in ("caller", "cut"):
            c[f"fwd_b16_{n}x{K}x{Kv}_{image}"] = ("fwd", dict(n=n, K=K, Kv=Kv, rowmap=False, image=image, b16=True))
    for n, K, Kv in BWD:
        c[f"bwd_{n}x{K}x{Kv}"] = ("bwd", dict(n=n, K=K, Kv=Kv))
        c[f"bwd_b16_{n}x{K}x{Kv}"] = ("bwd", dict(n=n, K=K, Kv=Kv, b16=True))
    c["bwd_200x64x64_rowmap"] = ("bwd", dict(n=200, K=64, Kv=64, rowmap=True))
    for n, K, Kv in ROWS:
        for acc in (0, 1):
            c[f"rows_{n}x{K}x{Kv}_{'accumulate' if acc else 'write'}"] = ("rows", dict(n=n, K=K, Kv=Kv, acc=acc))
    return c


CASES = _cases()


class Driver(base.Driver):
    def run(self, name):
        kind, kw = CASES[name]
        self.seed(name)
        getattr(self, kind)(**kw)
        self.keep = []

    def nan_bytes(self, nbytes):
        t = self.torch.full((nbytes + 256,), 0xFF, dtype=self.torch.uint8, device=self.dev)
        self.keep.append(t)
        return ctypes.c_void_p((t.data_ptr() + 255) // 256 * 256)

    def fwd(self, n, K, Kv, rowmap, image, b16=False):
        torch, ptr, L = self.torch, self.ptr, self.L
        sfx = "_bf16" if b16 else ""
        x = self.rnd(n + (5 if rowmap else 0), K)
        w, b = self.rnd(Kv, K, scale=0.05), self.rnd(Kv, scale=0.1)
        rm = torch.randperm(x.shape[0], generator=self.g)[:n].to(self.dev) if rowmap else None
        V = self.nan(n, Kv)
        if b16:
            x, V = x.to(torch.bfloat16), V.to(torch.bfloat16)
        img = None
        ws_bytes = L.dsmil_value_workspace_bf16_bytes(n, K, Kv) if b16 else L.dsmil_value_workspace_bytes(n, K, Kv)
        ws = (self.nan_bytes(ws_bytes), ws_bytes) if ws_bytes else (None, 0)
        if image == "caller":
            img = self.nan_bytes(getattr(L, f"dsmil_value_packed{sfx}_bytes")(K, Kv))
            self.call("dsmil_value_pack" + sfx, ptr(w), K, Kv, img, self.st)
            ws = (None, 0)
        if b16:
            self.call("dsmil_value_forward_bf16", ptr(x), n, K, Kv, ptr(w), ptr(b), img, ptr(V), *ws, self.st)
        else:
            self.call("dsmil_value_forward", ptr(x), n, K, Kv, ptr(w), ptr(b), img, ptr(rm), ptr(V), *ws, self.st)
        self.out("V", V.view(torch.int16) if b16 else V)

    def bwd(self, n, K, Kv, b16=False, rowmap=False):
        torch, ptr, L = self.torch, self.ptr, self.L
        x, V, g = self.rnd(n + (5 if rowmap else 0), K), self.rnd(n, Kv).clamp(min=0), self.rnd(n, Kv, scale=0.1)
        rm = torch.randperm(x.shape[0], generator=self.g)[:n].to(self.dev) if rowmap else None
        gw, gb = self.nan(Kv, K), self.nan(Kv)
        if b16:
            xb, Vb = x.to(torch.bfloat16), V.to(torch.bfloat16)
            ws = self.workspace(L.dsmil_value_backward_bf16_workspace_bytes(n, K, Kv))
            self.call("dsmil_value_backward_bf16", ptr(xb), ptr(Vb), ptr(g), n, K, Kv, ptr(gw), ptr(gb), *ws, self.st)
        else:
            ws = self.workspace(L.dsmil_value_workspace_bytes(n, K, Kv))
            self.call("dsmil_value_backward", ptr(x), ptr(V), ptr(g), n, K, Kv, ptr(rm), ptr(gw), ptr(gb), *ws, self.st)
        self.out("g_v_w", gw)
        self.out("g_v_b", gb)

    def rows(self, n, K, Kv, acc):
        ptr = self.ptr
        V, g, w = self.rnd(n, Kv).clamp(min=0), self.rnd(n, Kv, scale=0.1), self.rnd(Kv, K, scale=0.05)
        gx = self.rnd(n, K) if acc else self.nan(n, K)
        self.call("dsmil_value_backward_rows", None, ptr(V), ptr(g), n, K, Kv, ptr(w), None, acc, ptr(gx), None, 0, self.st)
        self.out("g_feats", gx)


def medians(d, path=()):
    """{leg: value} of every '*median*' number of a timing tool's result (its peak-share arithmetic left out)."""
    out = {}
    for k, v in d.items():
        if isinstance(v, dict) and k != "peak_share":
            out.update(medians(v, path + (k,)))
        elif isinstance(v, (int, float)) and not isinstance(v, bool) and "median" in k:
            out["/".join(path + (k,))] = v
    return out


def time_legs(lib_name, timeout):
    env = dict(os.environ, DSMIL_NATIVE_LIB=lib_name)
    legs = {}
    for tool in ("value_proj_time.py", "value_b16_time.py", "value_bwd_b16_time.py", "gx_time.py"):
        with tempfile.TemporaryDirectory() as d:
            out = os.path.join(d, "t.json")
            r = subprocess.run([sys.executable, os.path.join(_path.ROOT, "tools", tool), "--out", out], env=env, capture_output=True,
                               text=True, timeout=timeout)
            if r.returncode != 0:
                raise SystemExit(tool + " failed:\n" + r.stdout[-2000:] + r.stderr[-4000:])
            legs.update({tool[:-3] + ":" + k: v for k, v in medians(json.load(open(out))).items()})
    return legs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=("bits", "compare-bits", "launches", "compare-launches", "time", "case"))
    ap.add_argument("paths", nargs="*")
    ap.add_argument("--lib")
    ap.add_argument("--case", help="(ignored: `case` runs every case, the form `launches` traces)")
    ap.add_argument("--dump")
    ap.add_argument("--out")
    ap.add_argument("--names", nargs=2, metavar=("PARENT.so", "NEW.so"))
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--timeout", type=int, default=240, help="seconds per child process")
    a = ap.parse_args()
    res = None
    if a.mode in ("bits", "case"):
        d = Driver(a.lib, dump=a.dump)
        for name in CASES:     # a case that fails ends the process: nothing more is started on the device
            d.run(name)
            print(name, "ok", flush=True)
        return 0
    if a.mode == "compare-bits":
        res = base.compare_bits(*a.paths, cases=CASES)
    elif a.mode == "launches":
        res = {"all_cases_in_order": base.trace_case(a.lib, "all", a.timeout, script=os.path.abspath(__file__)), "cases": list(CASES)}
        print(len(res["all_cases_in_order"]), "launches", flush=True)
    elif a.mode == "compare-launches":
        A, B = (json.load(open(f)) for f in a.paths)
        res = {"a": os.path.basename(a.paths[0]), "b": os.path.basename(a.paths[1]), "cases": A["cases"],
               "launches": A["all_cases_in_order"]}
        res["all_equal"] = bool(A["all_cases_in_order"]) and A == B
        if not res["all_equal"]:
            res["launches_b"] = B["all_cases_in_order"]
    elif a.mode == "time":
        runs = {n: [] for n in a.names}
        for i in range(a.repeats):
            for n in a.names:      # alternating; a failed child ends the run
                runs[n].append(time_legs(n, a.timeout))
                print(i, n, "ok", flush=True)
        parent, new = a.names
        res = {"parent": parent, "new": new, "unit": "as the tool reports it (us per call)", "runs": runs, "legs": {}}
        for leg in runs[parent][0]:
            pv, nv = [r[leg] for r in runs[parent]], [r[leg] for r in runs[new]]
            res["legs"][leg] = {"parent_median": statistics.median(pv), "parent_min": min(pv), "parent_max": max(pv),
                                "new_median": statistics.median(nv), "new_min": min(nv), "new_max": max(nv),
                                "new_median_inside_parent_range": min(pv) <= statistics.median(nv) <= max(pv)}
        res["all_inside"] = all(v["new_median_inside_parent_range"] for v in res["legs"].values())
        res["legs_outside"] = [k for k, v in res["legs"].items() if not v["new_median_inside_parent_range"]]
        print(json.dumps(res["legs_outside"]))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        json.dump(res, open(a.out, "w"), indent=1)
    if a.mode.startswith("compare"):
        print("all_equal:", res["all_equal"])
        return 0 if res["all_equal"] else 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
