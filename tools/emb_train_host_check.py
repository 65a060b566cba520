#!/usr/bin/env python
"""One-off checks that a change of the embedder training path's HOST code and Python glue (csrc/emb_host.h and what includes
it, ops.py, simclr.py) left bits, launches and time alone: two builds, the parent commit's and the new one.  A library is named
by its path, and the Python that drives it is the tree the library lies in (<tree>/dsmil-wsi_amd/<lib>.so): the parent's
library inside a checkout of the parent is driven by the parent's ops.py and simclr.py.

    python tools/emb_train_host_check.py bits --lib L.so --dump DIR      every case in ONE process, inputs from fixed seeds; the
        stage entries through the C-ABI with the workspace and every output NaN-filled before each call, the blocks through
        simclr.NativeBasicBlock (forward + backward), the inference forward through tools/embed_plan_check.py's d18_in_f32.
        Every output tensor as DIR/<case>/<t>.npy.  The process ends at the first non-zero return code or HIP error and starts
        nothing after it.
    python tools/emb_train_host_check.py compare-bits DIR_A DIR_B --out profiles/emb_train_glue/bits.json
    python tools/emb_train_host_check.py launches --lib L.so --out A.json     the same cases in one process under ONE
        `rocprofv3 --kernel-trace --stats` run (no counters): the ordered (kernel, grid, workgroup, LDS bytes) of the library
    python tools/emb_train_host_check.py compare-launches A.json B.json --out profiles/emb_train_glue/launches.json
    python tools/emb_train_host_check.py time --libs PARENT.so NEW.so --out profiles/emb_train_glue/times.json
        each tree's own tools/norm_bwd_time.py, conv_bwd_time.py and trunk_time.py as they are, in fresh processes, alternating
        between the two (parent first in even repeats, new first in odd ones); per leg the parent's min-max and both medians
"""
import argparse
import hashlib
import json
import os
import re
import statistics
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))


def tree_of(lib):
    """(tree root, library file name) of <tree>/dsmil-wsi_amd/<name>.so"""
    lib = os.path.abspath(lib)
    return os.path.dirname(os.path.dirname(lib)), os.path.basename(lib)


def _cases():
    import conv_bwd_cases as cc
    import norm_bwd_cases as nc
    import trunk32_cases as tc
    c = {}
    for prec in (0, 1):
        for name, B, H, W, Cin, Cout, ks, stride, pad, norm in tc.DIRECT_CASES:
            c[f"t32_{name}_p{prec}"] = ("t32_conv", dict(B=B, H=H, W=W, Cin=Cin, Cout=Cout, ks=ks, stride=stride, pad=pad, norm=norm, prec=prec))
        for name, B, H, W, Cin, Cout, norm in tc.WINO_CASES:
            c[f"t32_{name}_p{prec}"] = ("t32_conv", dict(B=B, H=H, W=W, Cin=Cin, Cout=Cout, ks=3, stride=1, pad=1, norm=norm, prec=prec))
        for name, B, H, W, Cin, Cout, ks, stride, pad, _ in tc.EXACT_CASES:
            c[f"t32_{name}_p{prec}"] = ("t32_conv", dict(B=B, H=H, W=W, Cin=Cin, Cout=Cout, ks=ks, stride=stride, pad=pad, norm=False, prec=prec))
        for name, B, H, W, u8, frozen in tc.STEM_CASES:
            c[f"t32_{name}_p{prec}"] = ("t32_stem", dict(B=B, H=H, W=W, u8=u8, frozen=frozen, prec=prec))
        for name, B, H, W, _ in tc.STEM_EXACT:
            c[f"t32_{name}_p{prec}"] = ("t32_stem", dict(B=B, H=H, W=W, u8=False, frozen=False, prec=prec))
    for name, kind, B, HW, C in tc.TAIL_CASES:
        c[f"t32_{name}"] = ("t32_tail", dict(kind=kind, B=B, HW=HW, C=C))
    shapes = [(n, B, H, W, Cin, Cout, ks, s, p, mag) for n, B, H, W, Cin, Cout, ks, s, p, _, mag in cc.CASES]
    shapes += [(n, B, H, W, Cin, Cout, ks, s, p, 1.0) for n, _, B, H, W, Cin, Cout, ks, s, p, _ in cc.EXACT_CASES]
    for name, B, H, W, Cin, Cout, ks, stride, pad, mag in shapes:
        kw = dict(B=B, H=H, W=W, Cin=Cin, Cout=Cout, ks=ks, stride=stride, pad=pad, mag=mag)
        c[f"cb_{name}_weight"] = ("cb_weight", dict(kw, norm=False))
        c[f"cb_{name}_weight_in_stats"] = ("cb_weight", dict(kw, norm=True))
        if Cin != 3:                                            # (the stem has no data gradient)
            c[f"cb_{name}_data"] = ("cb_data", kw)
    for name, kind, B, HW, C, mag in nc.CASES:
        c[f"nb_{name}"] = ("norm_bwd", dict(kind=kind, B=B, HW=HW, C=C, mag=mag))
    for name in ("id_64", "down_128"):                          # the block shapes of tests/test_norm_bwd_gpu.py
        for cl in (True, False):
            c[f"block_{name}_{'channels_last' if cl else 'nchw'}"] = ("block", dict(name=name, channels_last=cl))
    c["embed_d18_in_f32"] = ("embed", {})
    return c


def make_driver(lib, dump):
    import bwd_host_check as base
    import trunk32_cases as tc

    class Driver(base.Driver):
        def run(self, name, kind, kw):
            self.seed(name)
            getattr(self, kind)(**kw)
            self.keep = []

        def ws(self, nbytes):
            if nbytes <= 0:
                raise SystemExit(f"{self.case}: the size query refuses the shape")
            return self.workspace(nbytes)

        def stats(self, B, C):
            return self.rnd(B, C, scale=0.3), self.uni(B, C) * 1.5 + 0.5

        def t32_conv(self, B, H, W, Cin, Cout, ks, stride, pad, norm, prec):
            ptr, L = self.ptr, self.L
            Ho, Wo = tc.out_size(H, ks, stride, pad), tc.out_size(W, ks, stride, pad)
            x, w = self.rnd(B, H, W, Cin), self.rnd(Cout, Cin, ks, ks, scale=(2.0 / (Cout * ks * ks)) ** 0.5)
            im, ir = self.stats(B, Cin) if norm else (None, None)
            y, mean, rstd = self.nan(B, Ho, Wo, Cout), self.nan(B, Cout), self.nan(B, Cout)
            ws = self.ws(L.dsmil_trunk32_conv_workspace_bytes(Cin, Cout, ks, stride, pad, B, H, W, prec))
            self.call("dsmil_trunk32_conv", ptr(x), ptr(w), ptr(im), ptr(ir), None, None, ptr(y), ptr(mean), ptr(rstd), B, H, W, Cin,
                      Cout, ks, stride, pad, prec, *ws, self.st)
            self.out("y", y); self.out("mean", mean); self.out("rstd", rstd)

        def t32_stem(self, B, H, W, u8, frozen, prec):
            torch, ptr, L = self.torch, self.ptr, self.L
            x = torch.randint(0, 256, (B, H, W, 3), generator=self.g, dtype=torch.uint8).to(self.dev) if u8 else self.uni(B, 3, H, W)
            w = self.rnd(64, 3, 7, 7, scale=(2.0 / (64 * 49)) ** 0.5)
            bm, br = (self.rnd(64, scale=0.1), self.uni(64) + 0.5) if frozen else (None, None)
            H1, W1, Hp, Wp = tc.stem_dims(H, W)
            pooled, mean, rstd = self.nan(B, Hp, Wp, 64), self.nan(B, 64), self.nan(B, 64)
            ws = self.ws(L.dsmil_trunk32_stem_workspace_bytes(B, H, W))
            self.call("dsmil_trunk32_stem", ptr(x), 1 if u8 else 0, ptr(w), ptr(bm), ptr(br), ptr(pooled), ptr(mean), ptr(rstd), B, H, W,
                      prec, *ws, self.st)
            self.out("pooled", pooled); self.out("mean", mean); self.out("rstd", rstd)

        def t32_tail(self, kind, B, HW, C):
            ptr = self.ptr
            y2, idn, (m, r) = self.rnd(B, HW, C), self.rnd(B, HW, C), self.stats(B, C)
            md, rd = self.stats(B, C) if kind == "down" else (None, None)
            out = self.nan(B, C) if kind == "pool" else self.nan(B, HW, C)
            self.call("dsmil_trunk32_tail", {"identity": 0, "down": 1, "pool": 2}[kind], ptr(y2), ptr(m), ptr(r), ptr(idn), ptr(md), ptr(rd),
                      ptr(out), B, HW, C, 0, self.st)
            self.out("out", out)

        def cb_weight(self, B, H, W, Cin, Cout, ks, stride, pad, mag, norm):
            ptr, L = self.ptr, self.L
            Ho, Wo = tc.out_size(H, ks, stride, pad), tc.out_size(W, ks, stride, pad)
            x, dy = self.rnd(B, H, W, Cin), self.rnd(B, Ho, Wo, Cout, scale=mag)
            im, ir = self.stats(B, Cin) if norm else (None, None)
            dw = self.nan(Cout, Cin, ks, ks)
            ws = self.ws(L.dsmil_conv_bwd_workspace_bytes(Cin, Cout, ks, stride, pad, B, H, W, 0))
            self.call("dsmil_conv_bwd_weight", ptr(x), ptr(im), ptr(ir), ptr(dy), ptr(dw), B, H, W, Cin, Cout, ks, stride, pad, *ws, self.st)
            self.out("dw", dw)

        def cb_data(self, B, H, W, Cin, Cout, ks, stride, pad, mag):
            ptr, L = self.ptr, self.L
            Ho, Wo = tc.out_size(H, ks, stride, pad), tc.out_size(W, ks, stride, pad)
            dy, w = self.rnd(B, Ho, Wo, Cout, scale=mag), self.rnd(Cout, Cin, ks, ks, scale=(2.0 / (Cout * ks * ks)) ** 0.5)
            dx = self.nan(B, H, W, Cin)
            ws = self.ws(L.dsmil_conv_bwd_workspace_bytes(Cin, Cout, ks, stride, pad, B, H, W, 1))
            self.call("dsmil_conv_bwd_data", ptr(dy), ptr(w), ptr(dx), B, H, W, Cin, Cout, ks, stride, pad, *ws, self.st)
            self.out("dx", dx)

        def norm_bwd(self, kind, B, HW, C, mag):
            ptr, L = self.ptr, self.L
            k = {"relu": 0, "add": 1, "add_down": 2}[kind]
            g, y, (m, r) = self.rnd(B, HW, C, scale=mag), self.rnd(B, HW, C), self.stats(B, C)
            out = self.rnd(B, HW, C).relu_() if k else None
            yd, (md, rd) = (self.rnd(B, HW, C), self.stats(B, C)) if k == 2 else (None, (None, None))
            gy, gyd, gres = self.nan(B, HW, C), (self.nan(B, HW, C) if k == 2 else None), (self.nan(B, HW, C) if k == 1 else None)
            ws = self.ws(L.dsmil_norm_bwd_workspace_bytes(k, B, HW, C))
            self.call("dsmil_norm_bwd", k, ptr(g), ptr(out), ptr(y), ptr(m), ptr(r), ptr(yd), ptr(md), ptr(rd), ptr(gy), ptr(gyd), ptr(gres),
                      B, HW, C, *ws, self.st)
            self.out("gy", gy); self.out("gyd", gyd); self.out("gres", gres)

        def block(self, name, channels_last):
            import norm_bwd_cases as nc
            from dsmil_wsi_amd import simclr
            torch = self.torch
            wrap = torch.nn.Sequential(nc.make_block(name))
            assert simclr.use_native_blocks(wrap) == 1
            blk = wrap[0].to(self.dev)
            x, c = (t.to(self.dev) for t in nc.block_inputs(name))
            if channels_last:
                x = x.contiguous(memory_format=torch.channels_last)
            x.requires_grad_(True)
            out = blk(x)
            assert "BasicBlockNative" in nc.grad_fn_names(out)
            params = [p for p in blk.parameters() if p.dim() == 4]
            grads = torch.autograd.grad((out * c).sum(), [x] + params)
            torch.cuda.synchronize()
            self.out("out", out.contiguous())
            for i, t in enumerate(grads):
                self.out(f"grad{i}", t.contiguous())

        def embed(self):
            import embed_plan_check as ep
            self.out("feats", self.torch.from_numpy(ep.run_case(*[c for c in ep.CASES if c[0] == "d18_in_f32"][0][1:])))

    return Driver(lib, dump=dump)


def ms_legs(d, path=()):
    """{leg: milliseconds} of every '*_ms' number of a timing tool's result."""
    out = {}
    for k, v in d.items():
        if isinstance(v, dict):
            out.update(ms_legs(v, path + (k,)))
        elif isinstance(v, (int, float)) and not isinstance(v, bool) and k.endswith("_ms"):
            out["/".join(path + (k,))] = v
    return out


def time_legs(lib, timeout, batches):
    """One fresh process per tool of the tree `lib` lies in: {leg: ms}."""
    tree, name = tree_of(lib)
    env = dict(os.environ, DSMIL_NATIVE_LIB=name)
    legs = {}

    def run(*args):
        r = subprocess.run([sys.executable, os.path.join(tree, "tools", args[0])] + list(args[1:]), env=env, cwd=tree, capture_output=True,
                           text=True, timeout=timeout)
        if r.returncode != 0:
            raise SystemExit(args[0] + " failed:\n" + r.stdout[-2000:] + r.stderr[-4000:])
        return r.stdout

    with tempfile.TemporaryDirectory() as d:
        run("norm_bwd_time.py", "--out-dir", d, "--batches", *batches)
        for f in ("times.json", "step.json"):
            res = json.load(open(os.path.join(d, f)))
            legs.update({f"norm_bwd_time:{f[:-5]}:{k}": v for k, v in ms_legs(res).items()})
        run("conv_bwd_time.py", "--out", os.path.join(d, "c.json"), "--batches", *batches)
        legs.update({"conv_bwd_time:" + k: v for k, v in ms_legs(json.load(open(os.path.join(d, "c.json")))).items()})
    for depth in ("18",):
        for B in batches:
            m = re.search(r"([\d.]+) ms per forward", run("trunk_time.py", depth, B))
            legs[f"trunk_time:depth{depth}_bs{B}/forward_ms"] = float(m.group(1))
    return legs


def bits_record(res):
    """compare_bits' result, one line per case: {tensor: first 16 hex digits of its SHA-256}."""
    out = {k: res[k] for k in ("a", "b", "all_equal")}
    out["tensors"] = sum(len(c["tensors"]) for c in res["cases"].values())
    out["nan_values"] = sum(t["nan_values"] for c in res["cases"].values() for t in c["tensors"].values())
    out["all_equal"] = out["all_equal"] and out["nan_values"] == 0
    out["unequal_cases"] = [n for n, c in res["cases"].items() if not c["equal"]]
    out["cases"] = {n: {t: (v["sha256"] or "missing")[:16] for t, v in c["tensors"].items()} for n, c in res["cases"].items()}
    return out


def launches_record(A, B, names):
    """The two ordered launch lists by their SHA-256, and per kernel the launches and the distinct (grid, workgroup, LDS) it ran with."""
    la, lb = A["all_cases_in_order"], B["all_cases_in_order"]
    sha = lambda l: hashlib.sha256(json.dumps(l, sort_keys=True).encode()).hexdigest()   # noqa: E731
    out = {"a": names[0], "b": names[1], "n_cases": len(A["cases"]), "n_launches": len(la), "n_launches_b": len(lb),
           "ordered_list_sha256": sha(la), "ordered_list_sha256_b": sha(lb), "all_equal": bool(la) and A == B, "kernels": {}}
    for x in la:
        k = out["kernels"].setdefault(x["kernel"], {"launches": 0, "grid_workgroup_lds": []})
        k["launches"] += 1
        if [x["grid"], x["workgroup"], x["lds"]] not in k["grid_workgroup_lds"]:
            k["grid_workgroup_lds"].append([x["grid"], x["workgroup"], x["lds"]])
    if not out["all_equal"]:
        out["first_difference"] = next(([i, p, q] for i, (p, q) in enumerate(zip(la, lb)) if p != q), None)
    return out


def times_record(runs, parent, new, batches):
    """Per leg every run of both sides (ms, in run order), both medians and whether the new median lies in the parent's range."""
    r4 = lambda v: round(v, 5)   # noqa: E731
    res = {"parent": parent, "new": new, "unit": "ms", "batches": batches, "order": "parent first in even repeats, new first in odd"}
    legs = {}
    for leg in runs[parent][0]:
        pv, nv = [r[leg] for r in runs[parent]], [r[leg] for r in runs[new]]
        legs[leg] = {"parent": [r4(v) for v in pv], "new": [r4(v) for v in nv], "parent_median": r4(statistics.median(pv)),
                     "new_median": r4(statistics.median(nv)), "inside_parent_range": min(pv) <= statistics.median(nv) <= max(pv)}
    res["all_inside"] = all(v["inside_parent_range"] for v in legs.values())
    res["legs_outside"] = [k for k, v in legs.items() if not v["inside_parent_range"]]
    res["legs"] = legs
    return res


def dump_rows(res, path, key):
    """json with one line per entry of res[key] (the last key): a record a reader can take in and a diff can show."""
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    head = {k: v for k, v in res.items() if k != key}
    with open(path, "w") as f:
        f.write(json.dumps(head, indent=1)[:-2] + ',\n "%s": {\n' % key)
        f.write(",\n".join("  %s: %s" % (json.dumps(k), json.dumps(v)) for k, v in res[key].items()))
        f.write("\n }\n}\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=("bits", "compare-bits", "launches", "compare-launches", "time", "case"))
    ap.add_argument("paths", nargs="*")
    ap.add_argument("--lib")
    ap.add_argument("--case", help="(ignored: `case` runs every case, the form `launches` traces)")
    ap.add_argument("--dump")
    ap.add_argument("--out")
    ap.add_argument("--libs", nargs=2, metavar=("PARENT.so", "NEW.so"))
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--batches", nargs="*", default=["64", "256"])
    ap.add_argument("--timeout", type=int, default=600, help="seconds per child process")
    a = ap.parse_args()
    tree = tree_of(a.lib)[0] if a.lib else os.path.dirname(HERE)
    if a.lib:
        os.environ["DSMIL_NATIVE_LIB"] = tree_of(a.lib)[1]         # what dsmil_wsi_amd._native loads in this process
    import bwd_host_check as base   # (puts this tree and its tests/ on sys.path: the case tables and tools are THIS tree's)
    sys.path.insert(0, tree)        # ... and the package is the library's tree's
    res = None
    if a.mode in ("bits", "case"):
        d = make_driver(a.lib, a.dump)
        for name, (kind, kw) in _cases().items():     # a case that fails ends the process: nothing more is started on the device
            d.run(name, kind, kw)
            print(name, "ok", flush=True)
        return 0
    if a.mode == "compare-bits":
        res = bits_record(base.compare_bits(*a.paths, cases=_cases()))
        print(len(res["cases"]), "cases,", res["tensors"], "tensors,", res["nan_values"], "NaN values")
    elif a.mode == "launches":
        res = {"all_cases_in_order": base.trace_case(a.lib, "all", a.timeout, script=os.path.abspath(__file__)), "cases": list(_cases())}
        print(len(res["all_cases_in_order"]), "launches", flush=True)
    elif a.mode == "compare-launches":
        A, B = (json.load(open(f)) for f in a.paths)
        res = launches_record(A, B, [os.path.basename(f) for f in a.paths])
    elif a.mode == "time":
        runs = {n: [] for n in a.libs}
        for i in range(a.repeats):
            for n in (a.libs if i % 2 == 0 else a.libs[::-1]):     # A B, B A, ...: neither is always the one that runs second
                runs[n].append(time_legs(n, a.timeout, a.batches))
                print(i, n, "ok", flush=True)
                if a.out:          # (kept as it grows: a run cut short still leaves what it measured)
                    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
                    json.dump({"partial_runs": runs}, open(a.out, "w"), indent=1)
        parent, new = a.libs
        res = times_record(runs, parent, new, a.batches)
        print(json.dumps(res["legs_outside"]))
    if a.out:
        if a.mode == "launches":     # (the raw ordered list of one side: an intermediate, compare-launches reads two of them)
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            json.dump(res, open(a.out, "w"))
        else:
            dump_rows(res, a.out, {"compare-bits": "cases", "compare-launches": "kernels", "time": "legs"}[a.mode])
    if a.mode.startswith("compare"):
        print("all_equal:", res["all_equal"])
        return 0 if res["all_equal"] else 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
