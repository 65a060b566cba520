#!/usr/bin/env python
"""One-off check that a change of the Python training glue (dsmil-wsi_amd/training.py, modules.py) left calls, progress lines
and bits alone: a fixed list of seeded scenarios, run on whichever tree is named, once on the parent commit's and once on the
new one's, and the two records compared.

    python tools/train_glue_check.py run --device cpu|cuda [--tree DIR] --out A.json
        every scenario in ONE process; per scenario the ordered native work entries called (a recording proxy around
        ``_native.lib()``, as tests/test_glue_calls_gpu.py; size queries and route functions left out), the number of progress
        lines and the SHA-256 of the printed text, and the SHA-256 of the bytes of the returned values, every parameter,
        exp_avg, exp_avg_sq and each parameter's ``step`` after the run.  A scenario that raises is recorded with its
        exception (and what it printed and left behind until then).  ``--tree``: the checkout whose package is driven
        (default: the one this file lies in).  On ``cuda`` the process ends at the first HIP error.
    python tools/train_glue_check.py diff A.json B.json --out profiles/train_glue/diff_cpu.json
    python tools/train_glue_check.py lines --trees PARENT NEW --out profiles/train_glue/lines.json
        code lines (comments, docstrings and blanks excluded) of training.py and modules.py in both trees
    python tools/train_glue_check.py time --trees PARENT NEW [--repeats 5] --out profiles/train_glue/times.json
        each tree's own tools/train_bench.py, tools/train_mil_time.py, bench.py's train leg and this file's ``loop`` mode, in
        fresh processes, alternating between the two trees (parent first in even repeats, new first in odd ones); per leg
        every run of both, both medians and whether the new median lies above the parent's slowest run
    python tools/train_glue_check.py loop [--tree DIR] --out F.json
        training.train(log=True) over 64 resident 10 000 x 512 bags with bags_per_step 1 and 8: median epoch, ms per bag
"""
import argparse
import contextlib
import hashlib
import io
import json
import os
import struct
import statistics
import subprocess
import sys
import tempfile
import tokenize

HERE = os.path.dirname(os.path.abspath(__file__))
ROWS = (5, 64, 33, 40)     # one wave of rows, two full 32-row tiles, not a multiple of 32; per step 3: a short last group
QUERIES = ("_bytes", "_route", "_form", "_query", "_grid", "_rows_per", "_version", "_strerror", "_cus", "_tile_rows")


class Recorder:
    def __init__(self, real):
        self._real, self.calls = real, []

    def __getattr__(self, name):
        fn = getattr(self._real, name)
        if not callable(fn) or name.endswith(QUERIES):
            return fn

        def call(*args):
            self.calls.append(name)
            return fn(*args)
        return call


def sha(*chunks):
    h = hashlib.sha256()
    for c in chunks:
        h.update(c)
    return h.hexdigest()


def value_bytes(v):
    """Bytes of a returned value: floats as doubles, tensors / arrays as they are, sequences element by element."""
    import numpy as np
    import torch
    if torch.is_tensor(v):
        v = v.detach().cpu().contiguous().numpy() if v.dtype != torch.bfloat16 else v.detach().cpu().view(torch.int16).numpy()
    if isinstance(v, np.ndarray):
        return str(v.dtype).encode() + str(v.shape).encode() + np.ascontiguousarray(v).tobytes()
    if isinstance(v, (list, tuple)):
        return b"[" + b",".join(value_bytes(x) for x in v) + b"]"
    if isinstance(v, (float, int, np.floating, np.integer)):
        return struct.pack("<d", float(v))
    return repr(v).encode()


def state_bytes(net, opt):
    out = []
    for name, p in net.named_parameters():
        st = opt.state.get(p, {}) if opt is not None else {}
        out += [name.encode(), value_bytes(p)] + [value_bytes(st[k]) for k in ("exp_avg", "exp_avg_sq", "step") if k in st]
    return out


def train_bags(K, C, device, seed=11):
    """Four stacked [N, K + C] bags (features || repeated one-hot label), as BagCache.get takes tensors."""
    import torch
    from dsmil_wsi_amd.synthetic import make_bag
    bags = []
    for b, n in enumerate(ROWS):
        lab = torch.zeros(n, C)
        lab[:, b % C] = 1.0
        bags.append(torch.cat([torch.from_numpy(make_bag(seed + b, n, K)), lab], 1).to(device))
    return bags


def scenarios(T, device):
    """name -> callable returning (values, net, optimiser)."""
    import numpy as np
    import torch
    from dsmil_wsi_amd.synthetic import VARIANT, build_net
    out = {}

    def criterion(weighted, C):
        if not weighted:
            return torch.nn.BCEWithLogitsLoss()
        return torch.nn.BCEWithLogitsLoss(weight=torch.linspace(0.5, 1.5, C, device=device), pos_weight=torch.tensor(2.0, device=device))

    def train(tag, per_step, dropout, dtype, weighted, fused, epochs=2):
        def run():
            K, C = VARIANT[tag][:2]
            net = build_net(tag, device).train()
            opt = torch.optim.Adam(net.parameters(), lr=1e-3, betas=(0.5, 0.9), weight_decay=1e-3)
            args = argparse.Namespace(feats_size=K, num_classes=C, dropout_patch=dropout, bags_per_step=per_step, fused_step=fused)
            cache = T.BagCache(device, K, dtype=dtype)
            crit, bags = criterion(weighted, C), train_bags(K, C, device)
            return [T.train(args, bags, net, crit, opt, cache=cache, log=True) for _ in range(epochs)], net, opt
        return run

    for per_step in (1, 3):
        for dropout in (0.0, 0.4):
            for dtype in (torch.float32, torch.bfloat16):
                for weighted in (False, True):
                    for fused in (True, False):
                        name = "train_per%d_drop%g_%s_%s_%s" % (per_step, dropout, "bf16" if dtype == torch.bfloat16 else "fp32",
                                                                "weighted" if weighted else "stock", "fused" if fused else "generic")
                        out[name] = train("tcga", per_step, dropout, dtype, weighted, fused)
        for dropout in (0.0, 0.4):
            out["train_passv_per%d_drop%g" % (per_step, dropout)] = train("passv", per_step, dropout, torch.float32, False, True)

    def test(dropout, average):
        def run():
            K, C = VARIANT["tcga"][:2]
            net = build_net("tcga", device)
            args = argparse.Namespace(feats_size=K, num_classes=C, dropout_patch=dropout, average=average)
            res = T.test(args, train_bags(K, C, device), net, criterion(False, C), cache=T.BagCache(device, K), log=True)
            return [res[0], res[1], list(res[2]), list(res[3])], net, None
        return run
    out["test_drop0"] = test(0.0, True)
    out["test_drop0.4"] = test(0.4, False)

    def mil(native):
        def run():
            import dsmil as mil_mod
            with tempfile.TemporaryDirectory() as d:
                X, bag_ids, labels = T.parse_mil_file(T.write_synthetic_mil_file(os.path.join(d, "musk1_synthetic.svm")))
            bags, ys = T.group_bags(X, bag_ids, labels)
            bags, ys = bags[:12], ys[:12]
            train_idx, test_idx = np.arange(9), np.arange(9, 12)
            torch.manual_seed(0)
            net = mil_mod.MILNet(mil_mod.FCLayer(X.shape[1], 1), mil_mod.BClassifier(input_size=X.shape[1], output_class=1)).to(device)
            pos = float(ys[train_idx].sum())
            crit = torch.nn.BCEWithLogitsLoss(torch.tensor((len(train_idx) - pos) / max(pos, 1.0), device=device))
            opt = torch.optim.Adam(net.parameters(), lr=2e-4, betas=(0.5, 0.9), weight_decay=5e-3)
            keep, vals = T.mil_fused_step, []
            T.mil_fused_step = native
            try:
                for _ in range(2):
                    vals.append(T.mil_epoch_train(bags, ys, train_idx, net, crit, opt, device))
                    vals.append(list(T.mil_epoch_test(bags, ys, test_idx, net, crit, device)))
            finally:
                T.mil_fused_step = keep
            return vals, net, opt
        return run
    out["mil_fused_on"] = mil(True)
    out["mil_fused_off"] = mil(False)
    return out


def run_all(device, out_path):
    import numpy as np
    import torch
    import dsmil  # noqa: F401  (registers the tree's package)
    from dsmil_wsi_amd import _native
    from dsmil_wsi_amd import training as T
    rec = None
    if device == "cuda":
        rec = Recorder(_native.lib())
        _native.lib = lambda: rec
    res = {"device": device, "torch": torch.__version__, "scenarios": {}}
    for name, run in scenarios(T, device).items():
        torch.manual_seed(1234)
        np.random.seed(1234)
        if rec is not None:
            rec.calls = []
        text, entry, vals, net, opt = io.StringIO(), {}, None, None, None
        try:
            with contextlib.redirect_stdout(text):
                vals, net, opt = run()
            if device == "cuda":
                torch.cuda.synchronize()
        except Exception as e:  # noqa: BLE001  (a scenario both trees refuse alike is a result too)
            entry["error"] = "%s: %s" % (type(e).__name__, str(e)[:200])
            if device == "cuda" and ("HIP error" in str(e) or "hipError" in str(e) or "illegal memory" in str(e)):
                raise      # nothing more is started on the device
        printed = text.getvalue()
        entry.update(calls=list(rec.calls) if rec is not None else [], n_lines=printed.count("\r"), lines_sha256=sha(printed.encode()),
                     values=json.loads(json.dumps(vals, default=lambda v: np.asarray(v).tolist())) if vals is not None else None,
                     state_sha256=sha(value_bytes(vals), *(state_bytes(net, opt) if net is not None else [])))
        res["scenarios"][name] = entry
        print(name, entry.get("error", "ok"), file=sys.stderr, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write('{"device": %s, "torch": %s, "scenarios": {\n' % (json.dumps(res["device"]), json.dumps(res["torch"])))
        f.write(",\n".join(" %s: %s" % (json.dumps(k), json.dumps(v)) for k, v in res["scenarios"].items()) + "\n}}\n")


def diff(a_path, b_path, out_path):
    A, B = (json.load(open(p)) for p in (a_path, b_path))
    sa, sb = A["scenarios"], B["scenarios"]
    differ = [n for n in sorted(set(sa) | set(sb)) if sa.get(n) != sb.get(n)]
    res = {"a": os.path.basename(a_path), "b": os.path.basename(b_path), "device": [A["device"], B["device"]], "n_scenarios": len(sa),
           "n_raised": sum("error" in v for v in sa.values()), "native_calls": sum(len(v["calls"]) for v in sa.values()),
           "identical": not differ and A["device"] == B["device"] and len(sa) > 0, "scenarios_that_differ": differ}
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    json.dump(res, open(out_path, "w"), indent=1)
    print(json.dumps(res))
    return 0 if res["identical"] else 1


def code_lines(path):
    """Lines that hold code: no blanks, no comments, no docstrings (a string that is a statement of its own)."""
    lines, prev = set(), tokenize.NEWLINE
    with open(path, "rb") as f:
        for tok in tokenize.tokenize(f.readline):
            if tok.type in (tokenize.COMMENT, tokenize.NL, tokenize.NEWLINE, tokenize.ENCODING, tokenize.ENDMARKER):
                if tok.type == tokenize.NEWLINE:
                    prev = tokenize.NEWLINE
                continue
            if tok.type in (tokenize.INDENT, tokenize.DEDENT):
                continue
            if tok.type == tokenize.STRING and prev == tokenize.NEWLINE and tok.line.strip().startswith(('"', "'", 'r"', "r'")):
                prev = tokenize.STRING     # a docstring: the NEWLINE after it resets `prev`
                continue
            prev = tok.type
            lines.update(range(tok.start[0], tok.end[0] + 1))
    return len(lines)


def count_lines(parent, new, out_path):
    files = ("dsmil-wsi_amd/training.py", "dsmil-wsi_amd/modules.py")
    res = {"what": "lines that hold code (blank lines, comments and docstrings excluded)",
           "before": {f: code_lines(os.path.join(parent, f)) for f in files}, "after": {f: code_lines(os.path.join(new, f)) for f in files}}
    res["sum_before"], res["sum_after"] = sum(res["before"].values()), sum(res["after"].values())
    res["change"] = res["sum_after"] - res["sum_before"]
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    json.dump(res, open(out_path, "w"), indent=1)
    print(json.dumps(res))
    return 0


def loop(out_path, n_bags=64, rows=10000, K=512, epochs=20, warmup=3):
    """ms per bag of training.train with the progress line on, bags resident in the cache (no load, no split per step)."""
    import time
    import numpy as np
    import torch
    import dsmil  # noqa: F401
    from dsmil_wsi_amd import training as T
    from dsmil_wsi_amd.synthetic import VARIANT, build_net
    C, res = VARIANT["tcga"][1], {}
    g = torch.Generator(device="cuda").manual_seed(77)
    cache = T.BagCache("cuda", K)
    for b in range(n_bags):
        label = torch.zeros(1, C, device="cuda")
        label[0, b % C] = 1.0
        cache.store["bag%d" % b] = (torch.randn((rows, K), generator=g, device="cuda"), label)
    for per_step in (1, 8):
        net = build_net("tcga", "cuda").train()
        opt = torch.optim.Adam(net.parameters(), lr=1e-4, betas=(0.5, 0.9), weight_decay=1e-3)
        args = argparse.Namespace(feats_size=K, num_classes=C, dropout_patch=0.0, bags_per_step=per_step)
        np.random.seed(0)
        times = []
        for epoch in range(warmup + epochs):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            with contextlib.redirect_stdout(io.StringIO()):
                T.train(args, list(cache.store), net, torch.nn.BCEWithLogitsLoss(), opt, cache=cache, log=True)
            torch.cuda.synchronize()
            if epoch >= warmup:
                times.append((time.perf_counter() - t0) / n_bags * 1e3)
        res["train_log_per_step%d_ms_per_bag" % per_step] = statistics.median(times)
    json.dump(res, open(out_path, "w"))


def time_legs(tree, timeout):
    """One fresh process per leg of ``tree``, each with the tree's own scripts: {leg: ms (lower is faster)}."""
    legs = {}

    def run(*cmd):
        r = subprocess.run([sys.executable] + list(cmd), cwd=tree, capture_output=True, text=True, timeout=timeout)
        if r.returncode != 0:
            raise SystemExit(" ".join(cmd) + " failed (%d):\n" % r.returncode + r.stdout[-2000:] + r.stderr[-4000:])
        return r.stdout

    def last_json(text):
        return json.loads([ln for ln in text.splitlines() if ln.startswith("{")][-1])
    tb = last_json(run("tools/train_bench.py", "--steps", "200"))
    legs.update({"train_bench:" + k: tb[k] for k in ("train_step_native_ms", "train_step_dense_ms")})
    tm = last_json(run("tools/train_mil_time.py", "--json", "--epochs", "30"))
    legs.update({"train_mil_time:%s_ms_per_epoch" % k: tm[k]["median_s_per_epoch"] * 1e3 for k in ("native", "generic")})
    b = last_json(run("bench.py", "--gpus", "1", "--steps", "200", "--warmup", "50", "--full", "--workload", "train", "--no-cpu-baseline"))
    # (without the headline leg the line IS the first leg, train_c1)
    legs.update({"bench:train_c1_ms_per_step": 1e3 / b["value"], "bench:train_c2_ms_per_step": 1e3 / b["train_c2"]["value"]})
    with tempfile.TemporaryDirectory() as d:
        run(os.path.join("tools", "train_glue_check.py"), "loop", "--out", os.path.join(d, "l.json"))
        legs.update({"train_loop:" + k: v for k, v in json.load(open(os.path.join(d, "l.json"))).items()})
    return legs


def time_trees(parent, new, repeats, timeout, out_path):
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    runs = {"parent": [], "new": []}
    for i in range(repeats):
        for side in (("parent", "new") if i % 2 == 0 else ("new", "parent")):
            runs[side].append(time_legs(os.path.abspath(parent if side == "parent" else new), timeout))
            print(i, side, "ok", flush=True)
            json.dump({"partial_runs": runs}, open(out_path, "w"), indent=1)   # (a run cut short still leaves what it measured)
    r4 = lambda v: round(v, 5)   # noqa: E731
    legs = {}
    for leg in runs["parent"][0]:
        pv, nv = [r[leg] for r in runs["parent"]], [r[leg] for r in runs["new"]]
        pm, nm = statistics.median(pv), statistics.median(nv)
        legs[leg] = {"parent": [r4(v) for v in pv], "new": [r4(v) for v in nv], "parent_median": r4(pm), "new_median": r4(nm),
                     "new_median_above_parent_slowest": nm > max(pv), "parent_scatter_exceeds_difference": max(pv) - min(pv) > abs(nm - pm)}
    res = {"unit": "ms, lower is faster", "repeats": repeats, "order": "parent first in even repeats, new first in odd",
           "legs_above_parent_slowest": [k for k, v in legs.items() if v["new_median_above_parent_slowest"]], "legs": legs}
    with open(out_path, "w") as f:
        f.write(json.dumps({k: v for k, v in res.items() if k != "legs"}, indent=1)[:-2] + ',\n "legs": {\n')
        f.write(",\n".join("  %s: %s" % (json.dumps(k), json.dumps(v)) for k, v in legs.items()) + "\n }\n}\n")
    print(json.dumps(res["legs_above_parent_slowest"]))
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=("run", "diff", "lines", "time", "loop"))
    ap.add_argument("paths", nargs="*")
    ap.add_argument("--device", default="cpu", choices=("cpu", "cuda"))
    ap.add_argument("--tree", default=os.path.dirname(HERE))
    ap.add_argument("--trees", nargs=2, metavar=("PARENT", "NEW"))
    ap.add_argument("--out", required=True)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--timeout", type=int, default=300, help="seconds per child process")
    a = ap.parse_args()
    if a.mode == "diff":
        return diff(*a.paths, a.out)
    if a.mode == "lines":
        return count_lines(*a.trees, a.out)
    if a.mode == "time":
        return time_trees(*a.trees, a.repeats, a.timeout, a.out)
    sys.path.insert(0, os.path.abspath(a.tree))
    if a.mode == "loop":
        return loop(a.out)
    run_all(a.device, a.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
