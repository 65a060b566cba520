#!/usr/bin/env python
"""One-off check that a change of the Python around an embedding pass (dsmil-wsi_amd/pipeline.py, ops.StreamPool) left the
stream program, the native calls and the bits alone: a fixed list of seeded scenarios, run on whichever tree is named, once on
the parent commit's and once on the new one's, and the two records compared.

    python tools/embed_pipeline_check.py run --device cpu|cuda [--tree DIR] --out A.json
        every scenario in ONE process.  Per scenario an ordered trace: every Stream.wait_event / wait_stream, Event.record /
        synchronize, Tensor.record_stream and entry into torch.cuda.stream(s), each with the current stream and the stream or
        event it names (streams and events numbered by first appearance in the scenario; what torch calls inside one of these
        is not listed again); every native work entry (a recording proxy around ``_native.lib()``, size queries left out;
        entries called from reader threads are counted, not ordered); every classifier forward with its batch shape.  And the
        SHA-256 of every returned tensor or array and the ``stats`` dict.  On ``cpu`` the scenarios that need device streams are
        left out and the traces hold native and forward entries only.  On ``cuda`` the process ends at the first HIP error.
    python tools/embed_pipeline_check.py diff A.json B.json --out profiles/embed_pipeline/diff_cuda.json
    python tools/embed_pipeline_check.py lines --trees PARENT NEW --out profiles/embed_pipeline/lines.json
        code lines (comments, docstrings and blanks excluded) of pipeline.py and of ops.StreamPool in both trees, the loops of
        _embed_jpeg_chunks and embed_files, and who touches free_ev / bufs / dss outside _ChunkDecoder
    python tools/embed_pipeline_check.py time --trees PARENT NEW [--repeats 5] --out profiles/embed_pipeline/times.json
        each tree's own bench.py legs (slide, slide_h2d, slide_jpeg, e2e) and this file's ``files`` mode, in fresh processes, one
        at a time, alternating between the two trees (parent first in even repeats, new first in odd ones); per leg every run of
        both, both medians and whether the new median lies above the parent's slowest run
    python tools/embed_pipeline_check.py files --dir D [--tree DIR] --out F.json
        embed_files(gpu_decode=True) over the JPEG files of D, without and with bg_threshold=15: median ms of three passes
"""
import argparse
import ast
import hashlib
import json
import os
import statistics
import subprocess
import sys
import tempfile
import threading
import tokenize

HERE = os.path.dirname(os.path.abspath(__file__))
QUERIES = ("_bytes", "_route", "_form", "_query", "_grid", "_rows_per", "_version", "_strerror", "_cus", "_tile_rows", "_size")


class Trace:
    """The ordered record of one scenario."""

    def __init__(self):
        self.reset()

    def reset(self):
        self.ops, self.off_thread, self.streams, self.events, self.keep, self.depth = [], {}, {}, {}, [], 0

    def stream(self, s):
        return "s%d" % self.streams.setdefault((s.device.index, s.cuda_stream), len(self.streams))

    def event(self, e):
        if id(e) not in self.events:
            self.events[id(e)] = len(self.events)
            self.keep.append(e)            # (alive until the scenario ends: no second event at the same address)
        return "e%d" % self.events[id(e)]

    def current(self):
        import torch
        return self.stream(torch.cuda.current_stream()) if torch.cuda.is_available() else "-"

    def add(self, *what):
        if threading.current_thread() is not threading.main_thread():
            self.off_thread[what[0]] = self.off_thread.get(what[0], 0) + 1
        else:
            self.ops.append(" ".join(str(w) for w in what))


TRACE = Trace()


def hook(cls, name, describe):
    """Record the outermost calls of cls.name (torch builds wait_stream out of record + wait_event: not listed again)."""
    real = getattr(cls, name)

    def wrapper(self, *args, **kwargs):
        if TRACE.depth == 0:
            TRACE.add("on", TRACE.current(), cls.__name__ + "." + name, *describe(self, *args, **kwargs))
        TRACE.depth += 1
        try:
            return real(self, *args, **kwargs)
        finally:
            TRACE.depth -= 1
    setattr(cls, name, wrapper)


def install_stream_hooks():
    import torch
    T = TRACE
    hook(torch.cuda.Stream, "wait_event", lambda s, e: (T.stream(s), T.event(e)))
    hook(torch.cuda.Stream, "wait_stream", lambda s, o: (T.stream(s), T.stream(o)))
    hook(torch.cuda.Event, "record", lambda e, s=None: (T.event(e), T.stream(s) if s is not None else T.current()))
    hook(torch.cuda.Event, "synchronize", lambda e: (T.event(e),))
    hook(torch.Tensor, "record_stream", lambda t, s: (str(t.dtype), tuple(t.shape), T.stream(s)))
    hook(torch.cuda.StreamContext, "__enter__", lambda c: (T.stream(c.stream) if c.stream is not None else "-",))


class Recorder:
    def __init__(self, real):
        self._real = real

    def __getattr__(self, name):
        fn = getattr(self._real, name)
        if not callable(fn) or name.endswith(QUERIES):
            return fn

        def call(*args):
            main = threading.current_thread() is threading.main_thread()
            TRACE.add(*(("native", name, "on", TRACE.current()) if main else (name,)))
            return fn(*args)
        return call


def watch(ic, tag):
    ic.register_forward_pre_hook(lambda m, inp: TRACE.add("forward", tag, str(inp[0].dtype), tuple(inp[0].shape), "on", TRACE.current()))
    return ic


def sha(v):
    """SHA-256 of a returned value: tensors / arrays as dtype, shape and bytes; sequences element by element; dicts sorted."""
    import numpy as np
    import torch
    h = hashlib.sha256()

    def feed(x):
        if torch.is_tensor(x):
            x = x.detach().cpu().contiguous().numpy()
        if isinstance(x, np.ndarray):
            h.update(str(x.dtype).encode() + str(x.shape).encode() + np.ascontiguousarray(x).tobytes())
        elif isinstance(x, (list, tuple)):
            h.update(b"[")
            for y in x:
                feed(y)
            h.update(b"]")
        elif isinstance(x, dict):
            feed([(k, x[k]) for k in sorted(x)])
        else:
            h.update(repr(x).encode())
    feed(v)
    return h.hexdigest()


def scenarios(device, tmp):
    """name -> callable returning the values whose bits are compared."""
    import numpy as np
    import torch
    from test_jpeg_gpu import _img, _jpeg, _pil
    from test_resnet_gpu import _build
    from dsmil_wsi_amd import pipeline as pl
    cuda = device == "cuda"
    out = {}
    ic = watch(_build(seed=13)[0].to(device), "ic")
    low, high = watch(_build(seed=17)[0].to(device), "low"), watch(_build(seed=19)[0].to(device), "high")

    rng = np.random.default_rng(47)
    blobs = [_jpeg(_img(rng, 96, 96, i % 3), quality=70, progressive=i in (5, 22, 23, 49) or 28 <= i < 32) for i in range(51)]

    def jpeg_blobs(n, ahead, nst, streams):
        def run():
            old = pl.DECODE_AHEAD[0], pl.DECODE_STREAMS[0]
            pl.DECODE_AHEAD[0], pl.DECODE_STREAMS[0] = ahead, nst
            try:
                st = {}
                f, c = pl.embed_jpeg_blobs(ic, blobs[:n], batch_size=4, decode_batch=4, streams=streams, device=device, stats=st)
                return [f, c, st]
            finally:
                pl.DECODE_AHEAD[0], pl.DECODE_STREAMS[0] = old
        return run
    if cuda:
        for streams in (3, 1):
            for ahead, nst in ((1, 1), (2, 2), (3, 2), (3, 1)):
                out["jpeg_blobs_51_ahead%d_dec%d_streams%d" % (ahead, nst, streams)] = jpeg_blobs(51, ahead, nst, streams)
        out["jpeg_blobs_3_streams3"], out["jpeg_blobs_3_streams1"] = jpeg_blobs(3, 3, 2, 3), jpeg_blobs(3, 3, 2, 1)
        out["jpeg_blobs_0"] = jpeg_blobs(0, 3, 2, 3)

    rng = np.random.default_rng(31)
    files = []
    for i in range(29):
        a = _img(rng, 96, 96, i % 4) if i % 4 < 3 else np.full((96, 96, 3), 200 + rng.integers(0, 40), np.uint8)
        files.append(os.path.join(tmp, "%d_%d.jpeg" % (i, i + 1)))
        with open(files[-1], "wb") as fh:
            fh.write(_jpeg(a, quality=70))

    def embed_files(n=29, **kw):
        def run():
            old = pl.DECODE_BATCH[0]
            pl.DECODE_BATCH[0] = 8
            try:
                return list(pl.embed_files(ic, files[:n], batch_size=4, num_workers=2 if kw.get("gpu_decode") else 0, device=device, **kw))
            finally:
                pl.DECODE_BATCH[0] = old
        return run
    out["files_loader"] = embed_files(gpu_decode=False)
    out["files_gpu_decode"] = embed_files(gpu_decode=True)
    out["files_gpu_decode_filter_keep"] = embed_files(gpu_decode=True, bg_threshold=15, return_keep=True)
    out["files_loader_filter"] = embed_files(gpu_decode=False, bg_threshold=15)
    out["files_position"] = embed_files(gpu_decode=False, want_position=True)
    out["files_none"] = embed_files(n=0, gpu_decode=True)

    tiles = torch.from_numpy(np.stack([_pil(b) for b in blobs[:23]]))

    def embed_tiles(t, bs, streams):
        return lambda: list(pl.embed_tiles(ic, t(), bs, streams=streams, device=device))
    for streams in (1, 3):
        out["tiles_device_streams%d" % streams] = embed_tiles(lambda: tiles.to(device), 4, streams)
    if cuda:
        out["tiles_pinned_host_streams3"] = embed_tiles(lambda: tiles.pin_memory(), 4, 3)
    out["tiles_one_batch"] = embed_tiles(lambda: tiles.to(device), 32, 3)
    out["tiles_none"] = embed_tiles(lambda: tiles[:0].to(device), 4, 3)

    g = torch.Generator().manual_seed(5)

    def bag(tile, streams, contiguous):   # 3 x 2 low tiles, factor 2; not contiguous: the gathers without 8-byte words
        wsi = torch.randint(0, 256, (3 * 2 * tile, 2 * 2 * tile + (not contiguous), 3), generator=g, dtype=torch.uint8)
        return lambda: list(pl.multiscale_bag(wsi.to(device)[:, :2 * 2 * tile], low, high, "cat", tile=tile, factor=2, batch_size=8, streams=streams))
    for tile in (32, 64):                 # (64: a 2 x 2 map in layer4 — torch's instance_norm, the trunk of a CPU run, refuses 1 x 1)
        for streams in (3, 1):
            out["multiscale_tile%d_streams%d" % (tile, streams)] = bag(tile, streams, True)
            out["multiscale_tile%d_noncontiguous_streams%d" % (tile, streams)] = bag(tile, streams, False)
    return out


def run_all(device, tree, out_path):
    import numpy as np
    import torch
    import dsmil  # noqa: F401  (registers the tree's package)
    from dsmil_wsi_amd import _native, pipeline
    assert os.path.samefile(os.path.dirname(os.path.dirname(pipeline.__file__)), tree), "the package of another tree was imported"
    rec = Recorder(_native.lib())
    _native.lib = lambda: rec
    if device == "cuda":
        install_stream_hooks()
    res = {}
    with tempfile.TemporaryDirectory() as tmp:
        for name, run in scenarios(device, tmp).items():
            torch.manual_seed(1234)
            np.random.seed(1234)
            TRACE.reset()
            entry = {}
            try:
                vals = run()
                if device == "cuda":
                    torch.cuda.synchronize()
                entry["sha256"] = [sha(v) for v in vals]
            except Exception as e:  # noqa: BLE001  (a scenario both trees refuse alike is a result too)
                entry["error"] = "%s: %s" % (type(e).__name__, str(e)[:200])
                if device == "cuda" and ("HIP error" in str(e) or "hipError" in str(e) or "illegal memory" in str(e)):
                    raise      # nothing more is started on the device
            entry.update(off_thread_native=dict(sorted(TRACE.off_thread.items())), trace=list(TRACE.ops))
            res[name] = entry
            print(name, entry.get("error", "ok"), len(entry["trace"]), "ops", file=sys.stderr, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write('{"device": %s, "torch": %s, "scenarios": {\n' % (json.dumps(device), json.dumps(torch.__version__)))
        f.write(",\n".join(" %s: %s" % (json.dumps(k), json.dumps(v)) for k, v in res.items()) + "\n}}\n")


def diff(a_path, b_path, out_path):
    A, B = (json.load(open(p)) for p in (a_path, b_path))
    sa, sb = A["scenarios"], B["scenarios"]
    differ = [n for n in sorted(set(sa) | set(sb)) if sa.get(n) != sb.get(n)]
    res = {"a": os.path.basename(a_path), "b": os.path.basename(b_path), "device": [A["device"], B["device"]], "n_scenarios": len(sa),
           "n_raised": sum("error" in v for v in sa.values()), "trace_entries": sum(len(v["trace"]) for v in sa.values()),
           "values_hashed": sum(len(v.get("sha256", ())) for v in sa.values()),
           "identical": not differ and A["device"] == B["device"] and len(sa) > 0, "scenarios_that_differ": differ,
           "scenarios": {n: {"trace_entries": len(v["trace"]), "trace_sha256": hashlib.sha256("\n".join(v["trace"]).encode()).hexdigest(),
                             "sha256": v.get("sha256"), "error": v.get("error")} for n, v in sa.items()}}
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    json.dump(res, open(out_path, "w"), indent=1)
    print(json.dumps({k: v for k, v in res.items() if k != "scenarios"}))
    return 0 if res["identical"] else 1


def code_lines(path, first=1, last=None):
    """Lines of [first, last] that hold code: no blanks, no comments, no docstrings (a string that is a statement of its own)."""
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
    return len([n for n in lines if n >= first and (last is None or n <= last)])


def tree_lines(tree):
    pipe, ops = os.path.join(tree, "dsmil-wsi_amd", "pipeline.py"), os.path.join(tree, "dsmil-wsi_amd", "ops.py")
    pool = next(n for n in ast.parse(open(ops).read()).body if isinstance(n, ast.ClassDef) and n.name == "StreamPool")
    mod = ast.parse(open(pipe).read())
    funcs = {n.name: n for n in mod.body if isinstance(n, ast.FunctionDef)}

    def loops(fn):   # for / while statements of the function itself (comprehensions and nested functions left out)
        def walk(node):
            n = 0
            for c in ast.iter_child_nodes(node):
                if isinstance(c, (ast.FunctionDef, ast.Lambda)):
                    continue
                n += isinstance(c, (ast.For, ast.While)) + walk(c)
            return n
        return walk(fn)
    batch_loops = [n for n in ast.walk(funcs["embed_files"]) if isinstance(n, ast.For) and isinstance(n.target, ast.Name) and n.target.id == "batch"]
    outside = sorted({"%s:%d" % (n.attr, n.lineno) for top in mod.body if not (isinstance(top, ast.ClassDef) and top.name == "_ChunkDecoder")
                      for n in ast.walk(top) if isinstance(n, ast.Attribute) and n.attr in ("free_ev", "bufs", "dss")})
    top_loops = [n for n in funcs["_embed_jpeg_chunks"].body if isinstance(n, (ast.For, ast.While))] + \
                [c for n in funcs["_embed_jpeg_chunks"].body if isinstance(n, ast.If) for c in n.body if isinstance(c, (ast.For, ast.While))]
    chunk_loops = [n for n in top_loops if any(isinstance(c, (ast.For, ast.While)) for c in ast.walk(n) if c is not n) or
                   any(isinstance(c, ast.Attribute) and c.attr in ("decode", "acquire", "end", "decoded") for c in ast.walk(n))]
    return {"pipeline.py": code_lines(pipe), "ops.StreamPool": code_lines(ops, pool.lineno, pool.end_lineno),
            "_embed_jpeg_chunks_loops_over_chunks": len(chunk_loops), "_embed_jpeg_chunks_loop_statements": loops(funcs["_embed_jpeg_chunks"]),
            "embed_files_batch_loops": len(batch_loops),
            "embed_files_decisions_naming_gpu_decode": sum(isinstance(n, (ast.If, ast.IfExp)) and any(isinstance(c, ast.Name) and c.id == "gpu_decode" for c in ast.walk(n.test))
                                                          and not any(isinstance(c, ast.Constant) and c.value is None for c in ast.walk(n.test)) for n in ast.walk(funcs["embed_files"])),
            "free_ev_bufs_dss_outside_ChunkDecoder": outside}


def count_lines(parent, new, out_path):
    res = {"what": "lines that hold code (blank lines, comments and docstrings excluded)", "before": tree_lines(parent), "after": tree_lines(new)}
    for k in ("before", "after"):
        res["sum_" + k] = res[k]["pipeline.py"] + res[k]["ops.StreamPool"]
    res["change"] = res["sum_after"] - res["sum_before"]
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    json.dump(res, open(out_path, "w"), indent=1)
    print(json.dumps(res))
    return 0


def files_leg(folder, out_path, passes=3):
    """ms of embed_files(gpu_decode=True) over a folder of JPEG tiles, plain and with the background filter."""
    import time
    import torch
    import bench
    import dsmil  # noqa: F401
    from dsmil_wsi_amd import pipeline as pl
    cx = type("C", (), {})()
    cx.torch, cx.dev = torch, torch.device("cuda", 0)
    ic = bench._build_iclassifier(cx)
    files = sorted(os.path.join(folder, f) for f in os.listdir(folder))
    res = {}
    for key, kw in (("embed_files_gpu_decode_ms", {}), ("embed_files_gpu_decode_filter_ms", {"bg_threshold": 15})):
        times = []
        for i in range(passes + 1):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            pl.embed_files(ic, files, batch_size=256, num_workers=4, gpu_decode=True, **kw)
            torch.cuda.synchronize()
            if i:       # (the first pass warms the allocator and the page cache)
                times.append((time.perf_counter() - t0) * 1e3)
        res[key] = statistics.median(times)
    json.dump(res, open(out_path, "w"))


def time_legs(tree, folder, timeout):
    """One fresh process at a time, each with the tree's own scripts: {leg: ms (lower is faster)}."""
    def run(*cmd):
        r = subprocess.run([sys.executable] + list(cmd), cwd=tree, capture_output=True, text=True, timeout=timeout)
        if r.returncode != 0:
            raise SystemExit(" ".join(cmd) + " failed (%d):\n" % r.returncode + r.stdout[-2000:] + r.stderr[-4000:])
        return r.stdout
    b = json.loads([ln for ln in run("bench.py", "--gpus", "1", "--steps", "5", "--warmup", "1", "--full", "--workload",
                                     "slide,slide_h2d,slide_jpeg,e2e", "--no-cpu-baseline").splitlines() if ln.startswith("{")][-1])
    # (without the headline leg the line IS the first leg, slide)
    legs = {"bench:slide_ms": b["ms_per_slide"], "bench:slide_h2d_ms": b["slide_h2d"]["ms_per_slide"],
            "bench:slide_jpeg_ms": b["slide_jpeg"]["ms_per_slide"], "bench:e2e_ms": b["e2e"]["ms_per_slide"]}
    with tempfile.TemporaryDirectory() as d:
        run(os.path.abspath(__file__), "files", "--tree", tree, "--dir", folder, "--out", os.path.join(d, "f.json"))
        legs.update(json.load(open(os.path.join(d, "f.json"))))
    return legs


def time_trees(parent, new, repeats, timeout, out_path):
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    sys.path.insert(0, os.path.abspath(new))
    import bench
    runs = {"parent": [], "new": []}
    with tempfile.TemporaryDirectory() as folder:
        for i, blob in enumerate(bench._jpeg_tiles(10000)):          # written once, read by every run of both trees
            with open(os.path.join(folder, "%d_%d.jpeg" % (i // 100, i % 100)), "wb") as fh:
                fh.write(blob)
        for i in range(repeats):
            for side in (("parent", "new") if i % 2 == 0 else ("new", "parent")):
                runs[side].append(time_legs(os.path.abspath(parent if side == "parent" else new), folder, timeout))
                print(i, side, runs[side][-1], flush=True)
                json.dump({"partial_runs": runs}, open(out_path, "w"), indent=1)   # (a run cut short still leaves what it measured)
    r4 = lambda v: round(v, 4)   # noqa: E731
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
    ap.add_argument("mode", choices=("run", "diff", "lines", "time", "files"))
    ap.add_argument("paths", nargs="*")
    ap.add_argument("--device", default="cpu", choices=("cpu", "cuda"))
    ap.add_argument("--tree", default=os.path.dirname(HERE))
    ap.add_argument("--trees", nargs=2, metavar=("PARENT", "NEW"))
    ap.add_argument("--dir")
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
    for sub in ("oracle", "tests", ""):
        sys.path.insert(0, os.path.join(os.path.abspath(a.tree), sub).rstrip(os.sep))
    if a.mode == "files":
        return files_leg(a.dir, a.out)
    run_all(a.device, a.tree, a.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
