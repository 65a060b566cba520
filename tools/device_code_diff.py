#!/usr/bin/env python
"""Is the device code of one translation unit, or of a set of them, the same in two trees?  For a change that claims
"host code only", or that moves kernels between units.

    python tools/device_code_diff.py <parent tree> <new tree> dsmil-wsi_amd/csrc/agg_bwd.hip [more units ...]
                                     [--new-files unit ...] [--allow-missing k_name ...] [--out F.json]

The units named first are the parent's; --new-files names the new tree's where the set differs (default: the same).  A
side's symbols are the union over its units, and a symbol that two units of one side emit is reported (`emitted_twice`).
Compiles every unit device-only device-only to assembly with build.py's flags (--cuda-device-only -S), once as the
product and once with -DDSMIL_EXPERIMENTS, and compares per kernel symbol: the symbol sets and every symbol's
instruction stream, with comments, assembler directives and the numbering of local labels taken out (they move with
the line numbers of the source).  It compares only: it reads no instruction's meaning and looks for nothing.
--allow-missing names kernels that may be absent from the new tree's unit.  No GPU needed."""
import argparse
import importlib.util
import json
import os
import re
import subprocess
import sys
import tempfile


def build_flags(tree):
    spec = importlib.util.spec_from_file_location("_b", os.path.join(tree, "dsmil-wsi_amd", "build.py"))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    return b.HIPCC, b.BASE_FLAGS


def assembly(tree, rel, extra):
    hipcc, flags = build_flags(tree)
    with tempfile.TemporaryDirectory() as d:
        out = os.path.join(d, "unit.s")
        subprocess.check_call([hipcc] + flags + list(extra) + ["--cuda-device-only", "-S", os.path.join(tree, rel), "-o", out])
        return open(out).read()


def kernels(asm):
    """{symbol: [normalised instruction lines]} for every kernel (.amdhsa_kernel) and every other function of the unit
    that holds instructions."""
    names = set(re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", asm, re.M))
    out, cur, labels = {}, None, {}
    for line in asm.splitlines():
        line = re.sub(r"\s*(;|//).*$", "", line).strip()
        if not line:
            continue
        if line.startswith(".amdgpu_metadata"):
            break       # the unit's metadata note (YAML) follows the code
        m = re.match(r"^([A-Za-z_.$][\w.$]*):$", line)
        if m:
            if not m.group(1).startswith(".L"):     # a global symbol: a kernel, a function or data
                cur, labels = m.group(1), {}
                out[cur] = []
            elif cur is not None:                   # a local label: numbered by first appearance inside its symbol
                out[cur].append(labels.setdefault(m.group(1), f".L#{len(labels)}") + ":")
            continue
        if cur is None or (line.startswith(".") and not line.startswith(".amdhsa_")):
            continue   # directives (.p2align, .loc, .cfi_*, .section ...); a kernel's descriptor (.amdhsa_*: registers, LDS) is kept
        out[cur].append(re.sub(r"\.L[\w.$]+", lambda t: labels.setdefault(t.group(0), f".L#{len(labels)}"), line))
    assert names and names <= set(out), "no kernels found in the assembly"
    return {k: v for k, v in out.items() if k in names or any(not s.endswith(":") for s in v)}


def side(tree, rels, extra):
    """The union of the units' symbols and the symbols that more than one unit emits."""
    out, twice = {}, []
    for rel in rels:
        k = kernels(assembly(tree, rel, extra))
        twice += sorted(set(k) & set(out))
        out.update(k)
    return out, twice


def compare(parent, new, rels, new_rels, extra, allow_missing):
    (a, twice_a), (b, twice_b) = side(parent, rels, extra), side(new, new_rels, extra)
    missing = sorted(set(a) - set(b))
    added = sorted(set(b) - set(a))
    differing = sorted(k for k in set(a) & set(b) if a[k] != b[k])
    excused = [k for k in missing if any(n in k for n in allow_missing)]
    return {"symbols_parent": len(a), "symbols_new": len(b),
            "instructions_parent": sum(len(v) for v in a.values()), "instructions_new": sum(len(v) for v in b.values()),
            "only_in_parent": missing, "only_in_new": added, "allowed_missing": excused,
            "symbol_sets_equal": not added and missing == excused,
            "emitted_twice_parent": twice_a, "emitted_twice_new": twice_b,
            "differing_instruction_streams": len(differing), "differing": differing}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("parent")
    ap.add_argument("new")
    ap.add_argument("files", nargs="+", help="paths of the .hip files relative to a tree's root")
    ap.add_argument("--new-files", nargs="+", default=None, metavar="FILE", help="the new tree's units (default: the same)")
    ap.add_argument("--allow-missing", nargs="*", default=[], metavar="KERNEL")
    ap.add_argument("--out")
    a = ap.parse_args()
    new_files = a.new_files or a.files
    res = {"compile": "build.py's HIPCC + BASE_FLAGS [-DDSMIL_EXPERIMENTS] --cuda-device-only -S, per unit",
           "units_parent": a.files, "units_new": new_files,
           "product": compare(a.parent, a.new, a.files, new_files, [], a.allow_missing),
           "experiment": compare(a.parent, a.new, a.files, new_files, ["-DDSMIL_EXPERIMENTS"], a.allow_missing)}
    res["same_device_code"] = all(res[k]["symbol_sets_equal"] and not res[k]["differing_instruction_streams"] and
                                  not res[k]["emitted_twice_new"] and res[k]["symbols_new"] > 0
                                  for k in ("product", "experiment"))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        json.dump(res, open(a.out, "w"), indent=1)
    print(json.dumps({k: v for k, v in res.items() if k != "compile"}, indent=1))
    return 0 if res["same_device_code"] else 1


if __name__ == "__main__":
    sys.exit(main())
