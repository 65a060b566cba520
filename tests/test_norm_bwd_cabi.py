"""The norm backward entries (dsmil_norm_bwd*: csrc/norm_bwd.hip) are declared, exported and bound — additive, ABI still 6 —;
their size query, plan and refusals answer without a device (every check runs before the first launch, in the documented
order); and the plan of every case of tests/norm_bwd_cases.py is PINNED, so the chunk, run_len, lanes and n_partials the bars are
formed from are declarations, not results.  CPU only: no call here reaches a launch, the pointers are never read."""
import ctypes
import os
import re

import pytest

import norm_bwd_cases as nc
import dsmil  # noqa: F401  (registers the dsmil_wsi_amd package)
import dsmil_wsi_amd._native as nat
from dsmil_wsi_amd import ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("dsmil_norm_bwd_plan", "dsmil_norm_bwd_workspace_bytes", "dsmil_norm_bwd")
E_INVALID, E_UNSUPPORTED, E_WORKSPACE, E_ALIGN = -1, -2, -3, -5
RELU, ADD, DOWN = 0, 1, 2
BIG = 1 << 40
FIELDS = ("chunk", "n_partials", "run_len", "lanes", "n_sums", "grid_partial", "grid_finish", "grid_apply", "groups")


def test_norm_bwd_symbols_are_declared_exported_and_bound():
    text = open(os.path.join(ROOT, "include", "dsmil_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    lib = ctypes.CDLL(nat.LIB_PATH)
    for name in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, src), f"{name} is not declared in include/dsmil_hip.h"
        assert hasattr(lib, name), f"{name} is not exported"
        assert name in nat.SIGNATURES, f"{name} is not in the binding table"
    assert re.search(r"DSMIL_NORM_BWD_RELU = 0, DSMIL_NORM_BWD_ADD = 1, DSMIL_NORM_BWD_ADD_DOWN = 2", src)
    assert int(re.search(r"#define DSMIL_ABI_VERSION (\d+)", text).group(1)) == 6
    assert nat.lib().dsmil_abi_version() == 6
    assert ops.NORM_BWD_KINDS == {"relu": RELU, "add": ADD, "add_down": DOWN}


def test_the_plan_of_every_case_is_pinned():
    for name, kind, B, HW, C, _ in nc.CASES:
        p = ops.norm_backward_plan(kind, B, HW, C)
        assert tuple(p[f] for f in FIELDS) == nc.PLANS[name], (name, p)
        assert p["kind"] == kind and p["block"] == 256
        assert (p["chunk"], p["n_partials"], p["run_len"], p["lanes"]) == nc.plan_of(kind, B, HW, C)
        assert p["n_sums"] == (3 if kind == "add_down" else 2) and p["grid_partial"] == B * p["n_partials"]
        assert p["grid_apply"] == min(-(-B * HW // p["lanes"]), 8192) and p["groups"] == (2 if C == 2048 else 1)
    for name, kind, B, HW, C in nc.EXACT_CASES:
        assert ops.norm_backward_plan(kind, B, HW, C)["chunk"] == 256          # what the emulation of the exact cases assumes
    # the conditions the case names claim
    P = nc.PLANS
    assert P["r_256"][1] == 1 and P["a_257"][1] == 2 and min(P[n][1] for n in ("r_700", "a_600", "d_700")) >= 3
    assert P["r_2048"][3] == 1 and P["r_2048"][8] == 2 and P["r_35"][2] * P["r_35"][3] >= 35
    # the block shapes of ResNet-18 at 224 x 224: the chunk doubles while B x chunks exceeds 2048 workgroups
    for B, HW, C, chunk, parts in [(256, 3136, 64, 512, 7), (64, 3136, 64, 256, 13), (256, 784, 128, 256, 4), (256, 196, 256, 256, 1),
                                   (256, 49, 512, 256, 1)]:
        p = ops.norm_backward_plan("add", B, HW, C)
        assert (p["chunk"], p["n_partials"]) == (chunk, parts), p
    p = ops.norm_backward_plan("relu", 2, 1 << 22, 64)                          # and stops at 4096 pixels
    assert (p["chunk"], p["n_partials"], p["run_len"], p["grid_apply"]) == (4096, 1024, 256, 8192)


def test_norm_bwd_sizes_without_a_device():
    wb = nat.lib().dsmil_norm_bwd_workspace_bytes
    for name, kind, B, HW, C, _ in nc.CASES:
        chunk, parts, _, _, sums = nc.PLANS[name][:5]
        assert wb(ops.NORM_BWD_KINDS[kind], B, HW, C) >= sums * B * C * 4 * (parts + 1)
        assert wb(ops.NORM_BWD_KINDS[kind], B, HW, C) % 256 == 0
        assert ops.norm_backward_supported(kind, B, HW, C)
    assert wb(3, 2, 35, 64) == 0 and wb(-1, 2, 35, 64) == 0 and wb(RELU, 0, 35, 64) == 0 and wb(RELU, 2, 0, 64) == 0


REFUSED = [(2, 35, 6), (2, 35, 66), (2, 35, 96), (2, 35, 40), (2, 35, 1536), (2, 35, 4096), (2, 35, 2052),   # C
           (4, 1 << 20, 512), (1 << 20, 1, 2048)]                                                        # B HW C >= 2^31


def test_norm_bwd_refusals_without_a_device():
    L = nat.lib()
    p = ctypes.c_void_p
    # addresses far enough apart that no two maps of the shapes below overlap; nothing here is ever dereferenced
    G, O, Y, M, R, YD, MD, RD, GY, GYD, GRES, WS = (p((i + 1) << 44) for i in range(12))
    N = None
    plan = (ctypes.c_int32 * 16)()
    cp, wb, nb = L.dsmil_norm_bwd_plan, L.dsmil_norm_bwd_workspace_bytes, L.dsmil_norm_bwd
    ok = (2, 35, 64)
    assert cp(RELU, *ok, None) == E_INVALID and cp(3, *ok, plan) == E_INVALID and cp(-1, *ok, plan) == E_INVALID
    assert cp(RELU, 0, 35, 64, plan) == E_INVALID and cp(RELU, 2, -1, 64, plan) == E_INVALID and cp(RELU, 2, 35, 0, plan) == E_INVALID
    assert cp(RELU, *ok, plan) == 0

    # (kind, g, out, y, mean, rstd, yd, md, rd, gy, gyd, gres, B, HW, C, ws, ws_bytes, stream)
    relu = lambda **k: _call(nb, RELU, dict(g=G, out=N, y=Y, mean=M, rstd=R, yd=N, md=N, rd=N, gy=GY, gyd=N, gres=N, ws=WS), ok, k)
    add = lambda **k: _call(nb, ADD, dict(g=G, out=O, y=Y, mean=M, rstd=R, yd=N, md=N, rd=N, gy=GY, gyd=N, gres=GRES, ws=WS), ok, k)
    down = lambda **k: _call(nb, DOWN, dict(g=G, out=O, y=Y, mean=M, rstd=R, yd=YD, md=MD, rd=RD, gy=GY, gyd=GYD, gres=N, ws=WS), ok, k)
    # a short workspace is the LAST check: the complete calls get that far
    assert relu(ws_bytes=0) == E_WORKSPACE and add(ws_bytes=0) == E_WORKSPACE and down(ws_bytes=0) == E_WORKSPACE
    for kind, call in ((RELU, relu), (ADD, add), (DOWN, down)):
        assert call(ws_bytes=wb(kind, *ok) - 1) == E_WORKSPACE
        for need in ("g", "y", "mean", "rstd", "gy", "ws"):                          # pointers every kind needs
            assert call(**{need: N}) == E_INVALID, (kind, need)
        assert call(shape=(0, 35, 64)) == E_INVALID and call(shape=(2, 0, 64)) == E_INVALID and call(shape=(2, 35, -4)) == E_INVALID
    assert _call(nb, 3, dict(g=G, out=N, y=Y, mean=M, rstd=R, yd=N, md=N, rd=N, gy=GY, gyd=N, gres=N, ws=WS), ok, {}) == E_INVALID
    # pointers the kind forbids, or needs
    for forbidden in ("out", "yd", "md", "rd", "gyd", "gres"):
        assert relu(**{forbidden: O}) == E_INVALID, forbidden
    for forbidden in ("yd", "md", "rd", "gyd"):
        assert add(**{forbidden: YD}) == E_INVALID, forbidden
    assert add(out=N) == E_INVALID and add(gres=N) == E_INVALID
    assert down(gres=GRES) == E_INVALID
    for need in ("out", "yd", "md", "rd", "gyd"):                                    # half-given pointers
        assert down(**{need: N}) == E_INVALID, need
    # an output aliasing an input or another output: the same pointer, or an overlapping range
    nbytes = 2 * 35 * 64 * 4
    assert relu(gy=G) == E_INVALID and relu(gy=Y) == E_INVALID and relu(gy=M) == E_INVALID
    assert relu(gy=p(G.value + nbytes - 16)) == E_INVALID and relu(gy=p(G.value - nbytes + 16)) == E_INVALID
    assert relu(gy=p(G.value + nbytes), ws_bytes=0) == E_WORKSPACE                    # adjacent is not aliasing
    assert relu(gy=p(R.value + 2 * 64 * 4 - 16)) == E_INVALID
    assert add(gres=G) == E_INVALID and add(gres=O) == E_INVALID and add(gres=GY) == E_INVALID and add(gy=O) == E_INVALID
    assert down(gyd=YD) == E_INVALID and down(gyd=GY) == E_INVALID and down(gy=YD) == E_INVALID and down(gyd=RD) == E_INVALID
    # INVALID comes before UNSUPPORTED, UNSUPPORTED before ALIGN, ALIGN before WORKSPACE
    odd = lambda q: p(q.value + 4)
    for shape in REFUSED:
        for kind, call in ((RELU, relu), (ADD, add), (DOWN, down)):
            assert call(shape=shape) == E_UNSUPPORTED, shape
            assert call(shape=shape, g=odd(G), ws_bytes=0) == E_UNSUPPORTED
            assert call(shape=shape, g=N) == E_INVALID
            assert cp(kind, *shape, plan) == E_UNSUPPORTED and wb(kind, *shape) == 0
    for name in ("g", "y", "mean", "rstd", "gy"):
        assert relu(**{name: odd(dict(g=G, y=Y, mean=M, rstd=R, gy=GY)[name])}, ws_bytes=0) == E_ALIGN, name
    assert add(out=odd(O), ws_bytes=0) == E_ALIGN and add(gres=odd(GRES), ws_bytes=0) == E_ALIGN
    for name, q in (("yd", YD), ("md", MD), ("rd", RD), ("gyd", GYD)):
        assert down(**{name: odd(q)}, ws_bytes=0) == E_ALIGN, name
    assert relu(ws=p(WS.value + 16), ws_bytes=0) == E_ALIGN and relu(ws=p(WS.value + 128)) == E_ALIGN


def _call(fn, kind, ptrs, shape, over):
    a = dict(ptrs, shape=shape, ws_bytes=BIG)
    a.update(over)
    return fn(kind, a["g"], a["out"], a["y"], a["mean"], a["rstd"], a["yd"], a["md"], a["rd"], a["gy"], a["gyd"], a["gres"],
              *a["shape"], a["ws"], a["ws_bytes"], None)


def test_python_wrappers_raise_not_implemented_for_refused_shapes():
    for shape in REFUSED:
        for kind in nc.KINDS:
            with pytest.raises(NotImplementedError):
                ops.norm_backward_plan(kind, *shape)
            assert not ops.norm_backward_supported(kind, *shape)
    with pytest.raises(KeyError):
        ops.norm_backward_plan("pool", 2, 35, 64)
