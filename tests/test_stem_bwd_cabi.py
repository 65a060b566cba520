"""The training stem's entries (dsmil_trunk32_stem_train*, dsmil_stem_pool_bwd*: csrc/resnet_fwd.hip, csrc/stem_bwd.hip) are
declared, exported and bound — additive, ABI still 6 —; their size queries, plan and refusals answer without a device (every
check runs before the first launch, in the documented order); the plan of every case of tests/stem_bwd_cases.py is PINNED, so
the chunk, run_len, lanes and n_partials the bars are formed from are declarations, not results; and use_native_stem keeps the
model's state dict, children and Parameters.  CPU only: no call here reaches a launch, the pointers are never read."""
import ctypes
import os
import re

import pytest
import torch
import torch.nn as nn

import stem_bwd_cases as sc
import dsmil  # noqa: F401  (registers the dsmil_wsi_amd package)
import dsmil_wsi_amd._native as nat
from dsmil_wsi_amd import modules, ops, simclr
from dsmil_wsi_amd.resnet import resnet18, resnet18_in_convs, resnet50

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("dsmil_trunk32_stem_train_workspace_bytes", "dsmil_trunk32_stem_train", "dsmil_stem_pool_bwd_plan",
           "dsmil_stem_pool_bwd_workspace_bytes", "dsmil_stem_pool_bwd")
E_INVALID, E_UNSUPPORTED, E_WORKSPACE, E_ALIGN = -1, -2, -3, -5
BIG = 1 << 40
FIELDS = ("Hp", "Wp", "chunk", "n_partials", "run_len", "lanes", "grid_partial", "grid_finish", "grid_apply", "groups")


def test_stem_symbols_are_declared_exported_and_bound():
    text = open(os.path.join(ROOT, "include", "dsmil_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    lib = ctypes.CDLL(nat.LIB_PATH)
    for name in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, src), f"{name} is not declared in include/dsmil_hip.h"
        assert hasattr(lib, name), f"{name} is not exported"
        assert name in nat.SIGNATURES, f"{name} is not in the binding table"
    assert int(re.search(r"#define DSMIL_ABI_VERSION (\d+)", text).group(1)) == 6
    assert nat.lib().dsmil_abi_version() == 6


def test_the_plan_of_every_case_is_pinned():
    for name, B, H1, W1, C, _ in sc.CASES:
        p = ops.stem_pool_backward_plan(B, H1, W1, C)
        assert tuple(p[f] for f in FIELDS) == sc.PLANS[name], (name, p)
        assert p["block"] == 256
        assert tuple(p[f] for f in FIELDS[:6]) == sc.plan_of(B, H1, W1, C)
        assert p["grid_partial"] == B * p["n_partials"] and p["grid_apply"] == min(-(-B * H1 * W1 // p["lanes"]), 8192)
    for name, B, H1, W1, C in sc.EXACT_CASES:
        assert ops.stem_pool_backward_plan(B, H1, W1, C)["chunk"] == 256        # what the emulation of the exact cases assumes
    # the conditions the case names claim
    P = sc.PLANS
    assert P["p_16x16"][3] == 1 and P["p_16x16"][4] * P["p_16x16"][5] == 256 and P["p_16x17"][3] == 2 and P["p_27x26"][3] == 3
    assert P["p_5x7"][:2] == (3, 4)
    # the stem of ResNet-18 at 224 x 224: the chunk doubles while B x chunks exceeds 2048 workgroups (dsmil_norm_bwd's rule)
    for B, chunk, parts in [(256, 2048, 7), (64, 512, 25)]:
        p = ops.stem_pool_backward_plan(B, 112, 112, 64)
        assert (p["Hp"], p["Wp"], p["chunk"], p["n_partials"]) == (56, 56, chunk, parts), p
        assert {k: v for k, v in p.items() if k not in ("Hp", "Wp")} == \
            {k: v for k, v in ops.norm_backward_plan("relu", B, 112 * 112, 64).items() if k not in ("kind", "n_sums")}


def test_sizes_without_a_device():
    L = nat.lib()
    wb = L.dsmil_stem_pool_bwd_workspace_bytes
    for name, B, H1, W1, C, _ in sc.CASES:
        parts = sc.PLANS[name][3]
        assert wb(B, H1, W1, C) >= 2 * B * C * 4 * (parts + 1) and wb(B, H1, W1, C) % 256 == 0
        assert ops.stem_pool_backward_supported(B, H1, W1, C)
    assert wb(0, 5, 7, 64) == 0 and wb(2, 0, 7, 64) == 0 and wb(2, 5, -1, 64) == 0 and wb(2, 5, 7, 0) == 0
    tb, sb = L.dsmil_trunk32_stem_train_workspace_bytes, L.dsmil_trunk32_stem_workspace_bytes
    for B, H, W in ((1, 32, 32), (3, 34, 38), (1, 65, 33), (256, 224, 224)):
        H1, W1 = (H - 1) // 2 + 1, (W - 1) // 2 + 1
        # the sibling's workspace without the raw map, which is an output here
        assert 0 < tb(B, H, W) <= sb(B, H, W) - B * H1 * W1 * 64 * 4 and tb(B, H, W) % 256 == 0
        assert ops.trunk32_stem_train_supported(B, H, W)
    for shape in ((0, 32, 32), (1, 31, 32), (1, 32, 31), (65536, 32, 32), (8192, 256, 256)):
        assert tb(*shape) == 0 and not ops.trunk32_stem_train_supported(*shape)
    assert sb(8192, 256, 256) > 0                                            # the raw map's 2^31 is the training entry's own limit


REFUSED = [(2, 5, 7, 6), (2, 5, 7, 66), (2, 5, 7, 96), (2, 5, 7, 40), (2, 5, 7, 1536), (2, 5, 7, 4096), (2, 5, 7, 2052),   # C
           (4, 1 << 10, 1 << 10, 512), (1 << 20, 1, 1, 2048), (1, 1 << 16, 1 << 16, 64)]                       # B H1 W1 C >= 2^31


def _bwd(fn, ptrs, shape, over):
    a = dict(ptrs, shape=shape, ws_bytes=BIG)
    a.update(over)
    return fn(a["g"], a["y"], a["mean"], a["rstd"], a["win"], a["gy"], *a["shape"], a["ws"], a["ws_bytes"], None)


def test_stem_pool_bwd_refusals_without_a_device():
    L = nat.lib()
    p = ctypes.c_void_p
    # addresses far enough apart that no two maps of the shapes below overlap; nothing here is ever dereferenced
    G, Y, M, R, WIN, GY, WS = (p((i + 1) << 44) for i in range(7))
    N = None
    plan = (ctypes.c_int32 * 16)()
    cp, wb, fn = L.dsmil_stem_pool_bwd_plan, L.dsmil_stem_pool_bwd_workspace_bytes, L.dsmil_stem_pool_bwd
    ok = (2, 5, 7, 64)
    assert cp(*ok, None) == E_INVALID and cp(0, 5, 7, 64, plan) == E_INVALID and cp(2, -1, 7, 64, plan) == E_INVALID
    assert cp(2, 5, 0, 64, plan) == E_INVALID and cp(2, 5, 7, 0, plan) == E_INVALID and cp(*ok, plan) == 0
    call = lambda **k: _bwd(fn, dict(g=G, y=Y, mean=M, rstd=R, win=WIN, gy=GY, ws=WS), ok, k)
    # a short workspace is the LAST check: the complete call gets that far
    assert call(ws_bytes=0) == E_WORKSPACE and call(ws_bytes=wb(*ok) - 1) == E_WORKSPACE
    for need in ("g", "y", "mean", "rstd", "win", "gy", "ws"):
        assert call(**{need: N}) == E_INVALID, need
    for bad in ((0, 5, 7, 64), (2, 0, 7, 64), (2, 5, -3, 64), (2, 5, 7, -4)):
        assert call(shape=bad) == E_INVALID
    # gy sharing a byte with an input: the same pointer, or an overlapping range
    nbytes, pooled = 2 * 5 * 7 * 64 * 4, 2 * 3 * 4 * 64
    assert call(gy=Y) == E_INVALID and call(gy=G) == E_INVALID and call(gy=M) == E_INVALID and call(gy=WIN) == E_INVALID
    assert call(gy=p(Y.value + nbytes - 16)) == E_INVALID and call(gy=p(Y.value - nbytes + 16)) == E_INVALID
    assert call(gy=p(Y.value + nbytes), ws_bytes=0) == E_WORKSPACE              # adjacent is not aliasing
    assert call(gy=p(G.value + pooled * 4 - 16)) == E_INVALID and call(gy=p(G.value + pooled * 4), ws_bytes=0) == E_WORKSPACE
    assert call(gy=p(WIN.value + pooled - 16)) == E_INVALID and call(gy=p(WIN.value + pooled), ws_bytes=0) == E_WORKSPACE
    assert call(gy=p(R.value + 2 * 64 * 4 - 16)) == E_INVALID
    # INVALID comes before UNSUPPORTED, UNSUPPORTED before ALIGN, ALIGN before WORKSPACE
    odd = lambda q, by=4: p(q.value + by)
    for shape in REFUSED:
        assert call(shape=shape) == E_UNSUPPORTED, shape
        assert call(shape=shape, g=odd(G), ws_bytes=0) == E_UNSUPPORTED
        assert call(shape=shape, g=N) == E_INVALID
        assert cp(*shape, plan) == E_UNSUPPORTED and wb(*shape) == 0
    for name, q in (("g", G), ("y", Y), ("mean", M), ("rstd", R), ("gy", GY)):
        assert call(**{name: odd(q)}, ws_bytes=0) == E_ALIGN, name
    assert call(win=odd(WIN, 2), ws_bytes=0) == E_ALIGN and call(win=odd(WIN), ws_bytes=0) == E_WORKSPACE
    assert call(ws=p(WS.value + 16), ws_bytes=0) == E_ALIGN and call(ws=p(WS.value + 128)) == E_ALIGN


def test_trunk32_stem_train_refusals_without_a_device():
    L = nat.lib()
    p = ctypes.c_void_p
    X, Wt, Y, M, R, P, WIN, WS = (p((i + 1) << 44) for i in range(8))
    fn, wb = L.dsmil_trunk32_stem_train, L.dsmil_trunk32_stem_train_workspace_bytes

    def call(shape=(2, 34, 38), u8=0, prec=0, ws_bytes=BIG, **over):
        a = dict(x=X, w=Wt, y=Y, mean=M, rstd=R, pooled=P, win=WIN, ws=WS)
        a.update(over)
        return fn(a["x"], u8, a["w"], a["y"], a["mean"], a["rstd"], a["pooled"], a["win"], *shape, prec, a["ws"], ws_bytes, None)

    assert call(ws_bytes=0) == E_WORKSPACE and call(ws_bytes=wb(2, 34, 38) - 1) == E_WORKSPACE and call(u8=1, ws_bytes=0) == E_WORKSPACE
    for need in ("x", "w", "y", "mean", "rstd", "pooled", "win", "ws"):
        assert call(**{need: None}) == E_INVALID, need
    assert call(shape=(0, 34, 38)) == E_INVALID and call(shape=(2, 0, 38)) == E_INVALID and call(shape=(2, 34, -1)) == E_INVALID
    odd = lambda q, by=4: p(q.value + by)
    for kw in (dict(prec=2), dict(shape=(2, 31, 38)), dict(shape=(2, 34, 16)), dict(shape=(65536, 32, 32)), dict(shape=(8192, 256, 256))):
        assert call(**kw) == E_UNSUPPORTED, kw
        assert call(y=odd(Y), ws_bytes=0, **kw) == E_UNSUPPORTED                # before ALIGN and WORKSPACE
        assert call(y=None, **kw) == E_INVALID                                  # after INVALID
    for name, q in (("y", Y), ("mean", M), ("rstd", R), ("pooled", P)):
        assert call(**{name: odd(q)}, ws_bytes=0) == E_ALIGN, name
    assert call(x=odd(X, 2), ws_bytes=0) == E_ALIGN and call(x=odd(X, 1), u8=1, ws_bytes=0) == E_WORKSPACE
    assert call(w=odd(Wt, 2), ws_bytes=0) == E_ALIGN and call(win=odd(WIN, 2), ws_bytes=0) == E_ALIGN
    assert call(ws=p(WS.value + 128), ws_bytes=0) == E_ALIGN


def test_python_wrappers_raise_not_implemented_for_refused_shapes():
    for shape in REFUSED:
        with pytest.raises(NotImplementedError):
            ops.stem_pool_backward_plan(*shape)
        assert not ops.stem_pool_backward_supported(*shape)


# ---- the module layer on the CPU --------------------------------------------------------------------------------------------
def _resnet(f=resnet18, norm=nn.InstanceNorm2d):
    m = f(norm_layer=norm)
    m.fc = nn.Identity()
    return m


def test_use_native_stem_keeps_the_state_dict_the_children_and_the_parameters():
    m = _resnet()
    before = {k: v.clone() for k, v in m.state_dict().items()}
    params = {n: p for n, p in m.named_parameters()}
    names = [n for n, _ in m.named_modules()]
    convs = resnet18_in_convs(m)
    assert simclr.use_native_stem(m) == 1
    after = m.state_dict()
    assert list(after) == list(before) and all(torch.equal(after[k], before[k]) for k in before)
    assert all(p is params[n] for n, p in m.named_parameters()) and len(list(m.named_parameters())) == len(params)
    assert [n for n, _ in m.named_modules()] == names
    got = resnet18_in_convs(m)
    assert got is not None and all(a is b for a, b in zip(got, convs)) and modules.resnet_convs_of(m)[1] is None
    # it composes with the other swaps in any order
    assert simclr.use_native_blocks(m) == 8 and simclr.use_native_convs(m) == 20
    m2 = _resnet()
    assert simclr.use_native_convs(m2) == 20 and simclr.use_native_blocks(m2) == 8 and simclr.use_native_stem(m2) == 1
    assert list(m2.state_dict()) == list(before) and [n for n, _ in m2.named_modules()] == names
    # the stems it leaves to torch, and what is not a ResNet
    assert simclr.use_native_stem(_resnet(resnet18, nn.BatchNorm2d)) == 0
    assert simclr.use_native_stem(_resnet(resnet50)) == 1                       # a Bottleneck trunk has the same stem
    odd = _resnet()
    odd.maxpool = nn.MaxPool2d(3, 2, 1, ceil_mode=True)
    assert simclr.use_native_stem(odd) == 0
    with pytest.raises(TypeError):
        simclr.use_native_stem(nn.Sequential())


def test_a_marked_resnet_on_the_cpu_is_the_torch_chain():
    m, ref = _resnet(), _resnet()
    ref.load_state_dict(m.state_dict())
    simclr.use_native_stem(m)
    x = torch.rand(1, 3, 64, 64)
    outs = []
    for model in (ref, m):
        out = model.train()(x)
        out.square().sum().backward()
        outs.append((out.detach(), model.conv1.weight.grad))
    assert all(torch.equal(a, b) for a, b in zip(*outs))
    with pytest.raises(NotImplementedError):
        simclr.native_stem(x, m.conv1.weight)                                  # the functional form has no fallback
