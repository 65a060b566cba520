"""The bf16-row backward of the C-ABI (dsmil_agg_backward_bags_bf16 and its workspace query; csrc/agg_bwd_bags.h) is
declared, exported and bound without a change of the ABI version, and its size / error paths answer without a device, in
the documented order.  CPU only."""
import ctypes
import os
import re

import dsmil  # noqa: F401  (registers the dsmil_wsi_amd package)
import dsmil_wsi_amd._native as nat

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("dsmil_agg_backward_bags_bf16", "dsmil_agg_backward_bags_bf16_workspace_bytes")


def test_b16_symbols_are_declared_exported_and_bound():
    raw = open(os.path.join(ROOT, "include", "dsmil_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    lib = ctypes.CDLL(nat.LIB_PATH)
    for name in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, src), f"{name} is not declared in include/dsmil_hip.h"
        assert hasattr(lib, name), f"{name} is not exported"
        assert name in nat.SIGNATURES, f"{name} is not in the binding table"
    assert int(re.search(r"#define DSMIL_ABI_VERSION (\d+)", raw).group(1)) == 6
    assert nat.lib().dsmil_abi_version() == 6
    # the fp32 batched call without its row_map and g_feats arguments, the two row pointers untyped
    f32, b16 = nat.SIGNATURES["dsmil_agg_backward_bags"], nat.SIGNATURES["dsmil_agg_backward_bags_bf16"]
    assert b16[0] is f32[0]
    assert b16[1][:2] == [ctypes.c_void_p, ctypes.c_void_p]
    assert b16[1][2:] == f32[1][2:17] + f32[1][18:21]
    assert nat.SIGNATURES[SYMBOLS[1]] == nat.SIGNATURES["dsmil_agg_backward_bags_workspace_bytes"]
    # the entry cites the reference lines it replaces
    doc = raw[raw.index("batched aggregator backward on bf16-STORED rows"):raw.index("size_t dsmil_agg_backward_bags_bf16_workspace_bytes")]
    assert "train_tcga.py:60-73" in doc


def _fake_params(ptr, K=64, Kv=64, C=2, nonlinear=1):
    """A dsmil_agg_params whose pointers are all `ptr` (aligned host memory that is never dereferenced: every check below
    fails before a launch)."""
    return nat.AggParams(ptr, ptr, ptr, ptr, ptr, ptr, ptr, ptr, K, Kv, C, nonlinear)


def test_b16_sizes_and_error_paths_without_a_device():
    L = nat.lib()
    size = L.dsmil_agg_backward_bags_bf16_workspace_bytes
    for bad in ((0, 1000, 512, 512, 2), (-1, 1000, 512, 512, 2), (4, 0, 512, 512, 2), (4, -7, 512, 512, 2),
                (4, 1000, 0, 512, 2), (4, 1000, 512, 0, 2), (4, 1000, 512, 512, 0)):
        assert size(*bad) == 0, bad
    # the workspace layout is the fp32 call's
    for shape in ((1, 10000, 512, 512, 2), (7, 1118, 512, 512, 2), (64, 640000, 512, 512, 2), (3, 40, 64, 64, 5)):
        assert size(*shape) == L.dsmil_agg_backward_bags_workspace_bytes(*shape) > 0, shape
    buf = (ctypes.c_char * 4096)()
    a256 = (ctypes.addressof(buf) + 255) // 256 * 256
    p = ctypes.c_void_p
    P = _fake_params(a256)
    G = nat.AggGrads(*([a256] * 8))
    pp, gp, a = ctypes.byref(P), ctypes.byref(G), p(a256)

    def bags(feats=a, vals=None, offsets=a, n_bags=3, total=40, max_rows=20, params=pp, A=a, B=a, idx=a, g_max=None, g_pred=a,
             grads=gp, ws=a, ws_bytes=1 << 40):
        return L.dsmil_agg_backward_bags_bf16(feats, vals, offsets, n_bags, total, max_rows, params, A, B, idx, None, g_max,
                                              g_pred, None, None, grads, None, ws, ws_bytes, None)
    # null pointers and non-positive / inconsistent sizes are rejected before any launch
    for kw in ({"feats": None}, {"offsets": None}, {"params": None}, {"A": None}, {"B": None}, {"idx": None},
               {"g_pred": None}, {"grads": None}, {"ws": None}, {"n_bags": 0}, {"n_bags": -2}, {"total": 0},
               {"total": 2}, {"max_rows": 0}, {"max_rows": 41}):
        assert bags(**kw) == -1, kw
    Gn = nat.AggGrads(*([a256] * 8))
    Gn.fc_w = None
    assert bags(grads=ctypes.byref(Gn), g_max=a) == -1         # the sparse max-stream gradient needs somewhere to go
    # INVALID first, then UNSUPPORTED (the row limit, the forward's shape condition), then ALIGN, then WORKSPACE
    assert bags(ws=p(a256 + 16), n_bags=0) == -1
    assert bags(total=(1 << 30) + 1, max_rows=5, ws=p(a256 + 16)) == -2
    assert bags(total=1 << 30, max_rows=5, ws_bytes=16) == -3          # the largest accepted batch passes that check
    for K, Kv in ((166, 166), (68, 68), (64, 62)):
        Pk = _fake_params(a256, K=K, Kv=Kv)
        assert bags(params=ctypes.byref(Pk), vals=a if K != Kv else None, feats=p(a256 + 8), ws_bytes=16) == -2, (K, Kv)
    assert bags(feats=p(a256 + 8), ws_bytes=16) == -5          # rows off 16-byte alignment
    assert bags(vals=p(a256 + 8), ws_bytes=16) == -5
    assert bags(ws=p(a256 + 16), ws_bytes=16) == -5
    Pm = _fake_params(a256)
    Pm.q0_b = a256 + 4
    assert bags(params=ctypes.byref(Pm), ws_bytes=16) == -5
    assert bags(ws_bytes=16) == -3
    assert bags(ws_bytes=size(3, 40, 64, 64, 2) - 1) == -3
