"""The row-gradient entry points of the C-ABI (dsmil_agg_backward_rows, dsmil_value_backward_rows and the workspace
query; csrc/agg_gx.h) are declared, exported and bound without a change of the ABI version, and their size / error
paths answer without a device.  CPU only."""
import ctypes
import os
import re

import dsmil  # noqa: F401  (registers the dsmil_wsi_amd package)
import dsmil_wsi_amd._native as nat

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GX_SYMBOLS = ("dsmil_agg_backward_rows", "dsmil_agg_backward_rows_workspace_bytes", "dsmil_value_backward_rows")


def test_gx_symbols_are_declared_exported_and_bound():
    raw = open(os.path.join(ROOT, "include", "dsmil_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    lib = ctypes.CDLL(nat.LIB_PATH)
    for name in GX_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, src), f"{name} is not declared in include/dsmil_hip.h"
        assert hasattr(lib, name), f"{name} is not exported"
        assert name in nat.SIGNATURES, f"{name} is not in the binding table"
    # additive: the version callers pin does not move, the new entries are found by symbol
    assert int(re.search(r"#define DSMIL_ABI_VERSION (\d+)", raw).group(1)) == 6
    assert nat.lib().dsmil_abi_version() == 6
    # the _rows call is the _ex call plus one trailing pointer
    ex, rows = nat.SIGNATURES["dsmil_agg_backward_ex"], nat.SIGNATURES["dsmil_agg_backward_rows"]
    assert rows[0] is ex[0] and rows[1][:-1] == ex[1] and len(rows[1]) == len(ex[1]) + 1


def _fake_params(ptr, K=64, Kv=64, C=2, nonlinear=1):
    """A dsmil_agg_params whose pointers are all `ptr` (16-B aligned host memory that is never dereferenced: every check
    below fails before a launch)."""
    return nat.AggParams(ptr, ptr, ptr, ptr, ptr, ptr, ptr, ptr, K, Kv, C, nonlinear)


def test_gx_sizes_and_error_paths_without_a_device():
    L = nat.lib()
    assert L.dsmil_agg_backward_rows_workspace_bytes(0, 512, 512, 2) == 0
    assert L.dsmil_agg_backward_rows_workspace_bytes(1000, 0, 512, 2) == 0
    need = L.dsmil_agg_backward_rows_workspace_bytes(10000, 512, 512, 2)
    assert need >= L.dsmil_agg_backward_workspace_bytes(10000, 512, 512, 2) > 10000 * 128 * 4 * 4
    buf = (ctypes.c_char * 4096)()
    a256 = (ctypes.addressof(buf) + 255) // 256 * 256
    p = ctypes.c_void_p
    P = _fake_params(a256)
    G = nat.AggGrads(*([a256] * 8))
    pp, gp, a = ctypes.byref(P), ctypes.byref(G), p(a256)

    def rows(feats=a, N=10, params=pp, A=a, B=a, idx=a, g_max=None, g_pred=a, grads=gp, ws=a, ws_bytes=1 << 40, g_feats=a):
        return L.dsmil_agg_backward_rows(feats, None, N, params, A, B, idx, None, g_max, g_pred, None, None, grads, None,
                                         None, ws, ws_bytes, None, g_feats)
    # null pointers and non-positive sizes are rejected before any launch
    assert L.dsmil_agg_backward_rows(*([None] * 2), 10, *([None] * 13), 0, None, None) == -1
    for kw in ({"feats": None}, {"params": None}, {"A": None}, {"B": None}, {"idx": None}, {"g_pred": None},
               {"grads": None}, {"ws": None}, {"N": 0}, {"N": -5}):
        assert rows(**kw) == -1, kw
    # the instance stream's share of the rows' gradient reads fc_w
    Pn = _fake_params(a256)
    Pn.fc_w = None
    assert rows(params=ctypes.byref(Pn), g_max=a) == -1
    # misaligned workspace / misaligned query bias, then a short workspace (checked in this order, before any launch)
    assert rows(ws=p(a256 + 16)) == -5
    Pm = _fake_params(a256)
    Pm.q0_b = a256 + 4
    assert rows(params=ctypes.byref(Pm)) == -5
    assert rows(ws_bytes=16) == -3
    assert rows(ws_bytes=L.dsmil_agg_backward_rows_workspace_bytes(10, 64, 64, 2) - 1) == -3
    # g_feats == NULL is dsmil_agg_backward_ex: the same answers
    assert rows(g_feats=None, ws_bytes=16) == -3 and rows(g_feats=None, N=0) == -1

    def vrows(V=a, g_vals=a, n=10, K=64, Kv=64, v_w=a, g_feats=a, ws=None, ws_bytes=0):
        return L.dsmil_value_backward_rows(None, V, g_vals, n, K, Kv, v_w, None, 0, g_feats, ws, ws_bytes, None)
    for kw in ({"V": None}, {"g_vals": None}, {"v_w": None}, {"g_feats": None}, {"n": 0}, {"n": -1}, {"K": 0}, {"Kv": 0}):
        assert vrows(**kw) == -1, kw
    assert vrows(ws=p(a256 + 16), ws_bytes=1 << 20) == -5   # it needs no workspace; one that is handed in must be aligned
