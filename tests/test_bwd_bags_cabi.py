"""The minibatch entry points of the C-ABI (dsmil_agg_backward_bags, its workspace query, dsmil_agg_loss_head_bags;
csrc/agg_bwd_bags.h) are declared, exported and bound without a change of the ABI version, and their size / error paths
answer without a device.  CPU only."""
import ctypes
import os
import re

import dsmil  # noqa: F401  (registers the dsmil_wsi_amd package)
import dsmil_wsi_amd._native as nat

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAGS_SYMBOLS = ("dsmil_agg_backward_bags", "dsmil_agg_backward_bags_workspace_bytes", "dsmil_agg_loss_head_bags")


def test_bags_symbols_are_declared_exported_and_bound():
    raw = open(os.path.join(ROOT, "include", "dsmil_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    lib = ctypes.CDLL(nat.LIB_PATH)
    for name in BAGS_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, src), f"{name} is not declared in include/dsmil_hip.h"
        assert hasattr(lib, name), f"{name} is not exported"
        assert name in nat.SIGNATURES, f"{name} is not in the binding table"
    # additive: the version callers pin does not move, the new entries are found by symbol
    assert int(re.search(r"#define DSMIL_ABI_VERSION (\d+)", raw).group(1)) == 6
    assert nat.lib().dsmil_abi_version() == 6
    # the batched call = the _rows call with (offsets, n_bags, total_rows, max_rows) in place of N
    rows, bags = nat.SIGNATURES["dsmil_agg_backward_rows"], nat.SIGNATURES["dsmil_agg_backward_bags"]
    assert bags[0] is rows[0] and bags[1][:2] == rows[1][:2] and bags[1][6:] == rows[1][3:]
    assert bags[1][2:6] == [nat.c_i64p, ctypes.c_int32, ctypes.c_int64, ctypes.c_int64]
    # every new entry cites the reference lines it replaces
    doc = raw[raw.index("aggregator backward over a BATCH"):raw.index("size_t dsmil_agg_backward_bags_workspace_bytes")]
    assert "train_tcga.py:60-73" in doc and "train_tcga.py:67-71" in doc


def _fake_params(ptr, K=64, Kv=64, C=2, nonlinear=1):
    """A dsmil_agg_params whose pointers are all `ptr` (aligned host memory that is never dereferenced: every check below
    fails before a launch)."""
    return nat.AggParams(ptr, ptr, ptr, ptr, ptr, ptr, ptr, ptr, K, Kv, C, nonlinear)


def test_bags_sizes_and_error_paths_without_a_device():
    L = nat.lib()
    size = L.dsmil_agg_backward_bags_workspace_bytes
    for bad in ((0, 1000, 512, 512, 2), (-1, 1000, 512, 512, 2), (4, 0, 512, 512, 2), (4, -7, 512, 512, 2),
                (4, 1000, 0, 512, 2), (4, 1000, 512, 0, 2), (4, 1000, 512, 512, 0)):
        assert size(*bad) == 0, bad
    # a batch needs what one bag of as many rows needs, plus the per-bag heads, idle tile slots and the row -> bag table
    one = L.dsmil_agg_backward_rows_workspace_bytes(640000, 512, 512, 2)
    need = size(64, 640000, 512, 512, 2)
    assert need >= one + 640000 * 4 and need < one * 1.05
    assert size(1, 10000, 512, 512, 2) >= L.dsmil_agg_backward_rows_workspace_bytes(10000, 512, 512, 2)
    assert size(64, 640000, 512, 512, 2) > size(8, 640000, 512, 512, 2) > size(8, 80000, 512, 512, 2)
    buf = (ctypes.c_char * 4096)()
    a256 = (ctypes.addressof(buf) + 255) // 256 * 256
    p = ctypes.c_void_p
    P = _fake_params(a256)
    G = nat.AggGrads(*([a256] * 8))
    pp, gp, a = ctypes.byref(P), ctypes.byref(G), p(a256)

    def bags(feats=a, offsets=a, n_bags=3, total=40, max_rows=20, params=pp, A=a, B=a, idx=a, g_max=None, g_pred=a,
             grads=gp, ws=a, ws_bytes=1 << 40, g_feats=a):
        return L.dsmil_agg_backward_bags(feats, None, offsets, n_bags, total, max_rows, params, A, B, idx, None, g_max, g_pred,
                                         None, None, grads, None, None, ws, ws_bytes, None, g_feats)
    # null pointers and non-positive / inconsistent sizes are rejected before any launch
    for kw in ({"feats": None}, {"offsets": None}, {"params": None}, {"A": None}, {"B": None}, {"idx": None},
               {"g_pred": None}, {"grads": None}, {"ws": None}, {"n_bags": 0}, {"n_bags": -2}, {"total": 0},
               {"total": 2}, {"max_rows": 0}, {"max_rows": 41}):
        assert bags(**kw) == -1, kw
    Pn = _fake_params(a256)
    Pn.fc_w = None
    assert bags(params=ctypes.byref(Pn), g_max=a) == -1     # the instance stream's share of the rows' gradient reads fc_w
    # INVALID comes first, then the row limit, then ALIGN, then WORKSPACE
    assert bags(ws=p(a256 + 16), n_bags=0) == -1
    assert bags(total=(1 << 30) + 1, max_rows=5, ws=p(a256 + 16)) == -2
    assert bags(total=1 << 30, max_rows=5, ws_bytes=16) == -3          # the largest accepted batch passes that check
    assert bags(ws=p(a256 + 16), ws_bytes=16) == -5
    Pm = _fake_params(a256)
    Pm.q0_b = a256 + 4
    assert bags(params=ctypes.byref(Pm), ws_bytes=16) == -5
    assert bags(ws_bytes=16) == -3
    assert bags(ws_bytes=size(3, 40, 64, 64, 2) - 1) == -3
    assert bags(g_feats=None, ws_bytes=16) == -3

    def head(classes=a, offsets=a, pred=a, idx=a, labels=a, n=3, C=2, loss=a):
        return L.dsmil_agg_loss_head_bags(classes, offsets, pred, idx, labels, n, C, loss, None, None, None, None)
    for kw in ({"classes": None}, {"offsets": None}, {"pred": None}, {"idx": None}, {"labels": None}, {"loss": None},
               {"n": 0}, {"C": 0}):
        assert head(**kw) == -1, kw
    assert head(C=65) == -2          # one wave of classes, like dsmil_agg_loss_head
