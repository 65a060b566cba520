"""dsmil_value_backward_bf16 / dsmil_value_backward_bf16_workspace_bytes (the value layer's parameter gradients on bf16-stored
rows, dsmil.py:35-39 behind g_vals) are declared, exported and bound — additive, ABI still 6 — and their size and error paths
answer, in the documented order, without a device: every call below returns before any launch and dereferences nothing.
CPU only."""
import ctypes
import os
import re

import dsmil  # noqa: F401  (registers the dsmil_wsi_amd package)
import dsmil_wsi_amd._native as nat

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("dsmil_value_backward_bf16_workspace_bytes", "dsmil_value_backward_bf16")
OK, E_INVALID, E_UNSUPPORTED, E_WORKSPACE, E_ALIGN = 0, -1, -2, -3, -5


def test_symbols_are_declared_exported_and_bound():
    text = open(os.path.join(ROOT, "include", "dsmil_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    lib = ctypes.CDLL(nat.LIB_PATH)
    for name in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, src), f"{name} is not declared in include/dsmil_hip.h"
        assert hasattr(lib, name), f"{name} is not exported"
        assert name in nat.SIGNATURES, f"{name} is not in the binding table"
    assert int(re.search(r"#define DSMIL_ABI_VERSION (\d+)", text).group(1)) == 6
    assert nat.lib().dsmil_abi_version() == 6
    block = text[:text.index("size_t dsmil_value_backward_bf16_workspace_bytes")]
    assert "dsmil.py:35-39" in block[block.rindex("/*"):]
    assert "there is no backward for bf16 rows" not in text


def test_workspace_bytes():
    L = nat.lib()
    n = L.dsmil_value_backward_bf16_workspace_bytes
    assert n(10000, 512, 512) > 0 and n(1, 64, 64) >= 64 * 64 * 4 + 64 * 4
    assert n(0, 512, 512) == 0 and n(-1, 512, 512) == 0 and n(10, 0, 512) == 0 and n(10, 512, 0) == 0 and n(10, -8, 64) == 0
    assert n(10000, 512, 512) % 256 == 0
    # partials only: no fp32 copy of the rows or of V (10 000 x 512 of either would be 20 MB)
    assert n(10000, 512, 512) < 10000 * 512 * 4


def test_error_paths_in_order_without_a_device():
    L = nat.lib()
    f = L.dsmil_value_backward_bf16
    buf = (ctypes.c_char * 4096)()
    a = (ctypes.addressof(buf) + 255) // 256 * 256
    p = ctypes.c_void_p
    big = 1 << 40
    good = dict(feats=p(a), V=p(a), g=p(a), rows=10, K=64, Kv=64, gw=p(a), gb=p(a), ws=p(a), nb=big)

    def call(**kw):
        c = dict(good, **kw)
        return f(c["feats"], c["V"], c["g"], c["rows"], c["K"], c["Kv"], c["gw"], c["gb"], c["ws"], c["nb"], None)
    # 1. invalid: a NULL operand, a non-positive extent
    for k in ("feats", "V", "g", "gw", "gb", "ws"):
        assert call(**{k: None}) == E_INVALID, k
    for k in ("rows", "K", "Kv"):
        assert call(**{k: 0}) == E_INVALID and call(**{k: -4}) == E_INVALID, k
    # ... which wins over everything behind it
    assert call(feats=None, K=166, ws=p(a + 16), nb=0) == E_INVALID
    # 2. unsupported: K % 8, Kv % 4 (dsmil_value_forward_bf16's condition), a grid beyond 2^31 - 1 workgroups
    assert call(K=166, Kv=166) == E_UNSUPPORTED
    assert call(K=68) == E_UNSUPPORTED and call(Kv=66) == E_UNSUPPORTED
    assert call(K=1 << 23, Kv=1 << 23) == E_UNSUPPORTED               # 2^17 x 2^16 slabs
    # ... which wins over alignment and workspace
    assert call(K=166, Kv=166, feats=p(a + 2), ws=p(a + 16), nb=0) == E_UNSUPPORTED
    # 3. alignment: rows 16 B, V 8 B, g_vals 16 B, workspace 256 B
    assert call(feats=p(a + 8)) == E_ALIGN
    assert call(V=p(a + 4)) == E_ALIGN and call(V=p(a + 8), nb=0) == E_WORKSPACE
    assert call(g=p(a + 8)) == E_ALIGN
    assert call(ws=p(a + 128)) == E_ALIGN
    # ... which wins over a short workspace
    assert call(feats=p(a + 8), nb=0) == E_ALIGN
    # 4. workspace
    need = L.dsmil_value_backward_bf16_workspace_bytes(10, 64, 64)
    assert call(nb=0) == E_WORKSPACE and call(nb=need - 1) == E_WORKSPACE
