"""The value-stream entry points of the C-ABI (ABI 6: dsmil_value_*; BClassifier(passing_v=True), dsmil.py:35-39,48) are
declared, exported and bound, and their size / error paths answer without a device.  CPU only."""
import ctypes
import os
import re

import dsmil  # noqa: F401  (registers the dsmil_wsi_amd package)
import dsmil_wsi_amd._native as nat

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VALUE_SYMBOLS = ("dsmil_value_packed_bytes", "dsmil_value_pack", "dsmil_value_forward", "dsmil_value_backward",
                 "dsmil_value_workspace_bytes")


def test_value_symbols_are_declared_exported_and_bound():
    src = open(os.path.join(ROOT, "include", "dsmil_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    lib = ctypes.CDLL(nat.LIB_PATH)
    for name in VALUE_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, src), f"{name} is not declared in include/dsmil_hip.h"
        assert hasattr(lib, name), f"{name} is not exported"
        assert name in nat.SIGNATURES, f"{name} is not in the binding table"
    assert int(re.search(r"#define DSMIL_ABI_VERSION (\d+)", open(os.path.join(ROOT, "include", "dsmil_hip.h")).read()).group(1)) == 6
    assert nat.lib().dsmil_abi_version() == 6


def test_value_sizes_and_error_paths_without_a_device():
    L = nat.lib()
    assert L.dsmil_value_packed_bytes(512, 512) > 0
    # two fp16 planes of every weight (K, Kv already multiples of the pad) and a small trailer: 1 MiB at K = Kv = 512
    assert 512 * 512 * 4 <= L.dsmil_value_packed_bytes(512, 512) <= 512 * 512 * 4 + 4096
    assert L.dsmil_value_packed_bytes(166, 166) >= 166 * 166 * 4          # padded widths
    assert L.dsmil_value_packed_bytes(0, 512) == 0
    assert L.dsmil_value_workspace_bytes(0, 512, 512) == 0
    assert L.dsmil_value_workspace_bytes(10000, 512, 512) >= L.dsmil_value_packed_bytes(512, 512) + 512 * 512 * 4
    # null pointers are rejected before any launch
    assert L.dsmil_value_forward(None, 10, 512, 512, None, None, None, None, None, None, 0, None) == -1
    assert L.dsmil_value_backward(None, None, None, 10, 512, 512, None, None, None, None, 0, None) == -1
    assert L.dsmil_value_pack(None, 512, 512, None, None) == -1
    # misaligned image / workspace, short workspace (checked before any launch; the pointers are never dereferenced)
    buf = (ctypes.c_char * 4096)()
    base = ctypes.addressof(buf)
    a256 = (base + 255) // 256 * 256
    p = ctypes.c_void_p
    assert L.dsmil_value_pack(p(a256), 64, 64, p(a256 + 4), None) == -5
    assert L.dsmil_value_forward(p(a256), 10, 64, 64, p(a256), p(a256), p(a256 + 4), None, p(a256), None, 0, None) == -5
    assert L.dsmil_value_forward(p(a256), 10, 64, 64, p(a256), p(a256), None, None, p(a256), p(a256 + 16), 1 << 30, None) == -5
    assert L.dsmil_value_forward(p(a256), 10, 64, 64, p(a256), p(a256), None, None, p(a256), p(a256), 16, None) == -3
    assert L.dsmil_value_backward(p(a256), p(a256), p(a256), 10, 64, 64, None, p(a256), p(a256), p(a256 + 16), 1 << 30, None) == -5
    assert L.dsmil_value_backward(p(a256), p(a256), p(a256), 10, 64, 64, None, p(a256), p(a256), p(a256), 16, None) == -3
