"""The bf16 value-stream entry points of the C-ABI (dsmil_value_*_bf16: BClassifier(passing_v=True) on bf16-stored rows,
dsmil.py:35-39,48) are declared, exported and bound — additive, ABI still 6 — and their size / error paths answer without a
device.  CPU only."""
import ctypes
import os
import re

import dsmil  # noqa: F401  (registers the dsmil_wsi_amd package)
import dsmil_wsi_amd._native as nat

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("dsmil_value_packed_bf16_bytes", "dsmil_value_pack_bf16", "dsmil_value_workspace_bf16_bytes",
           "dsmil_value_forward_bf16")
E_INVALID, E_UNSUPPORTED, E_WORKSPACE, E_ALIGN = -1, -2, -3, -5


def test_bf16_value_symbols_are_declared_exported_and_bound():
    text = open(os.path.join(ROOT, "include", "dsmil_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    lib = ctypes.CDLL(nat.LIB_PATH)
    for name in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, src), f"{name} is not declared in include/dsmil_hip.h"
        assert hasattr(lib, name), f"{name} is not exported"
        assert name in nat.SIGNATURES, f"{name} is not in the binding table"
    assert int(re.search(r"#define DSMIL_ABI_VERSION (\d+)", text).group(1)) == 6
    assert nat.lib().dsmil_abi_version() == 6
    assert nat.DSMIL_E_UNSUPPORTED == E_UNSUPPORTED and nat.DSMIL_E_WORKSPACE == E_WORKSPACE
    assert int(re.search(r"DSMIL_E_ALIGN\s*=\s*(-\d+)", text).group(1)) == E_ALIGN
    # the comment above the declarations cites the reference lines the entries replace
    block = text[:text.index("size_t dsmil_value_packed_bf16_bytes")]
    assert "dsmil.py:35-39,48" in block[block.rindex("/*"):]


def test_bf16_value_sizes_and_error_paths_without_a_device():
    L = nat.lib()
    # one bf16 per weight (K, Kv already multiples of the pad): 512 KiB at K = Kv = 512
    assert 512 * 512 * 2 <= L.dsmil_value_packed_bf16_bytes(512, 512) <= 512 * 512 * 2 + 4096
    assert L.dsmil_value_packed_bf16_bytes(72, 68) >= 72 * 68 * 2          # padded widths
    assert L.dsmil_value_packed_bf16_bytes(0, 512) == 0 and L.dsmil_value_packed_bf16_bytes(512, 0) == 0
    assert L.dsmil_value_workspace_bf16_bytes(0, 512, 512) == 0
    assert L.dsmil_value_workspace_bf16_bytes(10000, 512, 512) >= L.dsmil_value_packed_bf16_bytes(512, 512)
    # null pointers are rejected before any launch
    assert L.dsmil_value_forward_bf16(None, 10, 512, 512, None, None, None, None, None, 0, None) == E_INVALID
    assert L.dsmil_value_pack_bf16(None, 512, 512, None, None) == E_INVALID
    buf = (ctypes.c_char * 4096)()
    a256 = (ctypes.addressof(buf) + 255) // 256 * 256
    p = ctypes.c_void_p
    assert L.dsmil_value_forward_bf16(p(a256), 10, 64, 64, p(a256), p(a256), None, None, p(a256), 1 << 30, None) == E_INVALID
    assert L.dsmil_value_forward_bf16(p(a256), 10, 64, 64, p(a256), p(a256), None, p(a256), None, 0, None) == E_INVALID
    assert L.dsmil_value_forward_bf16(p(a256), 0, 64, 64, p(a256), p(a256), p(a256), p(a256), None, 0, None) == E_INVALID
    # misaligned image / workspace, short workspace (checked before any launch; the pointers are never dereferenced)
    assert L.dsmil_value_pack_bf16(p(a256), 64, 64, p(a256 + 4), None) == E_ALIGN
    assert L.dsmil_value_forward_bf16(p(a256), 10, 64, 64, p(a256), p(a256), p(a256 + 4), p(a256), None, 0, None) == E_ALIGN
    assert L.dsmil_value_forward_bf16(p(a256), 10, 64, 64, p(a256), p(a256), None, p(a256), p(a256 + 16), 1 << 30, None) == E_ALIGN
    assert L.dsmil_value_forward_bf16(p(a256), 10, 64, 64, p(a256), p(a256), None, p(a256), p(a256), 16, None) == E_WORKSPACE
    # widths the bf16 path does not take (dsmil_agg_forward_bf16's own condition): K % 8, Kv % 4
    assert L.dsmil_value_forward_bf16(p(a256), 10, 166, 166, p(a256), p(a256), p(a256), p(a256), None, 0, None) == E_UNSUPPORTED
    assert L.dsmil_value_forward_bf16(p(a256), 10, 64, 66, p(a256), p(a256), p(a256), p(a256), None, 0, None) == E_UNSUPPORTED
