"""The test entries of the 16-bit activation trunk (dsmil_trunk16_*: the stages of csrc/resnet_b16.h alone) are declared,
exported and bound — additive, ABI still 6 — and their size queries and refusals answer without a device: every check runs
before the first launch, so a bad call never reaches one.  CPU only."""
import ctypes
import os
import re

import dsmil  # noqa: F401  (registers the dsmil_wsi_amd package)
import dsmil_wsi_amd._native as nat

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("dsmil_trunk16_positions", "dsmil_trunk16_layout", "dsmil_trunk16_conv_workspace_bytes", "dsmil_trunk16_conv",
           "dsmil_trunk16_norm_workspace_bytes", "dsmil_trunk16_norm", "dsmil_trunk16_pool", "dsmil_trunk16_workspace_bytes",
           "dsmil_trunk16_forward")
E_INVALID, E_UNSUPPORTED, E_WORKSPACE, E_ALIGN = -1, -2, -3, -5
BIG = 1 << 30


def test_trunk16_symbols_are_declared_exported_and_bound():
    text = open(os.path.join(ROOT, "include", "dsmil_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    lib = ctypes.CDLL(nat.LIB_PATH)
    for name in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, src), f"{name} is not declared in include/dsmil_hip.h"
        assert hasattr(lib, name), f"{name} is not exported"
        assert name in nat.SIGNATURES, f"{name} is not in the binding table"
    assert int(re.search(r"#define DSMIL_ABI_VERSION (\d+)", text).group(1)) == 6
    assert nat.lib().dsmil_abi_version() == 6
    # the comment above the declarations says what the entries are for
    block = text[:text.index("size_t dsmil_trunk16_positions")]
    assert "FOR TESTS" in block[block.rindex("/*"):]


def test_trunk16_sizes_without_a_device():
    L = nat.lib()
    assert L.dsmil_trunk16_positions(3, 9, 7) == 3 * 10 * 8 + 8
    assert L.dsmil_trunk16_positions(0, 9, 7) == 0 and L.dsmil_trunk16_positions(1, 0, 7) == 0
    assert 512 * 512 * 9 * 2 <= L.dsmil_trunk16_conv_workspace_bytes(512, 512, 3) < 512 * 512 * 9 * 2 + 256
    assert L.dsmil_trunk16_conv_workspace_bytes(64, 128, 2) == 0 and L.dsmil_trunk16_conv_workspace_bytes(0, 128, 3) == 0
    assert L.dsmil_trunk16_norm_workspace_bytes(5, 512) >= 5 * 8 * 512 * 2 * 4 and L.dsmil_trunk16_norm_workspace_bytes(0, 512) == 0
    w18, w34 = L.dsmil_trunk16_workspace_bytes(18, 3, 9, 9), L.dsmil_trunk16_workspace_bytes(34, 3, 9, 9)
    packed18 = L.dsmil_resnet_packed_bytes_ex(18, 2) - L.dsmil_resnet_packed_bytes_ex(18, 1)     # the 16-bit weight image
    assert w34 > w18 >= packed18 + 4 * 2 * 64 * L.dsmil_trunk16_positions(3, 9, 9)
    assert L.dsmil_trunk16_workspace_bytes(50, 3, 9, 9) == 0 and L.dsmil_trunk16_workspace_bytes(18, 0, 9, 9) == 0


def test_trunk16_refusals_without_a_device():
    L = nat.lib()
    buf = (ctypes.c_char * 4096)()
    a = (ctypes.addressof(buf) + 255) // 256 * 256
    p = ctypes.c_void_p
    P, Q, R, odd = p(a), p(a + 256), p(a + 512), p(a + 4)         # three distinct aligned addresses (never dereferenced), one misaligned

    # layout
    lay = L.dsmil_trunk16_layout
    assert lay(None, None, 2, 5, 7, 64, 1, 0, None) == E_INVALID
    assert lay(None, Q, 2, 5, 7, 64, 1, 0, None) == E_INVALID           # pad mode reads x
    assert lay(P, Q, 0, 5, 7, 64, 1, 0, None) == E_INVALID and lay(P, Q, 2, 5, 7, 64, 0, 0, None) == E_INVALID
    assert lay(P, Q, 2, 5, 7, 64, 3, 0, None) == E_INVALID              # kind is 1 (bf16) or 2 (fp16)
    assert lay(P, Q, 2, 5, 7, 60, 1, 0, None) == E_UNSUPPORTED          # C % 8
    assert lay(P, Q, 60000, 1000, 1000, 64, 1, 0, None) == E_UNSUPPORTED
    assert lay(P, odd, 2, 5, 7, 64, 1, 0, None) == E_ALIGN and lay(odd, Q, 2, 5, 7, 64, 2, 0, None) == E_ALIGN

    # conv: (in, w, out, B, Hi, Wi, Cin, Cout, ks, stride, pad, kind, ws, ws_bytes, stream)
    conv = L.dsmil_trunk16_conv
    assert conv(None, Q, R, 2, 9, 7, 64, 64, 3, 1, 1, 1, P, BIG, None) == E_INVALID
    assert conv(P, None, R, 2, 9, 7, 64, 64, 3, 1, 1, 1, P, BIG, None) == E_INVALID
    assert conv(P, Q, None, 2, 9, 7, 64, 64, 3, 1, 1, 1, P, BIG, None) == E_INVALID
    assert conv(P, Q, R, 2, 9, 7, 64, 64, 3, 1, 1, 1, None, BIG, None) == E_INVALID
    assert conv(P, Q, P, 2, 9, 7, 64, 64, 3, 1, 1, 1, R, BIG, None) == E_INVALID            # in place
    assert conv(P, Q, R, 2, 0, 7, 64, 64, 3, 1, 1, 1, P, BIG, None) == E_INVALID
    assert conv(P, Q, R, 2, 9, 7, 64, 64, 3, 1, 1, 0, P, BIG, None) == E_INVALID            # kind
    for cin, cout, ks, stride, pad in [(60, 64, 3, 1, 1),          # Cin % 8
                                       (16, 64, 3, 1, 1),          # 3x3/1: Cin % 32
                                       (64, 96, 3, 1, 1),          # 3x3/1: Cout % 64
                                       (32, 128, 3, 2, 1),         # strided: Cin % 64
                                       (64, 64, 3, 2, 1),          # strided: Cout % 128
                                       (64, 128, 1, 1, 0),         # 1x1/1, 3x3 without its padding, 5x5, stride 3: no form of the trunk
                                       (64, 128, 3, 1, 0), (64, 128, 5, 1, 2), (64, 128, 3, 3, 1)]:
        assert conv(P, Q, R, 2, 9, 7, cin, cout, ks, stride, pad, 1, P, BIG, None) == E_UNSUPPORTED, (cin, cout, ks, stride, pad)
    # the window limits of k_conv_b16n, k_conv_b16w<512,64> and k_conv_b16w<256,128>: one pixel wider than each takes
    for Wi, cin, cout in [(127, 64, 64), (128, 64, 64), (255, 128, 64), (255, 32, 128), (256, 32, 128)]:
        assert conv(P, Q, R, 1, 3, Wi, cin, cout, 3, 1, 1, 2, P, BIG, None) == E_UNSUPPORTED, (Wi, cin, cout)
    assert conv(P, Q, R, 1, 1, 1, 64, 128, 3, 2, 0, 1, P, BIG, None) == E_UNSUPPORTED       # no output pixel
    assert conv(odd, Q, R, 2, 9, 7, 64, 64, 3, 1, 1, 1, P, BIG, None) == E_ALIGN
    assert conv(P, Q, odd, 2, 9, 7, 64, 64, 3, 1, 1, 1, P, BIG, None) == E_ALIGN
    assert conv(P, Q, R, 2, 9, 7, 64, 64, 3, 1, 1, 1, p(a + 16), BIG, None) == E_ALIGN       # workspace: 256 bytes
    assert conv(P, Q, R, 2, 9, 7, 64, 64, 3, 1, 1, 1, P, 64 * 64 * 9 * 2 - 1, None) == E_WORKSPACE

    # norm: (x, idn, y, B, H, W, C, relu, kind, ws, ws_bytes, stream); pool: (x, idn, feats, B, H, W, C, kind, ws, ws_bytes, stream)
    norm, pool = L.dsmil_trunk16_norm, L.dsmil_trunk16_pool
    assert norm(None, None, Q, 2, 7, 7, 512, 1, 1, R, BIG, None) == E_INVALID
    assert norm(P, None, None, 2, 7, 7, 512, 1, 1, R, BIG, None) == E_INVALID
    assert norm(P, None, Q, 2, 7, 7, 512, 1, 1, None, BIG, None) == E_INVALID
    assert norm(P, None, Q, 2, 7, 7, 512, 2, 1, R, BIG, None) == E_INVALID                  # relu is 0 or 1
    assert norm(P, None, Q, 2, 7, 7, 516, 1, 1, R, BIG, None) == E_UNSUPPORTED              # C % 8
    assert norm(P, None, Q, 2, 7, 7, 24, 1, 1, R, BIG, None) == E_UNSUPPORTED               # C / 8 does not divide 256
    assert norm(P, None, Q, 2, 7, 7, 4096, 1, 1, R, BIG, None) == E_UNSUPPORTED
    assert norm(P, Q, Q, 2, 7, 7, 512, 0, 1, R, BIG, None) == E_UNSUPPORTED                 # residual without ReLU
    assert norm(P, odd, Q, 2, 7, 7, 512, 1, 1, R, BIG, None) == E_ALIGN
    assert norm(P, None, Q, 2, 7, 7, 512, 1, 1, p(a + 16), BIG, None) == E_ALIGN
    assert norm(P, None, Q, 2, 7, 7, 512, 1, 1, R, 1024, None) == E_WORKSPACE
    assert pool(P, None, Q, 2, 7, 7, 512, 1, R, BIG, None) == E_INVALID                     # the pool always adds an identity
    assert pool(P, Q, None, 2, 7, 7, 512, 1, R, BIG, None) == E_INVALID
    assert pool(P, Q, R, 2, 7, 7, 516, 1, R, BIG, None) == E_UNSUPPORTED
    assert pool(odd, Q, R, 2, 7, 7, 512, 1, R, BIG, None) == E_ALIGN
    assert pool(P, Q, R, 2, 7, 7, 512, 1, R, 1024, None) == E_WORKSPACE

    # trunk: (depth, x, B, Hp, Wp, conv_w, feats, kind, ws, ws_bytes, stream)
    fwd = L.dsmil_trunk16_forward
    w18 = (ctypes.c_void_p * 20)(*([None] + [a] * 19))                  # entry 0, the stem's, is not read
    assert fwd(18, None, 3, 9, 9, w18, Q, 1, R, BIG, None) == E_INVALID
    assert fwd(18, P, 3, 9, 9, None, Q, 1, R, BIG, None) == E_INVALID
    assert fwd(18, P, 3, 9, 9, w18, Q, 1, None, BIG, None) == E_INVALID
    assert fwd(18, P, 3, 9, 9, w18, Q, 4, R, BIG, None) == E_INVALID
    assert fwd(18, P, 3, 9, 9, (ctypes.c_void_p * 20)(*([a] * 10 + [None] + [a] * 9)), Q, 1, R, BIG, None) == E_INVALID
    assert fwd(50, P, 3, 9, 9, w18, Q, 1, R, BIG, None) == E_UNSUPPORTED and fwd(19, P, 3, 9, 9, w18, Q, 1, R, BIG, None) == E_UNSUPPORTED
    assert fwd(18, P, 3, 9, 127, w18, Q, 1, R, BIG, None) == E_UNSUPPORTED                  # layer 1 wider than k_conv_b16n's window
    assert fwd(18, P, 3, 1, 1, w18, Q, 1, R, BIG, None) == E_UNSUPPORTED                    # layer 4's 512 channels outgrow the buffers
    assert fwd(18, odd, 3, 9, 9, w18, Q, 1, R, BIG, None) == E_ALIGN
    assert fwd(18, P, 3, 9, 9, w18, Q, 1, p(a + 16), BIG, None) == E_ALIGN
    assert fwd(18, P, 3, 9, 9, w18, Q, 1, R, L.dsmil_trunk16_workspace_bytes(18, 3, 9, 9) - 1, None) == E_WORKSPACE
