"""The test entries of the fp32-class trunk (dsmil_trunk32_*: the stages of csrc/resnet_fwd.hip / csrc/wino_w1.h alone) are
declared, exported and bound — additive, ABI still 6 —; their size queries and refusals answer without a device (every check runs
before the first launch, in the documented order); and the plan of every case of tests/trunk32_cases.py is PINNED: a change of
wino_shape or of the tile choice shows up here as a diff instead of as a case that silently no longer reaches the launch condition
it is named for.  CPU only."""
import ctypes
import os
import re

import dsmil  # noqa: F401  (registers the dsmil_wsi_amd package)
import dsmil_wsi_amd._native as nat
import trunk32_cases as tc
from dsmil_wsi_amd import ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("dsmil_trunk32_conv_plan", "dsmil_trunk32_conv_workspace_bytes", "dsmil_trunk32_conv", "dsmil_trunk32_stem_workspace_bytes",
           "dsmil_trunk32_stem", "dsmil_trunk32_tail")
E_INVALID, E_UNSUPPORTED, E_WORKSPACE, E_ALIGN = -1, -2, -3, -5
BIG = 1 << 30


def test_trunk32_symbols_are_declared_exported_and_bound():
    text = open(os.path.join(ROOT, "include", "dsmil_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    lib = ctypes.CDLL(nat.LIB_PATH)
    for name in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, src), f"{name} is not declared in include/dsmil_hip.h"
        assert hasattr(lib, name), f"{name} is not exported"
        assert name in nat.SIGNATURES, f"{name} is not in the binding table"
    assert int(re.search(r"#define DSMIL_ABI_VERSION (\d+)", text).group(1)) == 6
    assert nat.lib().dsmil_abi_version() == 6
    block = text[:text.index("#define DSMIL_T32_W1")]
    assert "FOR TESTS" in block[block.rindex("/*"):]


def test_the_plan_of_every_case_is_pinned():
    for precision in tc.PRECISIONS:
        for name, B, H, W, Cin, Cout, norm in tc.WINO_CASES:
            p = ops.trunk32_conv_plan(Cin, Cout, 3, 1, 1, B, H, W, norm, precision)
            got = (p["kernel"], p["IB"], p["TYB"], p["TXB"], p["nby"], p["nbx"], p["grid_x"], p["grid_y"])
            assert got == tc.WINO_PLANS[name], (name, precision, got)
            assert (p["Ho"], p["Wo"], p["tile"], p["nslots"], p["block"]) == (H, W, 0, 0, 256)
            assert p["IB"] * (2 * p["TYB"] + 2) * (2 * p["TXB"] + 2) <= 256 and p["IB"] * p["TYB"] * p["TXB"] <= 32
        for name, B, H, W, Cin, Cout, ks, stride, pad, norm in tc.DIRECT_CASES:
            p = ops.trunk32_conv_plan(Cin, Cout, ks, stride, pad, B, H, W, norm, precision)
            got = (p["tile"], p["Ho"], p["Wo"], p["nslots"], p["grid_x"], p["grid_y"])
            assert p["kernel"] == "s6" and got == tc.DIRECT_PLANS[name], (name, precision, got)
            assert p["products"] == (3 if precision == "fp32" else 1)
    # the conditions the case names claim
    P = tc.WINO_PLANS
    assert P["u_2x61"][1] * 4 * (2 * P["u_2x61"][3] + 2) == 256                      # the raw region is WRAW_MAX exactly
    assert P["u_2x63"][5] == 2 and ops.trunk32_conv_plan(64, 64, 3, 1, 1, 1, 2, 62)["nbx"] == 1   # the narrowest map with nbx > 1
    assert 4 * (2 * 32 + 2) > 256                                                    # ... because TXB = 32 would not fit the raw region
    assert P["u_63x2"][4] == 2 and ops.trunk32_conv_plan(64, 64, 3, 1, 1, 1, 62, 2)["nby"] == 1   # the shortest map with nby > 1
    assert P["u_5x7"][1] == 2 and 3 % P["u_5x7"][1] and P["u_2x2_b40"][1] == 14 and 40 % 14       # batches that do not divide by IB
    assert P["w256_14_g8"][6] % 8 == 0 and P["w256_5x7_g6"][6] % 8 != 0               # both block-to-cout maps of wino_w1.h
    assert P["w32_3x3"][1] == 2 and P["w_5x7"][1] == 1                                # cin < 64: the unit of the utilisation score
    D = tc.DIRECT_PLANS
    assert {D[n][0] for n in D} == {42, 22, 24} and {D[n][3] for n in D} >= {2, 4, 17, 33}
    assert {D[n][1] * D[n][2] for n in D} >= {1, 2, 12, 63}                          # a 32-pixel tile touching 32, 16, 3-4 and 2 images
    # the exact cases reach the kernels they are named for
    for name, B, H, W, Cin, Cout, ks, stride, pad, _ in tc.EXACT_CASES:
        p = ops.trunk32_conv_plan(Cin, Cout, ks, stride, pad, B, H, W)
        assert (p["kernel"], p["tile"]) == {"x42": ("s6", 42), "x22": ("s6", 22), "x24": ("s6", 24), "xu": ("unit", 0), "xw": ("w1", 0)}[name.split("_")[0]]


def test_trunk32_sizes_without_a_device():
    L = nat.lib()
    cw = L.dsmil_trunk32_conv_workspace_bytes
    # packed weights (1.5 floats per weight and transform position / tap) + statistics partials
    assert cw(64, 64, 3, 1, 1, 3, 5, 7, 0) >= 64 * 64 * 24 * 4 + 3 * 1 * 2 * 64 * 3 * 4
    assert cw(64, 128, 3, 2, 1, 3, 7, 5, 0) >= 64 * 128 * 9 * 6 + 2 * 4 * 128 * 2 * 4
    assert cw(64, 64, 3, 1, 1, 3, 5, 7, 2) == 0 and cw(60, 64, 3, 1, 1, 3, 5, 7, 0) == 0 and cw(64, 64, 3, 1, 1, 0, 5, 7, 0) == 0
    sw = L.dsmil_trunk32_stem_workspace_bytes
    assert sw(3, 34, 38) >= 3 * 64 * 184 * 2 + 3 * 17 * 19 * 64 * 4 + 3 * 2 * 2 * 8 * 64 * 3 * 4
    assert sw(3, 31, 38) == 0 and sw(0, 34, 38) == 0


def test_trunk32_refusals_without_a_device():
    L = nat.lib()
    buf = (ctypes.c_char * 8192)()
    a = (ctypes.addressof(buf) + 255) // 256 * 256
    p = ctypes.c_void_p
    P, Q, R, S, T, odd, odd4 = p(a), p(a + 256), p(a + 512), p(a + 768), p(a + 1024), p(a + 2), p(a + 4)
    plan = (ctypes.c_int32 * 16)()

    # plan: (Cin, Cout, ks, stride, pad, B, H, W, norm, precision, out)
    cp = L.dsmil_trunk32_conv_plan
    assert cp(64, 64, 3, 1, 1, 3, 5, 7, 0, 0, None) == E_INVALID and cp(64, 64, 3, 1, 1, 0, 5, 7, 0, 0, plan) == E_INVALID
    assert cp(64, 64, 3, 1, 1, 3, 5, 7, 2, 0, plan) == E_INVALID
    assert cp(64, 64, 3, 1, 1, 3, 5, 7, 0, 2, plan) == E_UNSUPPORTED and cp(64, 64, 3, 1, 1, 3, 5, 7, 0, -1, plan) == E_UNSUPPORTED

    # conv: (x, w, in_mean, in_rstd, bn_m, bn_r, y, mean, rstd, B, H, W, Cin, Cout, ks, stride, pad, precision, ws, ws_bytes, stream)
    conv = L.dsmil_trunk32_conv
    ok = (3, 5, 7, 64, 64, 3, 1, 1, 0)
    assert conv(None, Q, None, None, None, None, R, S, T, *ok, P, BIG, None) == E_INVALID
    assert conv(P, None, None, None, None, None, R, S, T, *ok, P, BIG, None) == E_INVALID
    assert conv(P, Q, None, None, None, None, None, S, T, *ok, P, BIG, None) == E_INVALID
    assert conv(P, Q, None, None, None, None, R, None, T, *ok, P, BIG, None) == E_INVALID
    assert conv(P, Q, None, None, None, None, R, S, T, *ok, None, BIG, None) == E_INVALID
    assert conv(P, Q, None, None, None, None, P, S, T, *ok, R, BIG, None) == E_INVALID                  # in place
    assert conv(P, Q, S, None, None, None, R, S, T, *ok, P, BIG, None) == E_INVALID                     # in_mean without in_rstd
    assert conv(P, Q, None, None, None, T, R, S, T, *ok, P, BIG, None) == E_INVALID                     # bn_r without bn_m
    assert conv(P, Q, None, None, None, None, R, S, T, 3, 0, 7, 64, 64, 3, 1, 1, 0, P, BIG, None) == E_INVALID
    assert conv(P, Q, None, None, None, None, R, S, T, 3, 5, 7, 64, 64, 3, 1, 1, 2, P, BIG, None) == E_UNSUPPORTED      # precision
    for cin, cout, ks, stride, pad in [(60, 64, 3, 1, 1), (8, 64, 3, 1, 1),          # Cin % 16 (the plan alone would take Cin % 8)
                                       (64, 96, 3, 1, 1), (64, 32, 1, 1, 0),         # Cout % 64
                                       (64, 4096, 1, 1, 0), (4096, 64, 1, 1, 0),     # widths over 2048
                                       (64, 64, 5, 1, 2), (64, 64, 2, 1, 0), (64, 64, 3, 3, 1), (64, 64, 3, 1, 2), (64, 64, 1, 1, 1)]:
        assert conv(P, Q, None, None, None, None, R, S, T, 3, 5, 7, cin, cout, ks, stride, pad, 0, P, BIG, None) == E_UNSUPPORTED, (cin, cout, ks)
        assert cp(cin, cout, ks, stride, pad, 3, 5, 7, 0, 0, plan) == E_UNSUPPORTED
    assert conv(P, Q, None, None, None, None, R, S, T, 1, 2, 2, 64, 64, 3, 1, 0, 0, P, BIG, None) == E_UNSUPPORTED      # no output pixel
    assert conv(P, Q, None, None, None, None, R, S, T, 40, 1024, 1024, 64, 64, 3, 1, 1, 0, P, BIG, None) == E_UNSUPPORTED  # 2^31 elements
    assert conv(odd4, Q, None, None, None, None, R, S, T, *ok, P, BIG, None) == E_ALIGN
    assert conv(P, Q, None, None, None, None, odd4, S, T, *ok, P, BIG, None) == E_ALIGN
    assert conv(P, Q, odd4, S, None, None, R, S, T, *ok, P, BIG, None) == E_ALIGN                       # in_mean: 16 bytes
    assert conv(P, odd, None, None, None, None, R, S, T, *ok, P, BIG, None) == E_ALIGN
    assert conv(P, Q, None, None, None, None, R, S, T, *ok, p(a + 16), BIG, None) == E_ALIGN             # workspace: 256 bytes
    need = L.dsmil_trunk32_conv_workspace_bytes(64, 64, 3, 1, 1, 3, 5, 7, 0)
    assert conv(P, Q, None, None, None, None, R, S, T, *ok, P, need - 1, None) == E_WORKSPACE

    # stem: (x, u8, conv1_w, bn_m, bn_r, pooled, mean, rstd, B, H, W, precision, ws, ws_bytes, stream)
    stem = L.dsmil_trunk32_stem
    assert stem(None, 0, Q, None, None, R, S, T, 3, 34, 38, 0, P, BIG, None) == E_INVALID
    assert stem(P, 0, None, None, None, R, S, T, 3, 34, 38, 0, P, BIG, None) == E_INVALID
    assert stem(P, 0, Q, None, None, None, S, T, 3, 34, 38, 0, P, BIG, None) == E_INVALID
    assert stem(P, 0, Q, S, None, R, S, T, 3, 34, 38, 0, P, BIG, None) == E_INVALID                     # bn_m without bn_r
    assert stem(P, 0, Q, None, None, R, S, T, 0, 34, 38, 0, P, BIG, None) == E_INVALID
    assert stem(P, 0, Q, None, None, R, S, T, 3, 34, 38, 3, P, BIG, None) == E_UNSUPPORTED
    assert stem(P, 0, Q, None, None, R, S, T, 3, 31, 38, 0, P, BIG, None) == E_UNSUPPORTED              # H, W >= 32
    assert stem(P, 1, Q, None, None, R, S, T, 3, 34, 31, 0, P, BIG, None) == E_UNSUPPORTED
    assert stem(odd, 0, Q, None, None, R, S, T, 3, 34, 38, 0, P, BIG, None) == E_ALIGN
    assert stem(P, 0, Q, None, None, odd4, S, T, 3, 34, 38, 0, P, BIG, None) == E_ALIGN
    assert stem(P, 0, Q, None, None, R, S, T, 3, 34, 38, 0, p(a + 16), BIG, None) == E_ALIGN
    assert stem(P, 0, Q, None, None, R, S, T, 3, 34, 38, 0, P, L.dsmil_trunk32_stem_workspace_bytes(3, 34, 38) - 1, None) == E_WORKSPACE

    # tail: (kind, y2, m2, r2, idn, md, rd, out, B, HW, C, precision, stream)
    tail = L.dsmil_trunk32_tail
    assert tail(0, None, Q, R, S, None, None, T, 3, 12, 64, 0, None) == E_INVALID
    assert tail(0, P, Q, R, None, None, None, T, 3, 12, 64, 0, None) == E_INVALID
    assert tail(3, P, Q, R, S, None, None, T, 3, 12, 64, 0, None) == E_INVALID
    assert tail(1, P, Q, R, S, None, None, T, 3, 12, 64, 0, None) == E_INVALID                          # the downsample's statistics
    assert tail(0, P, Q, R, S, Q, R, T, 3, 12, 64, 0, None) == E_INVALID                                # ... only there
    assert tail(0, P, Q, R, S, None, None, T, 3, 0, 64, 0, None) == E_INVALID
    assert tail(0, P, Q, R, S, None, None, T, 3, 12, 64, 5, None) == E_UNSUPPORTED
    for C in (62, 96, 1280, 4100):                                                   # C % 4; C / 4 against 256
        assert tail(0, P, Q, R, S, None, None, T, 3, 12, C, 0, None) == E_UNSUPPORTED, C
    assert tail(0, P, Q, R, S, None, None, T, 60000, 1024, 64, 0, None) == E_UNSUPPORTED
    assert tail(0, odd4, Q, R, S, None, None, T, 3, 12, 64, 0, None) == E_ALIGN
    assert tail(1, P, Q, R, S, odd4, R, T, 3, 12, 64, 0, None) == E_ALIGN
    assert tail(0, P, Q, R, S, None, None, odd4, 3, 12, 64, 0, None) == E_ALIGN
    assert tail(2, P, Q, R, S, None, None, odd, 3, 12, 64, 0, None) == E_ALIGN
