"""The conv backward entries (dsmil_conv_bwd_*: csrc/conv_bwd.hip) are declared, exported and bound — additive, ABI still 6 —;
their size query, plan and refusals answer without a device (every check runs before the first launch); and the plan of every
case of tests/conv_bwd_cases.py is PINNED, so the run_len / n_partials the bars are formed from are declarations, not results.
CPU only."""
import ctypes
import os
import re

import pytest

import conv_bwd_cases as cc
import dsmil  # noqa: F401  (registers the dsmil_wsi_amd package)
import dsmil_wsi_amd._native as nat
from dsmil_wsi_amd import ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("dsmil_conv_bwd_plan", "dsmil_conv_bwd_workspace_bytes", "dsmil_conv_bwd_weight", "dsmil_conv_bwd_data")
E_INVALID, E_UNSUPPORTED, E_WORKSPACE, E_ALIGN = -1, -2, -3, -5
BIG = 1 << 30


def test_conv_bwd_symbols_are_declared_exported_and_bound():
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
    for name, B, H, W, Cin, Cout, ks, stride, pad, _, _ in cc.CASES:
        p = ops.conv_backward_plan(Cin, Cout, ks, stride, pad, B, H, W, "weight")
        got = (p["grid_x"], p["grid_y"], p["grid_z"], p["chunk"], p["n_partials"], p["run_len"], p["cols_pad"])
        assert got == cc.WEIGHT_PLANS[name], (name, got)
        Ho, Wo = cc.out_size(H, ks, stride, pad), cc.out_size(W, ks, stride, pad)
        M = B * Ho * Wo
        assert (p["Ho"], p["Wo"], p["out_rows"], p["out_cols"], p["block"]) == (Ho, Wo, Cout, Cin * ks * ks, 256)
        assert p["n_partials"] == p["grid_z"] == -(-M // p["chunk"]) and p["run_len"] == min(M, p["chunk"])
        assert p["cols_pad"] % 64 == 0 and 0 <= p["cols_pad"] - Cin * ks * ks < 64
        if Cin == 3:
            with pytest.raises(NotImplementedError):
                ops.conv_backward_plan(Cin, Cout, ks, stride, pad, B, H, W, "data")
            assert name not in cc.DATA_PLANS
            continue
        p = ops.conv_backward_plan(Cin, Cout, ks, stride, pad, B, H, W, "data")
        assert (p["grid_x"], p["grid_y"], p["run_len"]) == cc.DATA_PLANS[name], (name, p)
        assert (p["Ho"], p["Wo"], p["out_rows"], p["out_cols"], p["grid_z"], p["n_partials"], p["chunk"]) == (Ho, Wo, B * H * W, Cin, 1, 1, 0)
        assert p["run_len"] == Cout * ks * ks
    # the conditions the case names claim
    P = cc.WEIGHT_PLANS
    assert P["a_14"][4] > 1 and P["l_28"][4] == 49 and P["s_33x37"][6] == 192 and P["a_1x1"][5] == 1
    # a large layer: the chunk grows until chunks x tiles fits the target, and stops at 4096 positions
    p = ops.conv_backward_plan(64, 64, 3, 1, 1, 256, 56, 56, "weight")
    assert (p["chunk"], p["n_partials"], p["run_len"]) == (4096, 196, 4096)
    # a narrow one (two tiles): the chunk grows until an element is summed from at most 256 partials
    p = ops.conv_backward_plan(64, 128, 1, 2, 0, 256, 56, 56, "weight")
    assert (p["chunk"], p["n_partials"], p["grid_x"], p["grid_y"]) == (1024, 196, 1, 2)
    # the data gradient at stride 2 tiles each of the four parity classes of the 56 x 56 input on its own
    p = ops.conv_backward_plan(64, 128, 1, 2, 0, 256, 56, 56, "data")
    assert p["grid_x"] == 4 * (256 * 28 * 28 // 64) and p["out_rows"] == 256 * 56 * 56
    for name, which, B, H, W, Cin, Cout, ks, stride, pad, _ in cc.EXACT_CASES:
        p = ops.conv_backward_plan(Cin, Cout, ks, stride, pad, B, H, W, which)
        assert p["chunk"] in (0, 256)                      # what the emulation of the exact cases assumes


def test_conv_bwd_sizes_without_a_device():
    wb = nat.lib().dsmil_conv_bwd_workspace_bytes
    for name, B, H, W, Cin, Cout, ks, stride, pad, _, _ in cc.CASES:
        p = cc.WEIGHT_PLANS[name]
        assert wb(Cin, Cout, ks, stride, pad, B, H, W, 0) >= p[4] * Cout * p[6] * 4 + 8
        if Cin != 3:
            assert wb(Cin, Cout, ks, stride, pad, B, H, W, 1) >= Cout * Cin * ks * ks * 4 + 8
    assert wb(3, 64, 7, 2, 3, 2, 33, 37, 1) == 0                                        # the stem's data gradient
    assert wb(64, 64, 3, 1, 1, 2, 5, 7, 2) == 0 and wb(64, 64, 3, 1, 1, 0, 5, 7, 0) == 0


REFUSED = [(60, 64, 3, 1, 1), (8, 64, 3, 1, 1), (64, 96, 3, 1, 1), (64, 32, 1, 1, 0),          # Cin % 16, Cout % 64
           (64, 64, 5, 1, 2), (64, 64, 2, 1, 0), (64, 64, 3, 3, 1), (64, 64, 3, 1, 2), (64, 64, 1, 1, 1)]   # ks, stride, pad


def test_conv_bwd_refusals_without_a_device():
    L = nat.lib()
    buf = (ctypes.c_char * 8192)()
    a = (ctypes.addressof(buf) + 255) // 256 * 256
    p = ctypes.c_void_p
    P, Q, R, S, T, odd4 = p(a), p(a + 256), p(a + 512), p(a + 768), p(a + 1024), p(a + 4)
    plan = (ctypes.c_int32 * 16)()
    cp, wb = L.dsmil_conv_bwd_plan, L.dsmil_conv_bwd_workspace_bytes
    assert cp(64, 64, 3, 1, 1, 2, 5, 7, 0, None) == E_INVALID and cp(64, 64, 3, 1, 1, 0, 5, 7, 0, plan) == E_INVALID
    assert cp(64, 64, 3, 1, 1, 2, 5, 7, 2, plan) == E_INVALID and cp(64, 64, 3, 1, -1, 2, 5, 7, 0, plan) == E_INVALID

    # weight: (x, in_mean, in_rstd, dy, dw, B, H, W, Cin, Cout, ks, stride, pad, ws, ws_bytes, stream)
    wg = L.dsmil_conv_bwd_weight
    ok = (2, 5, 7, 64, 64, 3, 1, 1)
    assert wg(None, None, None, Q, R, *ok, P, BIG, None) == E_INVALID
    assert wg(P, None, None, None, R, *ok, P, BIG, None) == E_INVALID
    assert wg(P, None, None, Q, None, *ok, P, BIG, None) == E_INVALID
    assert wg(P, None, None, Q, R, *ok, None, BIG, None) == E_INVALID
    assert wg(P, S, None, Q, R, *ok, T, BIG, None) == E_INVALID                           # in_mean without in_rstd
    assert wg(P, None, None, Q, R, 2, 0, 7, 64, 64, 3, 1, 1, T, BIG, None) == E_INVALID
    # data: (dy, w, dx, B, H, W, Cin, Cout, ks, stride, pad, ws, ws_bytes, stream)
    dg = L.dsmil_conv_bwd_data
    assert dg(None, Q, R, *ok, P, BIG, None) == E_INVALID
    assert dg(P, None, R, *ok, T, BIG, None) == E_INVALID
    assert dg(P, Q, None, *ok, T, BIG, None) == E_INVALID
    assert dg(P, Q, R, *ok, None, BIG, None) == E_INVALID
    for cin, cout, ks, stride, pad in REFUSED:
        shape = (2, 5, 7, cin, cout, ks, stride, pad)
        assert wg(P, None, None, Q, R, *shape, T, BIG, None) == E_UNSUPPORTED, shape
        assert dg(P, Q, R, *shape, T, BIG, None) == E_UNSUPPORTED, shape
        for which in (0, 1):
            assert cp(cin, cout, ks, stride, pad, 2, 5, 7, which, plan) == E_UNSUPPORTED
            assert wb(cin, cout, ks, stride, pad, 2, 5, 7, which) == 0
    assert dg(P, Q, R, 2, 33, 37, 3, 64, 7, 2, 3, T, BIG, None) == E_UNSUPPORTED            # the stem's data gradient
    assert cp(3, 64, 7, 2, 3, 2, 33, 37, 0, plan) == 0 and cp(3, 64, 7, 2, 3, 2, 33, 37, 1, plan) == E_UNSUPPORTED
    assert wg(P, None, None, Q, R, 1, 2, 2, 64, 64, 3, 1, 0, T, BIG, None) == E_UNSUPPORTED  # no output pixel
    assert wg(P, None, None, Q, R, 40, 1024, 1024, 64, 64, 3, 1, 1, T, BIG, None) == E_UNSUPPORTED   # 2^31 elements
    assert dg(P, Q, R, 40, 1024, 1024, 64, 64, 3, 1, 1, T, BIG, None) == E_UNSUPPORTED
    assert wg(odd4, None, None, Q, R, *ok, T, BIG, None) == E_ALIGN
    assert wg(P, None, None, odd4, R, *ok, T, BIG, None) == E_ALIGN
    assert wg(P, odd4, S, Q, R, *ok, T, BIG, None) == E_ALIGN
    assert wg(P, None, None, Q, R, *ok, p(a + 16), BIG, None) == E_ALIGN
    assert dg(odd4, Q, R, *ok, T, BIG, None) == E_ALIGN and dg(P, Q, odd4, *ok, T, BIG, None) == E_ALIGN
    assert dg(P, Q, R, *ok, p(a + 16), BIG, None) == E_ALIGN
    assert wg(P, None, None, Q, R, *ok, T, wb(64, 64, 3, 1, 1, 2, 5, 7, 0) - 1, None) == E_WORKSPACE
    assert dg(P, Q, R, *ok, T, wb(64, 64, 3, 1, 1, 2, 5, 7, 1) - 1, None) == E_WORKSPACE


def test_python_wrappers_raise_not_implemented_for_refused_shapes():
    for cin, cout, ks, stride, pad in REFUSED:
        for which in ("weight", "data"):
            with pytest.raises(NotImplementedError):
                ops.conv_backward_plan(cin, cout, ks, stride, pad, 2, 5, 7, which)
            assert not ops.conv_backward_supported(cin, cout, ks, stride, pad, 2, 5, 7, which)
    assert ops.conv_backward_supported(3, 64, 7, 2, 3, 2, 33, 37, "weight")
    assert not ops.conv_backward_supported(3, 64, 7, 2, 3, 2, 33, 37, "data")
