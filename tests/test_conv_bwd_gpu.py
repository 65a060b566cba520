"""The conv backward kernels (csrc/conv_bwd.hip) through ops.conv_backward_weight / conv_backward_data against fp64 at the derived
bars of tests/conv_bwd_cases.py (tests/test_conv_bwd_host.py shows the stated arithmetic reaches them and that they see the
mutants): every element is compared; the exact cases bit for bit; two calls bit-identical, also on another stream and over a
workspace full of NaN.  Then through simclr.NativeConv2d, and once through a whole ResNet-18 against the fp32 CPU yardstick."""
import numpy as np
import pytest
import torch
import torch.nn as nn

import conv_bwd_cases as cc
import dsmil
from dsmil_wsi_amd import ops, simclr
from dsmil_wsi_amd.resnet import resnet18

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _nhwc(a):
    return _dev(np.asarray(a).transpose(0, 2, 3, 1))


def _nchw64(t):
    return t.cpu().numpy().transpose(0, 3, 1, 2).astype(np.float64)


def _nan_ws(which, x, w, stride, pad):
    B, Cin, H, W = x.shape
    need = ops._native.lib().dsmil_conv_bwd_workspace_bytes(Cin, w.shape[0], w.shape[2], stride, pad, B, H, W, ops.CONV_BWD_WHICH[which])
    return torch.full(((need + 3) // 4,), float("nan"), dtype=torch.float32, device=DEV).view(torch.uint8)


def _assert_weight_plan(name):
    _, B, H, W, Cin, Cout, ks, stride, pad, _, _ = cc.BY_NAME[name]
    p = ops.conv_backward_plan(Cin, Cout, ks, stride, pad, B, H, W, "weight")
    assert (p["grid_x"], p["grid_y"], p["grid_z"], p["chunk"], p["n_partials"], p["run_len"], p["cols_pad"]) == cc.WEIGHT_PLANS[name]


@pytest.mark.parametrize("name,norm", [(c[0], False) for c in cc.CASES] + [(n, True) for n in cc.NORM_CASES])
def test_weight_gradient_against_fp64(name, norm):
    _assert_weight_plan(name)
    x, st, w, dy, ks, stride, pad = cc.case(name)
    ref, bar = cc.weight_expected(name, norm)
    ist = tuple(_dev(t) for t in st) if norm else None
    xd, dyd = _nhwc(x), _nhwc(dy)
    dw = ops.conv_backward_weight(xd, dyd, ks, stride, pad, in_stats=ist)
    got = dw.cpu().numpy().astype(np.float64)
    assert got.shape == ref.shape
    err = np.abs(got - ref)
    wst = cc.worst(err, bar)
    print(f"{name} norm={norm}: max err {err.max():.3e} worst err / bar {wst:.4f}")
    assert wst <= 1
    dw2 = ops.conv_backward_weight(xd, dyd, ks, stride, pad, in_stats=ist, ws=_nan_ws("weight", x, w, stride, pad))
    assert torch.equal(dw, dw2)                                   # no atomics, nothing read from a stale workspace


@pytest.mark.parametrize("name", [c[0] for c in cc.DATA_CASES])
def test_data_gradient_against_fp64(name):
    x, _, w, dy, ks, stride, pad = cc.case(name)
    _, B, H, W, Cin, Cout = cc.BY_NAME[name][:6]
    p = ops.conv_backward_plan(Cin, Cout, ks, stride, pad, B, H, W, "data")
    assert (p["grid_x"], p["grid_y"], p["run_len"]) == cc.DATA_PLANS[name]
    ref, bar = cc.data_expected(name)
    dyd, wd = _nhwc(dy), _dev(w)
    dx = ops.conv_backward_data(dyd, wd, H, W, stride, pad)
    got = _nchw64(dx)
    assert got.shape == ref.shape
    err = np.abs(got - ref)
    wst = cc.worst(err, bar)
    print(f"{name}: max err {err.max():.3e} worst err / bar {wst:.4f}")
    assert wst <= 1
    if ks == 1 and stride == 2:                                   # pixels no output reads: exact zeros, not small numbers
        assert np.all(got[:, :, 1::2, :] == 0) and np.all(got[:, :, :, 1::2] == 0)
        assert np.any(got[:, :, 0::2, 0::2] != 0)
    dx2 = ops.conv_backward_data(dyd, wd, H, W, stride, pad, ws=_nan_ws("data", x, w, stride, pad))
    assert torch.equal(dx, dx2)


def test_the_stems_data_gradient_is_refused():
    x, _, w, dy, ks, stride, pad = cc.case("s_33x37")
    with pytest.raises(NotImplementedError):
        ops.conv_backward_data(_nhwc(dy), _dev(w), x.shape[2], x.shape[3], stride, pad)


@pytest.mark.parametrize("name", [c[0] for c in cc.EXACT_CASES])
def test_exact_cases_bit_for_bit(name):
    which, x, w, dy, ks, stride, pad, ref = cc.exact_case(name)
    if which == "data":
        got = _nchw64(ops.conv_backward_data(_nhwc(dy), _dev(w), x.shape[2], x.shape[3], stride, pad))
    else:
        got = ops.conv_backward_weight(_nhwc(x), _nhwc(dy), ks, stride, pad).cpu().numpy().astype(np.float64)
    assert np.array_equal(got, ref), f"{name}: {np.count_nonzero(got != ref)} of {ref.size} differ, max {np.abs(got - ref).max():.3e}"


@pytest.mark.parametrize("name", ["a_14", "b_7x5"])
def test_calls_are_bit_identical_on_another_stream(name):
    x, st, w, dy, ks, stride, pad = cc.case(name)
    xd, dyd, wd = _nhwc(x), _nhwc(dy), _dev(w)
    ist = tuple(_dev(t) for t in st) if st is not None else None
    dw0 = ops.conv_backward_weight(xd, dyd, ks, stride, pad, in_stats=ist)
    dx0 = ops.conv_backward_data(dyd, wd, x.shape[2], x.shape[3], stride, pad)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        dw1 = ops.conv_backward_weight(xd, dyd, ks, stride, pad, in_stats=ist)
        dx1 = ops.conv_backward_data(dyd, wd, x.shape[2], x.shape[3], stride, pad)
    side.synchronize()
    assert torch.equal(dw0, dw1) and torch.equal(dx0, dx1)


# ---- through the module -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["a_8x6", "b_7x5"])
@pytest.mark.parametrize("channels_last", [True, False])
def test_native_conv2d_against_fp64(name, channels_last):
    x, _, w, dy, ks, stride, pad = cc.case(name)
    _, B, H, W, Cin, Cout = cc.BY_NAME[name][:6]
    ref_m = nn.Conv2d(Cin, Cout, ks, stride, pad, bias=False).to(DEV)
    nat_m = simclr.NativeConv2d(Cin, Cout, ks, stride, pad, bias=False).to(DEV)
    with torch.no_grad():
        ref_m.weight.copy_(_dev(w))
    nat_m.weight = ref_m.weight                                   # shared
    xs = []
    losses, scale = [], []
    c = _dev(dy)                                                  # loss = <dy, y>: the upstream gradient is the case's dy
    for m in (ref_m, nat_m):
        xt = _dev(x)
        if channels_last:
            xt = xt.contiguous(memory_format=torch.channels_last)
        xt.requires_grad_(True)
        ref_m.weight.grad = None
        y = m(xt)
        assert y.shape == (B, Cout) + tuple(c.shape[2:])
        loss = (y * c).sum()
        loss.backward()
        losses.append(loss.item())
        scale.append((y.detach() * c).abs().sum().item())
        xs.append((xt.grad.detach().clone(), ref_m.weight.grad.detach().clone()))
    assert abs(losses[0] - losses[1]) <= 1e-5 * scale[0]          # two fp32-class forwards of one sum of 1e3 .. 1e4 terms
    gx, gw = xs[1]
    ref_x, bar_x = cc.data_expected(name)
    ref_w, bar_w = cc.weight_expected(name, False)
    wx = cc.worst(np.abs(gx.cpu().numpy().astype(np.float64) - ref_x), bar_x)
    ww = cc.worst(np.abs(gw.cpu().numpy().astype(np.float64) - ref_w), bar_w)
    print(f"{name} channels_last={channels_last}: x.grad {wx:.4f}, weight.grad {ww:.4f} of the bar")
    assert wx <= 1 and ww <= 1
    assert not torch.equal(gw, xs[0][1]) or not torch.equal(gx, xs[0][0])     # the native backward ran, not aten's


def test_native_conv2d_refused_shapes_take_torchs_backward():
    torch.manual_seed(5)
    for args, kw, hw in [((24, 64, 3), dict(padding=1, bias=False), (6, 5)),       # Cin % 16
                         ((64, 64, 3), dict(padding=1, bias=True), (6, 5)),       # a bias
                         ((3, 64, 7), dict(stride=2, padding=3, bias=False), (33, 37))]:   # the stem with an input that requires grad
        ref_m = nn.Conv2d(*args, **kw).to(DEV)
        nat_m = simclr.NativeConv2d(*args, **kw).to(DEV)
        nat_m.load_state_dict(ref_m.state_dict())
        x0 = torch.randn(2, args[0], *hw, device=DEV)
        out = []
        with torch.backends.cudnn.flags(enabled=True, benchmark=False, deterministic=True):   # aten's own two runs must agree
            for m in (ref_m, nat_m):
                xt = x0.clone().requires_grad_(True)
                y = m(xt)
                assert "ConvNative" not in type(y.grad_fn).__name__ and "Convolution" in type(y.grad_fn).__name__
                y.square().sum().backward()
                out.append((y.detach(), xt.grad, m.weight.grad))
        assert [torch.equal(a, b) for a, b in zip(*out)] == [True, True, True], args


# ---- one model-level check --------------------------------------------------------------------------------------------------
def test_resnet18_weight_gradients_against_the_fp32_yardstick():
    """Per conv, ||g - g64|| / ||g64|| of the native run (use_native_convs, GPU) is at most 4 x the same quantity of the plain
    torch fp32 model on the CPU: the form's per-output bound is (3 K + 8) u S against K u S of a plain fp32 sum."""
    g64 = cc.model_weight_grads(torch.float64)
    yard = cc.rel_errors(cc.model_weight_grads(torch.float32), g64)
    assert all(np.linalg.norm(g) > 0 for g in g64) and max(yard) < 1e-4
    nat = cc.rel_errors(cc.model_weight_grads(torch.float32, device=DEV, native=True), g64)
    ratios = [a / b for a, b in zip(nat, yard)]
    for i, (a, b, r) in enumerate(zip(nat, yard, ratios)):
        print(f"conv {i:2d}: native {a:.3e} yardstick {b:.3e} ratio {r:.3f}")
    assert max(ratios) <= cc.MODEL_MARGIN


def test_iclassifier_inference_is_untouched_by_the_swap():
    from dsmil_wsi_amd.synthetic import make_patches, make_resnet18_weights
    feats = []
    for swap in (False, True):
        res = resnet18(norm_layer=nn.InstanceNorm2d)
        res.fc = nn.Identity()
        res.load_state_dict({k: torch.as_tensor(np.asarray(v)) for k, v in make_resnet18_weights(11).items()}, strict=True)
        if swap:
            assert simclr.use_native_convs(res) == 20
        torch.manual_seed(0)
        ic = dsmil.IClassifier(res, 512, output_class=2).eval().to(DEV)
        with torch.no_grad():
            f, c = ic(torch.from_numpy(make_patches(5, 2, 96, 96)).to(DEV))
        feats.append((f.clone(), c.clone()))
    assert torch.equal(feats[0][0], feats[1][0]) and torch.equal(feats[0][1], feats[1][1])
