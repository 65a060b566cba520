"""The bars of tests/conv_bwd_cases.py are reachable and sharp, without a device: a numpy emulation of the stated arithmetic (two
fp16 planes, three products, fp32 accumulation inside a chunk, partials in chunk order, dy scaled by the documented rule) meets
every bar on every case and is bit-exact on the EXACT cases; the mutants — one plane, either cross product dropped, dy unscaled
— are not.  And the module layer: NativeConv2d on CPU tensors is nn.Conv2d, use_native_convs keeps the state dict, a swapped
ResNet-18 still answers resnet_convs_of; the model-level check's yardstick stays below 1e-4 for the chosen seed.  CPU only."""
import numpy as np
import pytest
import torch
import torch.nn as nn

import conv_bwd_cases as cc
import dsmil  # noqa: F401  (registers the dsmil_wsi_amd package)
from dsmil_wsi_amd import modules, simclr
from dsmil_wsi_amd.resnet import resnet18


@pytest.mark.parametrize("name", [c[0] for c in cc.CASES])
def test_emulated_weight_gradient_meets_the_bar(name):
    x, st, w, dy, ks, stride, pad = cc.case(name)
    for norm in ((False, True) if st is not None else (False,)):
        ref, bar = cc.weight_expected(name, norm)
        got = cc.emulate_weight(x, st if norm else None, dy, ks, stride, pad, cc.WEIGHT_PLANS[name][3]).astype(np.float64)
        wst = cc.worst(np.abs(got - ref), bar)
        print(f"{name} norm={norm}: max err {np.abs(got - ref).max():.3e}, worst err / bar {wst:.3f}")
        assert wst <= 1


@pytest.mark.parametrize("name", [c[0] for c in cc.DATA_CASES])
def test_emulated_data_gradient_meets_the_bar(name):
    x, _, w, dy, ks, stride, pad = cc.case(name)
    ref, bar = cc.data_expected(name)
    got = cc.emulate_data(dy, w, x.shape[2], x.shape[3], stride, pad).astype(np.float64)
    wst = cc.worst(np.abs(got - ref), bar)
    print(f"{name}: max err {np.abs(got - ref).max():.3e}, worst err / bar {wst:.3f}")
    assert wst <= 1
    if stride == 2 and ks == 1:
        assert np.all(got[:, :, 1::2, :] == 0) and np.all(got[:, :, :, 1::2] == 0)


def _emulate_exact(name, mutant=None):
    which, x, w, dy, ks, stride, pad, ref = cc.exact_case(name)
    if which == "data":
        return cc.emulate_data(dy, w, x.shape[2], x.shape[3], stride, pad, mutant), ref
    return cc.emulate_weight(x, None, dy, ks, stride, pad, 256, mutant), ref


@pytest.mark.parametrize("name", [c[0] for c in cc.EXACT_CASES])
def test_emulation_is_exact_on_the_exact_cases(name):
    got, ref = _emulate_exact(name)
    assert np.array_equal(got.astype(np.float64), ref)


@pytest.mark.parametrize("which", ["data", "weight"])
def test_each_kept_product_is_necessary(which):
    x = {"data": "xd", "weight": "xw"}[which]
    for name, mutant, breaks in [(x + "_dywide", "drop_h1w0", True), (x + "_dywide", "drop_h0w1", False),
                                 (x + "_owide", "drop_h0w1", True), (x + "_owide", "drop_h1w0", False),
                                 (x + "_dywide", "one_plane", True), (x + "_owide", "one_plane", True)]:
        got, ref = _emulate_exact(name, mutant)
        assert (not np.array_equal(got.astype(np.float64), ref)) == breaks, (name, mutant)


@pytest.mark.parametrize("mutant", cc.MUTANTS)
def test_the_bars_see_the_mutants(mutant):
    """Each mutant misses the bar of both directions: the plane mutants on an O(1) case, the unscaled dy on a 1e-6 case (its
    elements lie below fp16's normal range)."""
    name = "a_5x7" if mutant == "unscaled" else "b_7x5"
    x, st, w, dy, ks, stride, pad = cc.case(name)
    ref, bar = cc.weight_expected(name, False)
    ww = cc.worst(np.abs(cc.emulate_weight(x, None, dy, ks, stride, pad, 256, mutant).astype(np.float64) - ref), bar)
    ref, bar = cc.data_expected(name)
    wd = cc.worst(np.abs(cc.emulate_data(dy, w, x.shape[2], x.shape[3], stride, pad, mutant).astype(np.float64) - ref), bar)
    print(f"{mutant} on {name}: weight {ww:.2f}, data {wd:.2f} bars")
    assert ww > 1 and wd > 1


def test_the_scale_rule():
    assert cc.scale_of(np.array([0.0])) == 0
    assert cc.scale_of(np.array([1.0, -3.0])) == 12 and cc.scale_of(np.array([2.0 ** -20])) == 33
    assert cc.scale_of(np.array([1e-38])) == 60 and cc.scale_of(np.array([3e38])) == -60
    for name in [c[0] for c in cc.CASES]:
        dy = cc.case(name)[3]
        top = np.abs(dy).max() * 2.0 ** cc.scale_of(dy)
        assert 2.0 ** 13 <= top < 2.0 ** 14
    assert {cc.scale_of(cc.case(c[0])[3]) > 20 for c in cc.CASES} == {True, False}       # both magnitudes are drawn


# ---- the module layer on the CPU --------------------------------------------------------------------------------------------
def test_native_conv2d_on_cpu_is_conv2d():
    torch.manual_seed(3)
    for args, kw in [((64, 64, 3), dict(stride=1, padding=1, bias=False)), ((64, 128, 1), dict(stride=2, bias=False)),
                     ((16, 64, 3), dict(padding=1, bias=True)), ((3, 64, 7), dict(stride=2, padding=3, bias=False))]:
        ref = nn.Conv2d(*args, **kw)
        nat = simclr.NativeConv2d(*args, **kw)
        assert list(nat.state_dict()) == list(ref.state_dict())
        nat.load_state_dict(ref.state_dict())
        x = torch.randn(2, args[0], 9, 7, requires_grad=True)
        x2 = x.detach().clone().requires_grad_(True)
        y, y2 = ref(x), nat(x2)
        assert torch.equal(y, y2)
        g = torch.randn_like(y)
        y.backward(g)
        y2.backward(g)
        assert torch.equal(x.grad, x2.grad) and torch.equal(ref.weight.grad, nat.weight.grad)


def _resnet():
    m = resnet18(norm_layer=nn.InstanceNorm2d)
    m.fc = nn.Identity()
    return m


def test_use_native_convs_keeps_the_state_dict_and_the_parameters():
    m = _resnet()
    before = {k: v.clone() for k, v in m.state_dict().items()}
    params = {n: p for n, p in m.named_parameters()}
    assert simclr.use_native_convs(m) == 20
    after = m.state_dict()
    assert list(after) == list(before) and all(torch.equal(after[k], before[k]) for k in before)
    assert all(p is params[n] for n, p in m.named_parameters()) and len(list(m.named_parameters())) == len(params)
    assert sum(isinstance(c, simclr.NativeConv2d) for c in m.modules()) == 20
    assert simclr.use_native_convs(m) == 0                                             # nothing left to swap
    # ineligible convs stay: a bias, a group, a dilation, a width the kernels do not take
    odd = nn.Sequential(nn.Conv2d(64, 64, 3, bias=True), nn.Conv2d(64, 64, 3, groups=2, bias=False),
                        nn.Conv2d(64, 64, 3, dilation=2, bias=False), nn.Conv2d(64, 32, 1, bias=False),
                        nn.Conv2d(8, 64, 1, bias=False), nn.Conv2d(64, 64, 5, padding=2, bias=False))
    assert simclr.use_native_convs(odd) == 0


def test_a_swapped_resnet_still_answers_resnet_convs_of():
    m = _resnet()
    plain = modules.resnet_convs_of(m)
    simclr.use_native_convs(m)
    got = modules.resnet_convs_of(m)
    assert plain is not None and got is not None
    assert len(got[0]) == len(plain[0]) == 20 and all(a is b for a, b in zip(got[0], plain[0])) and got[1] is None
    x = torch.rand(1, 3, 64, 64)
    with torch.no_grad():
        assert torch.equal(m(x), m(x))


def test_the_model_check_has_a_clean_yardstick():
    """The seed of the model-level check: no ReLU / max-pool decision flips between fp32 and fp64 (every yardstick below 1e-4)
    and every fp64 gradient is nonzero."""
    g64 = cc.model_weight_grads(torch.float64)
    yard = cc.rel_errors(cc.model_weight_grads(torch.float32), g64)
    print("yardstick:", " ".join(f"{v:.2e}" for v in yard))
    assert all(np.linalg.norm(g) > 0 for g in g64)
    assert max(yard) < 1e-4
