"""The training stem on the MI355X.  dsmil_stem_pool_bwd (csrc/stem_bwd.hip) through ops.stem_pool_backward against fp64 at the
derived bars of tests/stem_bwd_cases.py (tests/test_stem_bwd_host.py shows the stated arithmetic reaches them and that they see
the mutants): every element is compared, over a workspace full of NaN; the exact cases — most windows tied at the top — bit for
bit; the exact zeros of one pixel, of a fully masked channel and of g = 0; two calls bit-identical on another stream.
dsmil_trunk32_stem_train against dsmil_trunk32_stem bit for bit, its raw map at trunk32_cases' stem bar, its winners against the
numpy rule applied to what it returned.  Then simclr.use_native_stem: the stem alone and a whole ResNet-18 held to the fp32 CPU
yardstick with conv_bwd_cases.MODEL_MARGIN, the fallbacks, and IClassifier's inference untouched."""
import numpy as np
import pytest
import torch
import torch.nn as nn

import conv_bwd_cases as cc
import norm_bwd_cases as nc
import stem_bwd_cases as sc
import dsmil
from dsmil_wsi_amd import ops, simclr
from dsmil_wsi_amd.resnet import resnet18

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)           # a copy: the cached cases are read-only


def _nan_ws(B, H1, W1, C):
    need = ops._native.lib().dsmil_stem_pool_bwd_workspace_bytes(B, H1, W1, C)
    return torch.full(((need + 3) // 4,), float("nan"), dtype=torch.float32, device=DEV).view(torch.uint8)


def _run(inp, ws=None):
    d = {k: _dev(v) for k, v in inp.items()}
    return ops.stem_pool_backward(d["g"], d["y"], (d["m"], d["r"]), d["win"], ws=ws)


# ---- the backward stage -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [c[0] for c in sc.CASES])
def test_stage_against_fp64_on_a_poisoned_workspace(name):
    _, B, H1, W1, C, _ = sc.BY_NAME[name]
    p = ops.stem_pool_backward_plan(B, H1, W1, C)
    assert (p["Hp"], p["Wp"], p["chunk"], p["n_partials"], p["run_len"], p["lanes"]) == sc.PLANS[name][:6]
    inp = sc.case(name)
    res = _run(inp, ws=_nan_ws(B, H1, W1, C))
    got = res.cpu().numpy()
    wst = sc.worst_ratio(got, sc.expected(name))
    print(f"{name}: worst err / bar {wst:.4f}")
    assert wst <= 1
    if H1 * W1 == 1:                                               # x^ and q are exact zeros
        assert not got.any()
    else:                                                          # the fully masked channel of image 0
        assert got.any() and not got[0, :, :, sc.MASKED_CH].any()
    assert torch.equal(res, _run(inp))                             # nothing read from a stale workspace


@pytest.mark.parametrize("name", [c[0] for c in sc.EXACT_CASES])
def test_exact_cases_bit_for_bit(name):
    inp, ref = sc.exact_case(name)
    a = _run(inp).cpu().numpy().astype(np.float64)
    assert np.array_equal(a, ref), f"{name}: {np.count_nonzero(a != ref)} of {a.size} differ, max {np.abs(a - ref).max():.3e}"


@pytest.mark.parametrize("name", ["p_5x7", "p_16x17", "p_27x26"])
def test_all_zero_gradient_gives_exact_zeros(name):
    inp = dict(sc.case(name))
    inp["g"] = np.zeros_like(inp["g"])
    assert not _run(inp).cpu().numpy().any()


@pytest.mark.parametrize("name", ["p_16x17", "p_27x26", "p_9x9_128"])
def test_calls_are_bit_identical_on_another_stream(name):
    first = _run(sc.case(name))
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        second = _run(sc.case(name))
    side.synchronize()
    assert torch.equal(first, second)


def test_refused_shapes_raise_before_any_launch():
    y = torch.zeros(2, 5, 7, 40, device=DEV)
    g = torch.zeros(2, 3, 4, 40, device=DEV)
    st = (torch.zeros(2, 40, device=DEV), torch.ones(2, 40, device=DEV))
    with pytest.raises(NotImplementedError):
        ops.stem_pool_backward(g, y, st, torch.zeros(2, 3, 4, 40, dtype=torch.uint8, device=DEV))
    with pytest.raises(ValueError):
        ops.stem_pool_backward(g[:, :2], y, st, torch.zeros(2, 2, 4, 40, dtype=torch.uint8, device=DEV))
    with pytest.raises(NotImplementedError):
        ops.trunk32_stem_train(torch.zeros(1, 3, 31, 40, device=DEV), torch.zeros(64, 3, 7, 7, device=DEV))


# ---- the forward that keeps what the backward needs -------------------------------------------------------------------------
@pytest.mark.parametrize("u8", [False, True])
@pytest.mark.parametrize("shape", sc.FWD_SHAPES)
def test_stem_train_forward(shape, u8):
    x, w, s, bar = sc.fwd_case(*shape, u8)
    xd, wd = _dev(x), _dev(w)
    pooled0, mean0, rstd0 = ops.trunk32_stem(xd, wd)
    pooled, y, (mean, rstd), win = ops.trunk32_stem_train(xd, wd)
    assert torch.equal(pooled, pooled0) and torch.equal(mean, mean0) and torch.equal(rstd, rstd0)
    yh = y.cpu().numpy()
    wst = sc.worst(np.abs(yh.astype(np.float64) - s), bar)
    print(f"{shape} u8={u8}: raw map worst err / bar {wst:.4f}")
    assert wst <= 1
    a = sc.a_of(yh, mean.cpu().numpy(), rstd.cpu().numpy())
    assert np.array_equal(win.cpu().numpy(), sc.winners(a))
    assert np.array_equal(pooled.cpu().numpy(), np.maximum(sc._windows(a).max(0), np.float32(0)))


# ---- through the module -----------------------------------------------------------------------------------------------------
def _stem_model(w):
    model = resnet18(norm_layer=nn.InstanceNorm2d)
    with torch.no_grad():
        model.conv1.weight.copy_(w)
    return model.to(DEV).train()


@pytest.mark.parametrize("name", [s[0] for s in sc.STEMS])
def test_native_stem_alone_against_fp64(name):
    """||dw - dw64|| / ||dw64|| of conv1's weight gradient, native stem on the GPU against the fp64 CPU stem, is at most
    MODEL_MARGIN x the same quantity of the plain fp32 CPU stem; and it is, bit for bit, the three ops calls composed."""
    x, w, c = sc.stem_inputs(name)
    g64 = sc.stem_weight_grad(x, w, c, torch.float64)
    yard = cc.rel_errors([sc.stem_weight_grad(x, w, c, torch.float32)], [g64])[0]
    model = _stem_model(w)
    assert simclr.use_native_stem(model) == 1
    xd, cd = x.to(DEV), c.to(DEV)
    out = simclr.stem_forward(model, xd)
    assert "StemNative" in nc.grad_fn_names(out)
    dw = torch.autograd.grad((out * cd).sum(), model.conv1.weight)[0]
    nat = cc.rel_errors([dw.cpu().numpy().astype(np.float64)], [g64])[0]
    print(f"{name}: native {nat:.3e} yardstick {yard:.3e} ratio {nat / yard:.3f}")
    assert np.linalg.norm(g64) > 0 and nat <= cc.MODEL_MARGIN * yard
    pooled, y, stats, win = ops.trunk32_stem_train(xd, model.conv1.weight.detach())
    assert torch.equal(out.detach().permute(0, 2, 3, 1), pooled)
    gy = ops.stem_pool_backward(cd.permute(0, 2, 3, 1).contiguous(), y, stats, win)
    assert torch.equal(dw, ops.conv_backward_weight(xd.permute(0, 2, 3, 1).contiguous(), gy, 7, 2, 3))
    # the functional form is the same Function
    out2 = simclr.native_stem(xd, model.conv1.weight)
    assert torch.equal(out2, out) and "StemNative" in nc.grad_fn_names(out2)


def test_resnet18_weight_gradients_with_the_native_stem_against_the_fp32_yardstick():
    seed = sc.MODEL_SEED
    assert sc.model_stem_margin(seed) >= sc.MARGIN
    g64 = cc.model_weight_grads(torch.float64, seed=seed)
    yard = cc.rel_errors(cc.model_weight_grads(torch.float32, seed=seed), g64)
    assert all(np.linalg.norm(g) > 0 for g in g64) and max(yard) < 1e-4
    nat = cc.rel_errors(sc.model_weight_grads_native(DEV, seed), g64)
    ratios = [a / b for a, b in zip(nat, yard)]
    for i, (a, b, r) in enumerate(zip(nat, yard, ratios)):
        print(f"conv {i:2d}: native {a:.3e} yardstick {b:.3e} ratio {r:.3f}")
    assert max(ratios) <= cc.MODEL_MARGIN


def test_ineligible_stems_take_the_torch_chain():
    x, w, _ = sc.stem_inputs("stem_32")
    xd = x.to(DEV)
    plain = _stem_model(w)
    simclr.use_native_stem(plain)
    assert "StemNative" in nc.grad_fn_names(simclr.stem_forward(plain, xd))
    bn = resnet18(norm_layer=nn.BatchNorm2d).to(DEV).train()
    simclr.use_native_stem(bn)
    torch_chain = lambda out: "StemNative" not in nc.grad_fn_names(out) and nc.grad_fn_names(out).startswith("MaxPool2D")
    assert torch_chain(simclr.stem_forward(bn, xd))
    assert torch_chain(simclr.stem_forward(plain, xd.clone().requires_grad_(True)))        # an input that requires grad
    assert torch_chain(simclr.stem_forward(plain.double(), xd.double()))                     # another dtype
    cpu = resnet18(norm_layer=nn.InstanceNorm2d).train()
    simclr.use_native_stem(cpu)
    assert torch_chain(simclr.stem_forward(cpu, x))                                          # a CPU tensor


def test_iclassifier_inference_is_untouched_by_the_swap():
    from dsmil_wsi_amd.synthetic import make_patches, make_resnet18_weights
    feats = []
    for swap in (False, True):
        res = resnet18(norm_layer=nn.InstanceNorm2d)
        res.fc = nn.Identity()
        res.load_state_dict({k: torch.as_tensor(np.asarray(v)) for k, v in make_resnet18_weights(11).items()}, strict=True)
        if swap:
            assert simclr.use_native_stem(res) == 1 and simclr.use_native_blocks(res) == 8
        torch.manual_seed(0)
        ic = dsmil.IClassifier(res, 512, output_class=2).eval().to(DEV)
        with torch.no_grad():
            f, c = ic(torch.from_numpy(make_patches(5, 2, 96, 96)).to(DEV))
        feats.append((f.clone(), c.clone()))
    assert torch.equal(feats[0][0], feats[1][0]) and torch.equal(feats[0][1], feats[1][1])
