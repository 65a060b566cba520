"""The InstanceNorm / ReLU / residual-add backward kernels (csrc/norm_bwd.hip) through ops.norm_backward against fp64 at the
derived bars of tests/norm_bwd_cases.py (tests/test_norm_bwd_host.py shows the stated arithmetic reaches them and that they see
the mutants): every element is compared; the exact cases bit for bit; the exact zeros of HW = 1, of a fully masked channel and
of g = 0; two calls bit-identical, also over a workspace full of NaN and on another stream.  Then through
simclr.NativeBasicBlock against the fp64 CPU block, through a whole ResNet-18 and through one SimCLR step, each held to the fp32
CPU yardstick with conv_bwd_cases.MODEL_MARGIN."""
import numpy as np
import pytest
import torch
import torch.nn as nn

import conv_bwd_cases as cc
import norm_bwd_cases as nc
import dsmil
from dsmil_wsi_amd import ops, simclr
from dsmil_wsi_amd.resnet import resnet18

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)           # a copy: the cached cases are read-only


def _nan_ws(kind, B, HW, C):
    need = ops._native.lib().dsmil_norm_bwd_workspace_bytes(ops.NORM_BWD_KINDS[kind], B, HW, C)
    return torch.full(((need + 3) // 4,), float("nan"), dtype=torch.float32, device=DEV).view(torch.uint8)


def _run(kind, inp, ws=None):
    """ops.norm_backward on the device copies of a case's inputs -> a dict of device tensors like closed_form's."""
    d = {k: _dev(v) for k, v in inp.items()}
    kw = {}
    if kind != "relu":
        kw["out"] = d["out"]
    if kind == "add_down":
        kw["down"] = (d["yd"], (d["md"], d["rd"]))
    res = ops.norm_backward(kind, d["g"], d["y"], (d["m"], d["r"]), ws=ws, **kw)
    return {"gy": res} if kind == "relu" else dict(zip(("gy", "gres" if kind == "add" else "gyd"), res))


def _host(res):
    return {k: v.cpu().numpy() for k, v in res.items()}


@pytest.mark.parametrize("name", [c[0] for c in nc.CASES])
def test_stage_against_fp64(name):
    _, kind, B, HW, C, _ = nc.BY_NAME[name]
    p = ops.norm_backward_plan(kind, B, HW, C)
    assert (p["chunk"], p["n_partials"], p["run_len"], p["lanes"]) == nc.PLANS[name][:4]
    inp = nc.case(name)
    res = _run(kind, inp)
    got = _host(res)
    wst = nc.worst_ratio(got, nc.expected(name))
    print(f"{name}: worst err / bar {wst:.4f}")
    assert wst <= 1
    if HW == 1:                                                    # x^ and q - mean q are exact zeros
        assert not got["gy"].any() and not got.get("gyd", np.zeros(1)).any()
    else:                                                          # the fully masked channel of image 0
        assert got["gy"].any() and not got["gy"][0, :, nc.MASKED_CH].any()
        assert not got.get("gyd", np.zeros((1, 1, C)))[0, :, nc.MASKED_CH].any()
    res2 = _run(kind, inp, ws=_nan_ws(kind, B, HW, C))             # no atomics, nothing read from a stale workspace
    assert all(torch.equal(res[k], res2[k]) for k in res)


@pytest.mark.parametrize("name", [c[0] for c in nc.EXACT_CASES])
def test_exact_cases_bit_for_bit(name):
    inp, ref = nc.exact_case(name)
    got = _host(_run(nc.BY_NAME[name][1], inp))
    for k in ref:
        a = got[k].astype(np.float64)
        assert np.array_equal(a, ref[k]), f"{name} {k}: {np.count_nonzero(a != ref[k])} of {a.size} differ, max {np.abs(a - ref[k]).max():.3e}"


@pytest.mark.parametrize("name", ["r_35", "a_257", "d_257", "d_2048"])
def test_all_zero_gradient_gives_exact_zeros(name):
    inp = dict(nc.case(name))
    inp["g"] = np.zeros_like(inp["g"])
    got = _host(_run(nc.BY_NAME[name][1], inp))
    assert all(not v.any() for v in got.values())


@pytest.mark.parametrize("name", ["r_700", "a_257", "d_257"])
def test_calls_are_bit_identical_on_another_stream(name):
    kind = nc.BY_NAME[name][1]
    first = _run(kind, nc.case(name))
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        second = _run(kind, nc.case(name))
    side.synchronize()
    assert all(torch.equal(first[k], second[k]) for k in first)


def test_refused_shapes_raise_before_any_launch():
    g = torch.zeros(2, 35, 40, device=DEV)
    st = (torch.zeros(2, 40, device=DEV), torch.ones(2, 40, device=DEV))
    with pytest.raises(NotImplementedError):
        ops.norm_backward("relu", g, g.clone(), st)
    with pytest.raises(ValueError):
        ops.norm_backward("add", g, g.clone(), st)                 # "add" without out


# ---- through the block ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [b[0] for b in nc.BLOCKS])
@pytest.mark.parametrize("channels_last", [True, False])
def test_native_basic_block_against_fp64(name, channels_last):
    """||g - g64|| / ||g64|| of the input gradient and of every weight gradient, native block on the GPU against the fp64 CPU
    block, is at most MODEL_MARGIN x the same quantity of the plain fp32 CPU block."""
    g64, yard = nc.block_yardstick(name)
    wrap = nn.Sequential(nc.make_block(name))
    assert simclr.use_native_blocks(wrap) == 1
    blk = wrap[0].to(DEV)
    x, c = nc.block_inputs(name)
    x, c = x.to(DEV), c.to(DEV)
    if channels_last:
        x = x.contiguous(memory_format=torch.channels_last)
    got, fn = nc.block_grads(blk, x, c)
    assert "BasicBlockNative" in fn                                # the Function ran
    nat = nc.rel_errors(got, g64)
    ratios = [a / b for a, b in zip(nat, yard)]
    for what, a, b, r in zip(["x", "conv1", "conv2", "downsample"], nat, yard, ratios):
        print(f"{name} channels_last={channels_last} {what}: native {a:.3e} yardstick {b:.3e} ratio {r:.3f}")
    assert max(ratios) <= cc.MODEL_MARGIN


def test_ineligible_blocks_take_basic_block_forward():
    x, c = nc.block_inputs("id_64")
    x, c = x.to(DEV), c.to(DEV)
    bn = simclr.NativeBasicBlock(64, 64, norm_layer=nn.BatchNorm2d).to(DEV)
    biased = simclr.NativeBasicBlock(64, 64, norm_layer=nn.InstanceNorm2d)
    biased.conv2 = nn.Conv2d(64, 64, 3, 1, 1, bias=True)
    for blk in (bn, biased.to(DEV)):
        names = nc.grad_fn_names(blk(x.clone().requires_grad_(True)))
        assert "BasicBlockNative" not in names and names.startswith("Relu")
    plain = simclr.NativeBasicBlock(64, 64, norm_layer=nn.InstanceNorm2d).to(DEV)
    assert "BasicBlockNative" in nc.grad_fn_names(plain(x))
    assert "BasicBlockNative" not in nc.grad_fn_names(plain.double()(x.double()))         # another dtype


# ---- through the model ------------------------------------------------------------------------------------------------------
def test_resnet18_weight_gradients_against_the_fp32_yardstick():
    g64 = cc.model_weight_grads(torch.float64)
    yard = cc.rel_errors(cc.model_weight_grads(torch.float32), g64)
    assert all(np.linalg.norm(g) > 0 for g in g64) and max(yard) < 1e-4
    nat = cc.rel_errors(nc.model_weight_grads_native(DEV), g64)
    ratios = [a / b for a, b in zip(nat, yard)]
    for i, (a, b, r) in enumerate(zip(nat, yard, ratios)):
        print(f"conv {i:2d}: native {a:.3e} yardstick {b:.3e} ratio {r:.3f}")
    assert max(ratios) <= cc.MODEL_MARGIN


def test_one_simclr_step_against_fp64():
    """Loss within the forward's own tolerance (1e-4 absolute + 1e-4 relative, tests/test_resnet_gpu.py) of the fp64 CPU model;
    the 20 conv and 4 head gradients at the model-level criterion."""
    l64, g64, yard = nc.simclr_yardstick()
    assert all(np.linalg.norm(g) > 0 for g in g64)
    loss, got = nc.simclr_step(torch.float32, device=DEV, native=True)
    print(f"loss native {loss:.7f} fp64 {l64:.7f}")
    assert abs(loss - l64) <= 1e-4 + 1e-4 * abs(l64)
    nat = cc.rel_errors(got, g64)
    ratios = [a / b for a, b in zip(nat, yard)]
    for i, (a, b, r) in enumerate(zip(nat, yard, ratios)):
        print(f"param {i:2d}: native {a:.3e} yardstick {b:.3e} ratio {r:.3f}")
    assert max(ratios) <= cc.MODEL_MARGIN


def test_iclassifier_inference_is_untouched_by_the_swap():
    from dsmil_wsi_amd.synthetic import make_patches, make_resnet18_weights
    feats = []
    for swap in (False, True):
        res = resnet18(norm_layer=nn.InstanceNorm2d)
        res.fc = nn.Identity()
        res.load_state_dict({k: torch.as_tensor(np.asarray(v)) for k, v in make_resnet18_weights(11).items()}, strict=True)
        if swap:
            assert simclr.use_native_blocks(res) == 8 and simclr.use_native_convs(res) == 20
        torch.manual_seed(0)
        ic = dsmil.IClassifier(res, 512, output_class=2).eval().to(DEV)
        with torch.no_grad():
            f, c = ic(torch.from_numpy(make_patches(5, 2, 96, 96)).to(DEV))
        feats.append((f.clone(), c.clone()))
    assert torch.equal(feats[0][0], feats[1][0]) and torch.equal(feats[0][1], feats[1][1])
