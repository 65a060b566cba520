"""The bars of tests/norm_bwd_cases.py are reachable and sharp, without a device: a numpy emulation of the stated arithmetic (fp32
element operations, serial runs, a fixed tree, partials in chunk order) meets every bar on every case and is bit-exact on the
EXACT cases; the mutants — the x^ mean(q x^) term dropped, mean q dropped, the leading rstd dropped, the mask taken from g's
sign, "add_down" normalising yd with y's statistics — are not.  The closed form is the fp64 autograd gradient.  And the module
layer: NativeBasicBlock on CPU tensors is BasicBlock, use_native_blocks swaps what it should and keeps the state dict.  CPU only."""
import numpy as np
import pytest
import torch
import torch.nn as nn

import norm_bwd_cases as nc
import dsmil  # noqa: F401  (registers the dsmil_wsi_amd package)
from dsmil_wsi_amd import modules, simclr
from dsmil_wsi_amd.resnet import BasicBlock, resnet18, resnet18_in_convs, resnet34, resnet50


@pytest.mark.parametrize("kind", nc.KINDS)
def test_the_closed_form_is_the_fp64_autograd_gradient(kind):
    err = nc.autograd_check(kind)
    print(f"{kind}: closed form against fp64 autograd {err:.3e}")
    assert err <= 1e-13


@pytest.mark.parametrize("name", [c[0] for c in nc.CASES])
def test_the_emulation_meets_the_bar(name):
    kind, HW = nc.BY_NAME[name][1], nc.BY_NAME[name][3]
    assert nc.PLANS[name][:4] == nc.plan_of(*nc.BY_NAME[name][1:5])           # the emulation's order is the pinned plan's
    got = nc.emulate(kind, nc.case(name), chunk=nc.PLANS[name][0])
    wst = nc.worst_ratio(got, nc.expected(name))
    print(f"{name}: worst err / bar {wst:.4f}")
    assert wst <= 1
    if HW == 1:
        assert not got["gy"].any() and not got.get("gyd", np.zeros(1)).any()
    else:
        assert got["gy"].any() and not got["gy"][0, :, nc.MASKED_CH].any()     # the fully masked channel: exact zeros


@pytest.mark.parametrize("name", [c[0] for c in nc.EXACT_CASES])
def test_the_emulation_is_exact_on_the_exact_cases(name):
    inp, ref = nc.exact_case(name)
    got = nc.emulate(nc.BY_NAME[name][1], inp)
    assert all(np.array_equal(got[k].astype(np.float64), ref[k]) for k in ref)
    assert all(np.any(ref[k] != 0) for k in ref)


@pytest.mark.parametrize("mutant", nc.MUTANTS)
def test_the_bars_see_the_mutants(mutant):
    """Each mutant misses the bar on every case of its kind with more than one pixel, at either magnitude of g."""
    seen = 0
    for name, kind, B, HW, C, mag in nc.CASES:
        if HW == 1 or (mutant == "down_uses_main_stats" and kind != "add_down"):
            continue
        wst = nc.worst_ratio(nc.emulate(kind, nc.case(name), mutant=mutant), nc.expected(name))
        assert wst > 1, (name, wst)
        seen += 1
    assert seen >= 4


def test_all_zero_gradient_gives_exact_zeros():
    for name in ("r_35", "a_257", "d_257"):
        inp = dict(nc.case(name), g=np.zeros_like(nc.case(name)["g"]))
        got = nc.emulate(nc.BY_NAME[name][1], inp)
        assert all(not v.any() for v in got.values())


# ---- the module layer on the CPU --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [b[0] for b in nc.BLOCKS])
def test_native_basic_block_on_cpu_is_basic_block(name):
    ref = nc.make_block(name)
    nat = nn.Sequential(nc.make_block(name))
    assert simclr.use_native_blocks(nat) == 1 and isinstance(nat[0], simclr.NativeBasicBlock)
    x, c = nc.block_inputs(name)
    outs = []
    for blk in (ref, nat[0]):
        xt = x.clone().requires_grad_(True)
        out = blk(xt)
        assert "BasicBlockNative" not in nc.grad_fn_names(out)
        (out * c).sum().backward()
        outs.append([out.detach(), xt.grad] + [p.grad for p in blk.parameters()])
    assert len(outs[0]) == len(outs[1]) and all(torch.equal(a, b) for a, b in zip(*outs))


def _resnet(f=resnet18, norm=nn.InstanceNorm2d):
    m = f(norm_layer=norm)
    m.fc = nn.Identity()
    return m


def test_use_native_blocks_counts():
    assert simclr.use_native_blocks(_resnet(resnet18)) == 8
    assert simclr.use_native_blocks(_resnet(resnet34)) == 16
    assert simclr.use_native_blocks(_resnet(resnet18, nn.BatchNorm2d)) == 0
    assert simclr.use_native_blocks(_resnet(resnet50)) == 0
    # ineligible blocks stay: affine InstanceNorm, a biased conv, widths the kernels do not take
    affine = BasicBlock(64, 64, norm_layer=lambda c: nn.InstanceNorm2d(c, affine=True))
    assert simclr.use_native_blocks(nn.Sequential(affine, nc.make_block("id_64", bias=True), BasicBlock(24, 24, norm_layer=nn.InstanceNorm2d),
                                                  BasicBlock(32, 32, norm_layer=nn.InstanceNorm2d))) == 0


def test_use_native_blocks_keeps_the_state_dict_and_the_parameters():
    m = _resnet()
    before = {k: v.clone() for k, v in m.state_dict().items()}
    params = {n: p for n, p in m.named_parameters()}
    names = [n for n, _ in m.named_modules()]
    assert simclr.use_native_blocks(m) == 8
    after = m.state_dict()
    assert list(after) == list(before) and all(torch.equal(after[k], before[k]) for k in before)
    assert all(p is params[n] for n, p in m.named_parameters()) and len(list(m.named_parameters())) == len(params)
    assert [n for n, _ in m.named_modules()] == names
    assert sum(isinstance(c, simclr.NativeBasicBlock) for c in m.modules()) == 8
    assert simclr.use_native_blocks(m) == 0                                            # nothing left to swap
    assert m.layer1[0].downsample is None and m.layer2[0].stride == 2 and m.layer1[0].training == m.training
    # it composes with use_native_convs in either order
    assert simclr.use_native_convs(m) == 20
    m2 = _resnet()
    assert simclr.use_native_convs(m2) == 20 and simclr.use_native_blocks(m2) == 8
    assert list(m2.state_dict()) == list(before)


def test_a_swapped_resnet_still_answers_resnet18_in_convs():
    m = _resnet()
    plain = resnet18_in_convs(m)
    simclr.use_native_blocks(m)
    got = resnet18_in_convs(m)
    assert plain is not None and got is not None and len(got) == 20 and all(a is b for a, b in zip(got, plain))
    got = modules.resnet_convs_of(m)
    assert got is not None and len(got[0]) == 20 and got[1] is None
    x = torch.rand(1, 3, 64, 64)
    ref = _resnet()
    ref.load_state_dict(m.state_dict())
    with torch.no_grad():
        assert torch.equal(m(x), ref(x))


def test_the_block_checks_have_clean_yardsticks():
    """The fp32 CPU blocks of the block-level check agree with fp64 to fp32's own class: no ReLU decision flips between the
    two, so the yardstick measures rounding."""
    for name, *_ in nc.BLOCKS:
        g64, yard = nc.block_yardstick(name)
        print(name, " ".join(f"{v:.2e}" for v in yard))
        assert all(np.linalg.norm(g) > 0 for g in g64) and max(yard) < 1e-5
