"""The native NT-Xent forward and backward (csrc/ntxent.hip) against the fp64 closed form at the bars DERIVED in
tests/ntxent_cases.py (no bar here is tuned on a GPU), and the behaviour of simclr.NTXentLoss around them."""
import numpy as np
import pytest
import torch

import dsmil  # noqa: F401
import ntxent_cases as nc
from dsmil_wsi_amd import ops
from dsmil_wsi_amd.simclr import NTXentLoss, ntxent_composite

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _run(zis, zjs, T, cosine, scale=1.0):
    a = torch.tensor(zis, device=DEV, requires_grad=True)
    b = torch.tensor(zjs, device=DEV, requires_grad=True)
    loss = NTXentLoss(DEV, zis.shape[0], T, bool(cosine))(a, b)
    (scale * loss).backward()
    return loss.item(), a.grad.cpu().numpy(), b.grad.cpu().numpy()


def _check(got, ref, what):
    r = nc.ratios(got, ref)
    print(what, "error / bar (loss, g_zis, g_zjs):", r)
    assert max(r) <= 1.0, (what, r)


@pytest.mark.parametrize("case", nc.CASES, ids=nc.case_name)
def test_forward_and_backward_meet_the_derived_bars(case):
    zis, zjs = nc.make_inputs(case)
    got = _run(zis, zjs, case[2], case[3])
    _check(got, nc.reference(case), nc.case_name(case))
    if case[0] == 1:       # the only column is the positive
        assert got[0] == 0.0 and not got[1].any() and not got[2].any()


@pytest.mark.parametrize("case", [(20, 48, .5, 1, "spread"), (24, 40, .5, 1, "twins")], ids=nc.case_name)
def test_unnormalised_rows_and_identical_samples(case):
    """Row norms over six decades in cosine mode; zis == zjs with two identical samples (S = 1 off the diagonal)."""
    zis, zjs = nc.make_inputs(case)
    _check(_run(zis, zjs, case[2], case[3]), nc.reference(case), nc.case_name(case))


def test_upstream_gradient_is_read_on_the_device():
    case = (33, 256, .5, 1)
    zis, zjs = nc.make_inputs(case)
    got = _run(zis, zjs, case[2], case[3], scale=3.0)
    _check(got, nc.reference(case, 3.0), "3 * loss")


def test_other_dtypes_and_layouts_take_the_composite_path():
    case = (17, 64, .5, 0)
    zis, zjs = nc.make_inputs(case)
    ref = nc.closed_form(zis, zjs, case[2], case[3])
    crit = NTXentLoss(DEV, 17, case[2], False)
    a = torch.tensor(zis, device=DEV, dtype=torch.float64, requires_grad=True)
    b = torch.tensor(zjs, device=DEV, dtype=torch.float64, requires_grad=True)
    loss = crit(a, b)
    assert loss.dtype == torch.float64 and loss.grad_fn is not None and "NTXentNative" not in type(loss.grad_fn).__name__
    loss.backward()
    assert abs(loss.item() - ref[0]) < 1e-12 and np.max(np.abs(a.grad.cpu().numpy() - ref[1])) < 1e-13
    # a non-contiguous fp32 view: same values as the native path within the bars
    wide = torch.zeros((17, 128), device=DEV)
    wide[:, ::2] = torch.tensor(zis, device=DEV)
    av = wide[:, ::2].detach().requires_grad_(True)
    bv = torch.tensor(zjs, device=DEV, requires_grad=True)
    assert not av.is_contiguous()
    loss = crit(av, bv)
    assert "NTXentNative" not in type(loss.grad_fn).__name__
    loss.backward()
    refb = nc.reference(case)
    assert abs(loss.item() - refb[0]) <= 64 * nc.U * max(abs(refb[0]), 1 / case[2])
    assert np.max(np.abs(av.grad.cpu().numpy() - refb[1])) <= 64 * nc.U * np.abs(refb[1]).max()


def test_non_default_stream_and_bit_identical_calls():
    case = (300, 128, .5, 1)
    zis, zjs = nc.make_inputs(case)
    a, b = torch.tensor(zis, device=DEV), torch.tensor(zjs, device=DEV)
    one = torch.ones((), device=DEV)
    loss0, lse0 = ops.ntxent_forward(a, b, case[2], True)
    g0 = ops.ntxent_backward(a, b, case[2], lse0, one, True)
    torch.cuda.synchronize()
    s = torch.cuda.Stream(device=DEV)
    with torch.cuda.stream(s):
        loss1, lse1 = ops.ntxent_forward(a, b, case[2], True)
        g1 = ops.ntxent_backward(a, b, case[2], lse1, one, True)
    s.synchronize()
    assert torch.equal(loss0, loss1) and torch.equal(lse0, lse1) and torch.equal(g0[0], g1[0]) and torch.equal(g0[1], g1[1])
    _check((loss1.item(), g1[0].cpu().numpy(), g1[1].cpu().numpy()), nc.reference(case), "side stream")


def test_backward_does_not_depend_on_the_forward_workspace():
    case = (65, 100, .1, 1)
    zis, zjs = nc.make_inputs(case)
    a, b = torch.tensor(zis, device=DEV), torch.tensor(zjs, device=DEV)
    loss, lse = ops.ntxent_forward(a, b, case[2], True)
    lse = lse.clone()
    ops._workspace(torch.device(DEV), 1).fill_(255)      # the cached buffer of this stream: every fp32 and fp16 in it a NaN
    g = ops.ntxent_backward(a, b, case[2], lse, torch.ones((), device=DEV), True)
    _check((loss.item(), g[0].cpu().numpy(), g[1].cpu().numpy()), nc.reference(case), "NaN workspace")


def test_inside_a_training_step():
    """NTXentLoss behind F.normalize(Linear(x)): the parameter gradients of the native path against the composite path in
    fp64, at the bars carried through the (linear) chain: |dW| <= sum_rows bar_g |d row / d W|."""
    torch.manual_seed(5)
    N, Din, D, T = 48, 32, 64, .5
    lin = torch.nn.Linear(Din, D).to(DEV)
    xi, xj = torch.randn(N, Din, device=DEV), torch.randn(N, Din, device=DEV)
    xj = 0.9 * xi + 0.44 * xj
    zi = torch.nn.functional.normalize(lin(xi), dim=1)
    zj = torch.nn.functional.normalize(lin(xj), dim=1)
    zi.retain_grad(); zj.retain_grad()
    loss = NTXentLoss(DEV, N, T, True)(zi.contiguous(), zj.contiguous())
    assert "NTXentNative" in type(loss.grad_fn).__name__
    loss.backward()
    ref = nc.reference_of(zi.detach().cpu().numpy(), zj.detach().cpu().numpy(), T, 1)
    _check((loss.item(), zi.grad.cpu().numpy(), zj.grad.cpu().numpy()), ref, "training step, projections")
    # the same step in fp64 on the composite path
    lin64 = torch.nn.Linear(Din, D).to(DEV).double()
    lin64.load_state_dict({k: v.double() for k, v in lin.state_dict().items()})
    zi64 = torch.nn.functional.normalize(lin64(xi.double()), dim=1)
    zj64 = torch.nn.functional.normalize(lin64(xj.double()), dim=1)
    ntxent_composite(zi64, zj64, T, True).backward()
    gw, gw64 = lin.weight.grad.double(), lin64.weight.grad
    # the chain behind the loss runs in fp32 torch ops on one side: 64 u of the gradient's scale on top of the carried bars
    jac = torch.tensor(np.concatenate([ref[4], ref[5]], 0), device=DEV)           # bars of (g_zis, g_zjs)
    xin = torch.cat([xi, xj], 0).double().abs()
    pre = torch.cat([lin64(xi.double()), lin64(xj.double())], 0)
    zn = pre.norm(dim=1, keepdim=True)
    zh = (pre / zn).abs()
    carried = (((jac + zh * (zh * jac).sum(1, keepdim=True)) / zn).t() @ xin)      # through d normalize = (I - z z^T) / |row|
    assert torch.all((gw - gw64).abs() <= carried + 64 * nc.U * gw64.abs().max())
