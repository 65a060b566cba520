"""NT-Xent on the host: the closed form against the reference class's own fp64 values (tests/golden/ntxent_golden.npz,
written by tests/golden/make_ntxent_golden.py), the composite path of simclr.NTXentLoss, the derived bars of
tests/ntxent_cases.py against a numpy emulation of the kernels' arithmetic (two planes meet them, one plane misses them by
at least 8), the O(M D) workspace and the argument checks of the three entry points — none of it needs a device."""
import ctypes
import os

import numpy as np
import pytest
import torch

import dsmil  # noqa: F401
import dsmil_wsi_amd._native as nat
import ntxent_cases as nc
from dsmil_wsi_amd.simclr import NTXentLoss

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = np.load(os.path.join(ROOT, "tests", "golden", "ntxent_golden.npz"))
EMU_CASES = nc.CASES      # the emulation walks the whole table (the largest case takes about 3 s in numpy)


@pytest.mark.parametrize("case", nc.GOLDEN_CASES, ids=nc.case_name)
def test_closed_form_equals_the_reference_class(case):
    name = nc.case_name(case)
    zis, zjs = nc.make_inputs(case)
    assert np.array_equal(zis, GOLD[name + "/zis"]) and np.array_equal(zjs, GOLD[name + "/zjs"])
    loss, g_zis, g_zjs = nc.closed_form(zis, zjs, case[2], case[3])
    assert abs(loss - float(GOLD[name + "/loss"])) <= 1e-12 * max(abs(loss), 1e-300) or loss == GOLD[name + "/loss"]
    for got, key in ((g_zis, "/g_zis"), (g_zjs, "/g_zjs")):
        want = GOLD[name + key]
        assert np.max(np.abs(got - want)) <= 1e-12 * max(float(np.abs(want).max()), 1e-300) or not want.any()


@pytest.mark.parametrize("case", nc.GOLDEN_CASES, ids=nc.case_name)
def test_cpu_module_meets_the_golden_at_fp32_bars(case):
    """fp32 torch ops: a dot product of D terms, M exps and sums, no plane cut: 64 u relative to the largest magnitude of
    the output is a generous fp32 bar (u sqrt(D) LAM is about 64 u at D = 256)."""
    name = nc.case_name(case)
    zis = torch.tensor(GOLD[name + "/zis"], requires_grad=True)
    zjs = torch.tensor(GOLD[name + "/zjs"], requires_grad=True)
    crit = NTXentLoss(torch.device("cpu"), case[0], case[2], bool(case[3]))
    loss = crit(zis, zjs)
    loss.backward()
    want = float(GOLD[name + "/loss"])
    lim = 64 * nc.U
    assert abs(loss.item() - want) <= lim * max(abs(want), 1.0 / case[2])
    for got, key in ((zis.grad, "/g_zis"), (zjs.grad, "/g_zjs")):
        w = GOLD[name + key]
        row = np.abs(w).max(1, keepdims=True)
        if len(case) > 4:      # "spread": rows of very different scale, each against its own
            assert np.all(np.abs(got.numpy() - w) <= lim * 16 * row + 1e-30)
        else:
            assert np.max(np.abs(got.numpy() - w)) <= lim * max(float(np.abs(w).max()), 1e-30) or not w.any()


def test_cpu_module_fp64_and_short_batch():
    case = (17, 64, .5, 0)
    zis, zjs = nc.make_inputs(case)
    crit = NTXentLoss("cpu", 4096, .5, False)     # batch_size is not the batch: N comes from the input
    a = torch.tensor(zis, dtype=torch.float64, requires_grad=True)
    b = torch.tensor(zjs, dtype=torch.float64, requires_grad=True)
    loss = crit(a, b)
    loss.backward()
    ref = nc.closed_form(zis, zjs, .5, 0)
    assert abs(loss.item() - ref[0]) < 1e-12
    assert np.max(np.abs(a.grad.numpy() - ref[1])) < 1e-13 and np.max(np.abs(b.grad.numpy() - ref[2])) < 1e-13


@pytest.mark.parametrize("case", EMU_CASES, ids=nc.case_name)
def test_two_planes_meet_the_bars_and_one_plane_misses_them(case):
    zis, zjs = nc.make_inputs(case)
    ref = nc.reference(case)
    two = nc.ratios(nc.emulate(zis, zjs, case[2], case[3])[:3], ref)
    one = nc.ratios(nc.emulate(zis, zjs, case[2], case[3], planes=1)[:3], ref)
    print(nc.case_name(case), "two planes:", two, "one plane:", one)
    assert max(two) <= 1.0
    if case[0] == 1:       # the only column is the positive: loss and gradient are exactly 0 whatever the operand holds
        assert max(one) == 0.0 and max(two) == 0.0
    else:
        assert max(one) >= 8.0


def test_workspace_is_linear_in_the_batch():
    L = nat.lib()
    got = L.dsmil_ntxent_workspace_bytes(4096, 256)
    assert 0 < got <= nc.workspace_bound(4096, 256) < 8192 * 8192 * 4
    assert L.dsmil_ntxent_workspace_bytes(8, 100) > 0
    for n, d in ((0, 8), (8, 0), (65537, 8), (8, 4097)):
        assert L.dsmil_ntxent_workspace_bytes(n, d) == 0


def test_bad_arguments_are_rejected_without_a_device():
    L = nat.lib()
    buf = (ctypes.c_char * 4096)()
    base = ctypes.addressof(buf)
    p = ctypes.c_void_p((base + 255) // 256 * 256)        # never dereferenced: every call below returns before a launch
    big = 1 << 40
    fwd = lambda zis=p, zjs=p, n=4, d=8, t=.5, loss=p, lse=p, ws=p, nb=big: L.dsmil_ntxent_forward(  # noqa: E731
        zis, zjs, n, d, t, 1, loss, lse, ws, nb, None)
    bwd = lambda zis=p, zjs=p, n=4, d=8, t=.5, lse=p, g=p, gi=p, gj=p, ws=p, nb=big: L.dsmil_ntxent_backward(  # noqa: E731
        zis, zjs, n, d, t, 1, lse, g, gi, gj, ws, nb, None)
    for f in (fwd, bwd):
        assert f(zis=None) == nat.DSMIL_E_INVALID and f(zjs=None) == nat.DSMIL_E_INVALID and f(ws=None) == nat.DSMIL_E_INVALID
        assert f(n=0) == nat.DSMIL_E_INVALID and f(d=0) == nat.DSMIL_E_INVALID
        assert f(t=0.0) == nat.DSMIL_E_INVALID and f(t=-1.0) == nat.DSMIL_E_INVALID
        assert f(n=65537) == nat.DSMIL_E_UNSUPPORTED and f(d=4097) == nat.DSMIL_E_UNSUPPORTED
        assert f(nb=L.dsmil_ntxent_workspace_bytes(4, 8) - 1) == nat.DSMIL_E_WORKSPACE
    assert fwd(loss=None) == nat.DSMIL_E_INVALID and fwd(lse=None) == nat.DSMIL_E_INVALID
    assert bwd(lse=None) == nat.DSMIL_E_INVALID and bwd(g=None) == nat.DSMIL_E_INVALID
    assert bwd(gi=None) == nat.DSMIL_E_INVALID and bwd(gj=None) == nat.DSMIL_E_INVALID
