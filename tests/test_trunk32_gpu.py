"""The kernels of the fp32-class embedder trunk (csrc/resnet_fwd.hip, csrc/wino_w1.h), ONE AT A TIME through the dsmil_trunk32_*
entries, against fp64 at the derived bars of tests/trunk32_cases.py (tests/test_trunk32_host.py shows the reference arithmetic
reaches them and that they see the mutants); the exact cases bit for bit; and dsmil_resnet_forward equal, bit for bit, to the
chain of its stages.  Every case first asserts — through dsmil_trunk32_conv_plan — that it reaches the launch condition it is
named for."""
import numpy as np
import pytest
import torch

import trunk32_cases as tc
from trunk32_cases import PRECISIONS
from dsmil_wsi_amd import ops

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _nhwc(a):
    return _dev(np.asarray(a).transpose(0, 2, 3, 1))


def _nchw64(t):
    return t.cpu().numpy().transpose(0, 3, 1, 2).astype(np.float64)


def _assert_plan(name, precision):
    c = tc.BY_NAME[name]
    if len(c) == 7:
        _, B, H, W, Cin, Cout, norm = c
        p = ops.trunk32_conv_plan(Cin, Cout, 3, 1, 1, B, H, W, norm, precision)
        assert (p["kernel"], p["IB"], p["TYB"], p["TXB"], p["nby"], p["nbx"], p["grid_x"], p["grid_y"]) == tc.WINO_PLANS[name], (name, p)
    else:
        _, B, H, W, Cin, Cout, ks, stride, pad, norm = c
        p = ops.trunk32_conv_plan(Cin, Cout, ks, stride, pad, B, H, W, norm, precision)
        assert p["kernel"] == "s6" and (p["tile"], p["Ho"], p["Wo"], p["nslots"], p["grid_x"], p["grid_y"]) == tc.DIRECT_PLANS[name], (name, p)
    assert p["products"] == (3 if precision == "fp32" else 1)


def _run_conv(x, w, st, stride, pad, precision, frozen=None):
    ist = tuple(_dev(t) for t in st) if st is not None else None
    fz = tuple(_dev(t) for t in frozen) if frozen is not None else None
    return ops.trunk32_conv(_nhwc(x), _dev(w), stride, pad, in_stats=ist, frozen=fz, precision=precision)


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("name", [c[0] for c in tc.DIRECT_CASES + tc.WINO_CASES])
def test_conv_kernel_against_fp64(name, precision):
    _assert_plan(name, precision)
    x, w, st, stride, pad, _ = tc.conv_case(name)
    s, bar, (m, r, dm, dr) = tc.conv_expected(name, precision)
    y, mean, rstd = _run_conv(x, w, st, stride, pad, precision)
    got, gm, gr = _nchw64(y), mean.cpu().numpy().astype(np.float64), rstd.cpu().numpy().astype(np.float64)
    assert got.shape == s.shape
    err = np.abs(got - s)
    wy, wm, wr = tc.worst(err, bar), tc.worst(np.abs(gm - m), dm), tc.worst(np.abs(gr - r), dr)
    print(f"{name} {precision}: max err {err.max():.3e} worst err / bar {wy:.3f}; mean {np.abs(gm - m).max():.3e} {wm:.3f}; "
          f"rstd {np.abs(gr - r).max():.3e} {wr:.3f}")
    assert wy <= 1 and wm <= 1 and wr <= 1
    assert np.all(got[:, tc.ZERO_CH] == 0) and np.all(gm[:, tc.ZERO_CH] == 0)
    assert np.all(np.abs(gr[:, tc.ZERO_CH] - tc.RSTD0) <= 8 * tc.U32 * tc.RSTD0)
    y2, mean2, rstd2 = _run_conv(x, w, st, stride, pad, precision)                    # no atomics: two runs are one result
    assert torch.equal(y, y2) and torch.equal(mean, mean2) and torch.equal(rstd, rstd2)


@pytest.mark.parametrize("name", ["d42_1x1_9x7", "d22_s2_7x5", "u_5x7", "w_5x7"])
def test_conv_with_frozen_statistics(name):
    x, w, st, stride, pad, _ = tc.conv_case(name)
    Cout = w.shape[0]
    rng = np.random.default_rng(7)
    fm, fr = rng.standard_normal(Cout).astype(np.float32), (rng.uniform(0.5, 2, Cout) * rng.choice([-1, 1], Cout)).astype(np.float32)
    y, mean, rstd = _run_conv(x, w, st, stride, pad, "fp32", frozen=(fm, fr))
    y0, _, _ = _run_conv(x, w, st, stride, pad, "fp32")
    B = x.shape[0]
    assert torch.equal(y, y0)
    assert np.array_equal(mean.cpu().numpy(), np.tile(fm, (B, 1))) and np.array_equal(rstd.cpu().numpy(), np.tile(fr, (B, 1)))


@pytest.mark.parametrize("name", [c[0] for c in tc.EXACT_CASES])
def test_conv_exact_cases_bit_for_bit(name):
    x, w, stride, pad, wino, s = tc.exact_case(name)
    _, B, H, W, Cin, Cout, ks, _, _, flav = tc.BY_NAME[name]
    p = ops.trunk32_conv_plan(Cin, Cout, ks, stride, pad, B, H, W, False, "fp32")
    want = {"x42": ("s6", 42), "x22": ("s6", 22), "x24": ("s6", 24), "xu": ("unit", 0), "xw": ("w1", 0)}[name.split("_")[0]]
    assert (p["kernel"], p["tile"]) == want
    for precision in (("fp32", "half") if flav == "plain" else ("fp32",)):
        y, _, _ = _run_conv(x, w, None, stride, pad, precision)
        got = _nchw64(y)
        bad = int((got != s).sum())
        print(f"{name} {precision}: {bad} of {s.size} elements differ, max |diff| {np.abs(got - s).max():.3e}")
        assert bad == 0


# ---- stem ---------------------------------------------------------------------------------------------------------------------
def _run_stem(x, w, fz, precision):
    return ops.trunk32_stem(_dev(x), _dev(w), frozen=tuple(_dev(t) for t in fz) if fz else None, precision=precision)


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("name", [c[0] for c in tc.STEM_CASES])
def test_stem_against_fp64(name, precision):
    x, w, fz = tc.stem_case(name)
    ref, bar, m, r, dm, dr = tc.stem_expected(name, precision)
    pooled, mean, rstd = _run_stem(x, w, fz, precision)
    got, gm, gr = _nchw64(pooled), mean.cpu().numpy().astype(np.float64), rstd.cpu().numpy().astype(np.float64)
    assert got.shape == ref.shape
    err = np.abs(got - ref)
    wp = tc.worst(err, bar)
    if fz:
        assert np.array_equal(gm, m) and np.array_equal(gr, r)
        wm = wr = 0.0
    else:
        wm, wr = tc.worst(np.abs(gm - m), dm), tc.worst(np.abs(gr - r), dr)
        assert np.all(gm[:, tc.ZERO_CH] == 0) and np.all(got[:, tc.ZERO_CH] == 0)
    print(f"{name} {precision}: max err {err.max():.3e} worst err / bar {wp:.3f}; mean {wm:.3f}; rstd {wr:.3f}")
    assert wp <= 1 and wm <= 1 and wr <= 1
    again = _run_stem(x, w, fz, precision)
    assert all(torch.equal(a, b) for a, b in zip((pooled, mean, rstd), again))


@pytest.mark.parametrize("name", [c[0] for c in tc.STEM_EXACT])
def test_stem_exact_cases_bit_for_bit(name):
    """The raw conv is not an output of the stem entry; with frozen statistics m = 0, r = 1 the pooled map is relu(max of
    the window) of the raw conv values, exactly."""
    x, w, s = tc.stem_exact_case(name)
    fz = (np.zeros(64, np.float32), np.ones(64, np.float32))
    pooled, _, _ = _run_stem(x, w, fz, "fp32")
    want = np.maximum(tc.maxpool64(s), 0)
    got = _nchw64(pooled)
    bad = int((got != want).sum())
    print(f"{name}: {bad} of {want.size} elements differ, max |diff| {np.abs(got - want).max():.3e}")
    assert bad == 0
    neg = (np.zeros(64, np.float32), -np.ones(64, np.float32))                        # r = -1: relu(-(window minimum))
    pooled, _, _ = _run_stem(x, w, neg, "fp32")
    assert np.array_equal(_nchw64(pooled), np.maximum(-tc.maxpool64(s, negate=np.ones(64, bool)), 0))


# ---- tail ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [c[0] for c in tc.TAIL_CASES])
def test_tail_against_fp64(name):
    y2, st, idn, dst = tc.tail_case(name)
    kind = tc.BY_NAME[name][1]
    ref, bar = tc.tail_reference(kind, y2, st, idn, dst)
    args = (kind, _dev(y2), tuple(_dev(t) for t in st), _dev(idn), tuple(_dev(t) for t in dst) if dst else None)
    out = ops.trunk32_tail(*args)
    err = np.abs(out.cpu().numpy().astype(np.float64) - ref)
    w = tc.worst(err, bar)
    print(f"{name}: max err {err.max():.3e} worst err / bar {w:.3f}")
    assert out.shape == ref.shape and w <= 1
    assert torch.equal(out, ops.trunk32_tail(*args))


# ---- wiring: dsmil_resnet_forward == the chain of its stages --------------------------------------------------------------------
def _chain(x, convs, depth, frozen=None):
    """stem -> per block conv / conv [/ conv] [/ downsample] -> tail ... -> pool, from the stage entries, as resnet_forward_impl
    walks make_arch.  frozen: (m, r) per conv in state_dict order, or None."""
    fz = (lambda i: frozen[i]) if frozen is not None else (lambda i: None)
    cur, _, _ = ops.trunk32_stem(x, convs[0], frozen=fz(0))
    nblk = {18: (2, 2, 2, 2), 34: (3, 4, 6, 3), 50: (3, 4, 6, 3)}[depth]
    ci = 1
    for l, n in enumerate(nblk):
        for b in range(n):
            last = l == 3 and b == n - 1
            if depth >= 50:
                down, stride = b == 0, 2 if (l > 0 and b == 0) else 1
                y1, m1, r1 = ops.trunk32_conv(cur, convs[ci], 1, 0, frozen=fz(ci))
                y2, m2, r2 = ops.trunk32_conv(y1, convs[ci + 1], stride, 1, in_stats=(m1, r1), frozen=fz(ci + 1))
                yo, mo, ro = ops.trunk32_conv(y2, convs[ci + 2], 1, 0, in_stats=(m2, r2), frozen=fz(ci + 2))
                if down:
                    yd, md, rd = ops.trunk32_conv(cur, convs[ci + 3], stride, 0, frozen=fz(ci + 3))
                ci += 4 if down else 3
            else:
                down = l > 0 and b == 0
                y1, m1, r1 = ops.trunk32_conv(cur, convs[ci], 2 if down else 1, 1, frozen=fz(ci))
                yo, mo, ro = ops.trunk32_conv(y1, convs[ci + 1], 1, 1, in_stats=(m1, r1), frozen=fz(ci + 1))
                if down:
                    yd, md, rd = ops.trunk32_conv(cur, convs[ci + 2], 2, 0, frozen=fz(ci + 2))
                ci += 3 if down else 2
            if last:
                return ops.trunk32_tail("pool", yo, (mo, ro), cur)
            cur = ops.trunk32_tail("down", yo, (mo, ro), yd, (md, rd)) if down else ops.trunk32_tail("identity", yo, (mo, ro), cur)


@pytest.mark.parametrize("u8", [True, False])
@pytest.mark.parametrize("depth", [18, 34, 50])
def test_forward_equals_the_chain_of_its_stages(depth, u8):
    x, ws = tc.wiring_inputs(depth)
    xd = _dev(x) if u8 else _dev((x.astype(np.float32) / np.float32(255)).transpose(0, 3, 1, 2))
    convs = [_dev(w) for w in ws]
    feats, _ = ops.resnet18in_forward(xd, convs)
    chain = _chain(xd, convs, depth)
    assert feats.shape == chain.shape and bool(torch.isfinite(feats).all())
    assert torch.equal(feats, chain), f"max |diff| {(feats - chain).abs().max().item():.3e}"


def test_frozen_batchnorm_forward_equals_the_chain_of_its_stages():
    x, ws = tc.wiring_inputs(18)
    xd, convs = _dev(x), [_dev(w) for w in ws]
    g = torch.Generator().manual_seed(5)
    norms = []
    for w in ws:
        bn = torch.nn.BatchNorm2d(w.shape[0]).eval()
        with torch.no_grad():
            bn.weight.copy_(torch.randn(w.shape[0], generator=g) * 0.5 + 1.0)       # some scales negative
            bn.bias.copy_(torch.randn(w.shape[0], generator=g) * 0.1)
            bn.running_mean.copy_(torch.randn(w.shape[0], generator=g) * 0.1)
            bn.running_var.copy_(torch.rand(w.shape[0], generator=g) * 0.5 + 0.05)
        norms.append(bn.to(DEV))
    feats, _ = ops.resnet18in_forward(xd, convs, bn_norms=norms)
    bn_m, bn_r = ops._folded_bn(norms, xd.device)
    assert bool((bn_r < 0).any())
    off = np.concatenate([[0], np.cumsum([w.shape[0] for w in ws])])
    frozen = [(bn_m[off[i]:off[i + 1]].clone(), bn_r[off[i]:off[i + 1]].clone()) for i in range(len(ws))]
    chain = _chain(xd, convs, 18, frozen)
    assert bool(torch.isfinite(feats).all()) and torch.equal(feats, chain), f"max |diff| {(feats - chain).abs().max().item():.3e}"
