"""The kernels of the 16-bit activation trunk (csrc/resnet_b16.h), ONE AT A TIME through the dsmil_trunk16_* entries, against
fp64 at the derived bars of tests/trunk16_cases.py (tests/test_trunk16_host.py shows the reference arithmetic reaches them and
that they see a wrapped border pixel, a dropped tap or chunk, truncation and padded statistics).  Both element types for every
case.  Then the trunk's wiring: b16::trunk equals, bit for bit, the chain of its stages.  Needs a real MI355X."""
import numpy as np
import pytest
import torch

import trunk16_cases as tc
from trunk16_cases import KINDS

pytestmark = pytest.mark.gpu


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _bits_dev(x_nchw, kind):
    """A representable NCHW map as the int16 device buffer the kernels read (built on the host: independent of k_b16_pad)."""
    return _dev(tc.pad_bits(x_nchw, kind).view(np.int16))


def _host(buf):
    return buf.cpu().numpy().view(np.uint16)


# ---- layout -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("B,H,W,C", [(2, 5, 7, 64), (3, 9, 3, 8), (2, 1, 1, 512)])
def test_pad_is_exact_and_borders_zero_only_the_borders(B, H, W, C, kind):
    from dsmil_wsi_amd import ops
    x = tc.relu_map(11 + H, B, C, H, W, kind) + np.float32(0.5)                 # representable, no zero inside
    x = tc.rne16(x, kind)
    nhwc = _dev(x.transpose(0, 2, 3, 1))
    got = _host(ops.trunk16_layout(nhwc, kind))
    assert got.shape == (ops.trunk16_positions(B, H, W), C) == (tc.npos(B, H, W), C)
    assert np.array_equal(got, tc.pad_bits(x, kind))                            # exact inside, zero on every border position
    # arbitrary fp32 (not representable): round to nearest even, as torch's cast
    y = (np.random.default_rng(3).standard_normal((B, C, H, W)) * 3).astype(np.float32)
    got = _host(ops.trunk16_layout(_dev(y.transpose(0, 2, 3, 1)), kind))
    assert np.array_equal(got, tc.pad_bits(tc.torch_round(y, kind), kind))
    # borders mode: a buffer of bytes 0x3C in which exactly the border positions became zero
    got = _host(ops.trunk16_layout(nhwc, kind, borders_only=True))
    m = tc.border_mask(B, H, W)
    assert not got[m].any() and np.all(got[~m] == 0x3C3C)


# ---- convolution ------------------------------------------------------------------------------------------------------------
def _run_conv(x, w, stride, pad, kind):
    from dsmil_wsi_amd import ops
    B, _, Hi, Wi = x.shape
    out, Ho, Wo = ops.trunk16_conv(_bits_dev(x, kind), _dev(w), B, Hi, Wi, stride, pad, kind)
    got, border = tc.unpad(_host(out), B, Ho, Wo, kind)
    assert out.shape[1] == w.shape[0] and not border.any(), "border positions / the closing row are not zero"
    return got


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", [c[0] for c in tc.CONV_CASES])
def test_conv_vs_fp64(name, kind):
    _, B, Hi, Wi, Cin, Cout, ks, stride, pad = tc.CONV_BY_NAME[name]
    x, w, s, S = tc.conv_case(name, kind)
    got = _run_conv(x, w, stride, pad, kind)
    assert got.shape == s.shape
    err, lim = np.abs(got - s), tc.conv_bar(s, S, Cin * ks * ks, kind)
    print(f"conv {name} {kind}: max err {err.max():.3e}, worst err / bar {tc.worst(err, lim):.3f}")
    assert np.all(err <= lim)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", [c[0] for c in tc.EXACT_CASES])
def test_conv_exact_case_bit_for_bit(name, kind):
    _, B, Hi, Wi, Cin, Cout, ks, stride, pad, _ = tc.EXACT_BY_NAME[name]
    x, w, s = tc.exact_case(name)
    got = _run_conv(x, w, stride, pad, kind)
    want = tc.rne16(s, kind).astype(np.float64)
    bad = got != want
    print(f"conv {name} {kind}: {int(bad.sum())} of {bad.size} differ, {int(tc.is_tie(s, kind).sum())} ties")
    assert not bad.any()


@pytest.mark.parametrize("kind", KINDS)
def test_conv_refuses_maps_wider_than_its_window(kind):
    from dsmil_wsi_amd import ops
    for B, Hi, Wi, Cin, Cout in tc.CONV_REFUSED:
        x = np.zeros((B, Cin, Hi, Wi), np.float32)
        with pytest.raises(NotImplementedError):
            ops.trunk16_conv(_bits_dev(x, kind), _dev(tc.conv_weights(1, Cout, Cin, 3)), B, Hi, Wi, 1, 1, kind)


# ---- InstanceNorm and pool --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", [c[0] for c in tc.NORM_CASES])
def test_norm_vs_fp64(name, kind):
    from dsmil_wsi_amd import ops
    _, B, H, W, C = tc.NORM_BY_NAME[name]
    x, idn = tc.norm_inputs(name, kind)
    idn_d = _bits_dev(idn, kind)
    for vname, res, relu in (("plain", False, False), ("relu", False, True), ("residual", True, True)):
        ref, lim = tc.norm_reference(x, idn if res else None, relu, kind)
        buf = _bits_dev(x, kind)
        out = ops.trunk16_norm(buf, B, H, W, kind, idn=idn_d if res else None, relu=relu, out=buf)        # in place, as the trunk
        got, border = tc.unpad(_host(out), B, H, W, kind)
        err = np.abs(got - ref)
        print(f"norm {name} {kind} {vname}: max err {err.max():.3e}, worst err / bar {tc.worst(err, lim):.3f}")
        assert not border.any() and np.all(err <= lim)
        if H * W <= 200 and not res:                    # the constant channel: the variance clamps, the output stays within the bar of 0
            assert not ref[:, tc.CONST_CH].any() and np.all(np.abs(got[:, tc.CONST_CH]) <= lim[:, tc.CONST_CH])
        if vname == "residual":
            # out of place into a buffer of 0x3C bytes: the same bits on the images' positions, the closing row left alone
            dst = torch.full_like(buf, 0x3C3C)
            ops.trunk16_norm(_bits_dev(x, kind), B, H, W, kind, idn=idn_d, relu=True, out=dst)
            d, o = _host(dst), _host(out)
            closing = B * (H + 1) * (W + 1)
            assert np.array_equal(d[:closing], o[:closing]) and np.all(d[closing:] == 0x3C3C)


def test_norm_residual_without_relu_is_refused():
    from dsmil_wsi_amd import ops
    x, idn = tc.norm_inputs("c512_2x2", "bf16")
    with pytest.raises(NotImplementedError):
        ops.trunk16_norm(_bits_dev(x, "bf16"), 3, 2, 2, "bf16", idn=_bits_dev(idn, "bf16"), relu=False)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", [c[0] for c in tc.POOL_CASES])
def test_pool_vs_fp64(name, kind):
    from dsmil_wsi_amd import ops
    _, B, H, W, C = tc.POOL_BY_NAME[name]
    x, idn = tc.norm_inputs(name, kind)
    ref, lim = tc.norm_reference(x, idn, True, kind, pool=True)
    got = ops.trunk16_pool(_bits_dev(x, kind), _bits_dev(idn, kind), B, H, W, kind).cpu().numpy().astype(np.float64)
    err = np.abs(got - ref)
    print(f"pool {name} {kind}: max err {err.max():.3e}, worst err / bar {tc.worst(err, lim):.3f}")
    assert got.shape == (B, C) and np.all(err <= lim)


# ---- the trunk's wiring -----------------------------------------------------------------------------------------------------
def _chain(x_nhwc, convs, depth, kind):
    """The trunk as a chain of its stages, in the block order of oracle/resnet_oracle.py::_block (conv1 -> IN -> ReLU; the
    downsample conv -> IN on the block's input; conv2 -> IN, + identity, ReLU; the last block's tail is the pool)."""
    from dsmil_wsi_amd import ops
    B, H, W, _ = x_nhwc.shape
    cur = ops.trunk16_layout(x_nhwc, kind)
    nblk = {18: (2, 2, 2, 2), 34: (3, 4, 6, 3)}[depth]
    ci = 1
    for l, n in enumerate(nblk):
        for b in range(n):
            down = l > 0 and b == 0
            r1, Ho, Wo = ops.trunk16_conv(cur, convs[ci], B, H, W, 2 if down else 1, 1, kind)
            ops.trunk16_norm(r1, B, Ho, Wo, kind, relu=True, out=r1)
            idn = cur
            if down:
                idn, Hd, Wd = ops.trunk16_conv(cur, convs[ci + 2], B, H, W, 2, 0, kind)
                assert (Hd, Wd) == (Ho, Wo)
                ops.trunk16_norm(idn, B, Ho, Wo, kind, relu=False, out=idn)
            r2, _, _ = ops.trunk16_conv(r1, convs[ci + 1], B, Ho, Wo, 1, 1, kind)
            if l == 3 and b == n - 1:
                return ops.trunk16_pool(r2, idn, B, Ho, Wo, kind)
            cur = ops.trunk16_norm(r2, B, Ho, Wo, kind, idn=idn, relu=True, out=r2)
            ci += 3 if down else 2
            H, W = Ho, Wo


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("depth", [18, 34])
def test_trunk_equals_the_chain_of_its_stages_bit_for_bit(depth, kind):
    from dsmil_wsi_amd import ops
    x, ws = tc.trunk_inputs(depth, kind)                       # B = 3, 9 x 9 -> 5 -> 3 -> 2
    xd, convs = _dev(x), [_dev(w) for w in ws]
    feats = ops.trunk16_forward(xd, convs, kind)
    again = ops.trunk16_forward(xd, convs, kind)
    chain = _chain(xd, convs, depth, kind)
    torch.cuda.synchronize()
    assert feats.shape == (3, 512) and bool(torch.isfinite(feats).all()) and float(feats.abs().max()) > 0.1
    assert torch.equal(feats, again)                           # no atomics: two runs, equal bits
    assert torch.equal(feats, chain)                           # buffer rotation and pack offsets of trunk_t
