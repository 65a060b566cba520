"""The arithmetic of the 16-bit trunk's stages (csrc/resnet_b16.h) restated in numpy fp32, and the bars of
tests/trunk16_cases.py shown (a) to be reachable by that arithmetic in two summation orders on every case — the exact cases bit
for bit — and (b) to see the mutants a wrong kernel would be: a wrapped right-border pixel, a dropped tap, a dropped
16-channel chunk, truncation instead of round-to-nearest-even, statistics over the padded positions.  The derivations are in
the docstring of trunk16_cases.  CPU only: nothing here calls the library."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import trunk16_cases as tc
from trunk16_cases import KINDS

ORDERS = ("sequential", "blocks16_pairwise")


# ---- helpers ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_rounding_helpers_are_torchs(kind):
    rng = np.random.default_rng(0)
    span = 20 if kind == "bf16" else 6                      # (fp16: inside its range, subnormals included)
    a = (rng.standard_normal(200000) * np.exp(rng.uniform(-span, span, 200000))).astype(np.float32)
    a[:4] = [0.0, -0.0, 1.0, -2.5]
    r = tc.rne16(a, kind)
    assert np.array_equal(r, tc.torch_round(a, kind))
    assert np.array_equal(tc.rne16(r, kind), r)                                           # representable values are fixed points
    assert np.array_equal(tc.from_bits(tc.to_bits(r, kind), kind), r)
    t = tc.trunc16(a, kind)
    assert np.all(np.abs(t) <= np.abs(a)) and np.array_equal(tc.rne16(t, kind), t)        # toward zero, representable
    assert np.all((t == r) | (np.abs(r) > np.abs(a)))                                     # differs only where rne went away from zero
    ties = np.array([257.0, 258.0, 259.0, 2049.0, 2051.0, 4098.0, 1.00390625])
    want = {"bf16": [True, False, True, False, False, False, True], "fp16": [False, False, False, True, True, True, False]}[kind]
    assert tc.is_tie(ties, kind).tolist() == want
    assert tc.rne16(np.float32(257.0), "bf16") == 256.0 and tc.rne16(np.float32(259.0), "bf16") == 260.0     # to even


def test_layout_helpers():
    B, H, W, C = 3, 5, 4, 8
    x = tc.rne16(tc.relu_map(1, B, C, H, W, "bf16") + np.float32(1.0), "bf16")            # representable, no zeros inside
    buf = tc.pad_bits(x, "bf16")
    assert buf.shape == (tc.npos(B, H, W), C) == (B * (H + 1) * (W + 1) + W + 1, C)
    m = tc.border_mask(B, H, W)
    assert m.sum() == B * (W + 1 + H) + W + 1 and np.all(buf[m] == 0) and np.all(buf[~m] != 0)
    rows = np.arange(tc.npos(B, H, W)) // (W + 1)
    assert np.array_equal(m, (rows % (H + 1) == 0) | (np.arange(tc.npos(B, H, W)) % (W + 1) == W) | (rows == B * (H + 1)))
    back, border = tc.unpad(buf.view(np.int16), B, H, W, "bf16")
    assert np.array_equal(back, x.astype(np.float64)) and not border.any()


# ---- convolution: the reference arithmetic in two orders --------------------------------------------------------------------
def _columns(x, ks, stride, pad, pick):
    """im2col of NCHW x at the picked flat output pixels: [len(pick), K] fp32 (K ordered (cin, ky, kx)), as [image, pixel]."""
    cols = F.unfold(torch.from_numpy(np.ascontiguousarray(x, np.float32)), ks, padding=pad, stride=stride).numpy()   # [B, K, L]
    B, K, L = cols.shape
    return cols.transpose(0, 2, 1).reshape(B * L, K)[pick]


def _pick(n, k=40):
    """First, last and evenly spaced indices of range(n)."""
    return np.unique(np.concatenate([[0, n - 1], np.linspace(0, n - 1, min(n, k)).astype(int)]))


def _sequential(a, w):
    acc = np.zeros((a.shape[0], w.shape[0]), np.float32)
    for k in range(a.shape[1]):
        acc += a[:, k:k + 1] * w[None, :, k]              # exact products, one fp32 rounding per add
    return acc


def _blocks_pairwise(a, w):
    parts = [_sequential(a[:, k:k + 16], w[:, k:k + 16]) for k in range(0, a.shape[1], 16)]
    while len(parts) > 1:
        parts = [parts[i] + parts[i + 1] if i + 1 < len(parts) else parts[i] for i in range(0, len(parts), 2)]
    return parts[0]


def _conv_fp32(x, w16, ks, stride, pad, order):
    """The picked outputs of the conv in fp32: (values [pixels, channels], pixel index, channel index)."""
    B, _, Hi, Wi = x.shape
    L = tc.out_size(Hi, ks, stride, pad) * tc.out_size(Wi, ks, stride, pad)
    pix, ch = _pick(B * L), _pick(w16.shape[0], 48)
    a = _columns(x, ks, stride, pad, pix)
    wm = np.ascontiguousarray(w16[ch].reshape(len(ch), -1), np.float32)
    return (_sequential if order == "sequential" else _blocks_pairwise)(a, wm), pix, ch


def _at(s, pix, ch):
    """Elements [pixels, channels] of an NCHW array at flat (image, pixel) and channel indices."""
    B, C, H, W = s.shape
    return s.transpose(0, 2, 3, 1).reshape(B * H * W, C)[np.ix_(pix, ch)]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("name", [c[0] for c in tc.CONV_CASES])
def test_conv_reference_arithmetic_meets_the_bar(name, order, kind):
    _, B, Hi, Wi, Cin, Cout, ks, stride, pad = tc.CONV_BY_NAME[name]
    x, w, s, S = tc.conv_case(name, kind)
    assert np.array_equal(tc.rne16(x, kind), x) and not np.array_equal(tc.rne16(w, kind), w)
    acc, pix, ch = _conv_fp32(x, tc.rne16(w, kind), ks, stride, pad, order)
    got = tc.rne16(acc, kind).astype(np.float64)
    err, lim = np.abs(got - _at(s, pix, ch)), _at(tc.conv_bar(s, S, Cin * ks * ks, kind), pix, ch)
    print(f"{name} {kind} {order}: worst err / bar {tc.worst(err, lim):.3f}")
    assert np.all(err <= lim)


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("name", [c[0] for c in tc.EXACT_CASES])
def test_exact_conv_cases_are_exact_and_contain_ties(name, order):
    _, B, Hi, Wi, Cin, Cout, ks, stride, pad, tie_kinds = tc.EXACT_BY_NAME[name]
    x, w, s = tc.exact_case(name)
    assert set(np.unique(x)) <= {0.0, 1.0, 2.0} and np.all(np.isin(np.abs(w) * 2.0 ** (np.arange(Cout) % 4)[:, None, None, None], (0.0, 1.0)))
    acc, pix, ch = _conv_fp32(x, w, ks, stride, pad, order)
    assert np.array_equal(acc.astype(np.float64), _at(s, pix, ch))                       # every partial sum exact: fp32 == fp64
    for kind in KINDS:
        assert np.array_equal(tc.rne16(x, kind), x) and np.array_equal(tc.rne16(w, kind), w)
        ties = int(tc.is_tie(s, kind).sum())
        print(f"{name} {kind}: |s| up to {np.abs(s).max():g}, {ties} ties of {s.size}")
        assert np.abs(s).max() < 65504
        if kind in tie_kinds:
            assert ties >= 16
            assert np.any(tc.rne16(s, kind)[tc.is_tie(s, kind)] != tc.trunc16(np.float32(s), kind)[tc.is_tie(s, kind)])   # some round up


# ---- InstanceNorm and pool: the reference arithmetic in two orders ----------------------------------------------------------
def _fsum(a, order, fma_squares=False):
    """fp32 sum over the last axis: one by one, or numpy's pairwise blocks.  fma_squares: the sum of squares by fma(a, a, acc)
    (the square exact, one rounding per step) instead of rounded products."""
    a = np.ascontiguousarray(a, np.float32)
    if order == "sequential":
        acc = np.zeros(a.shape[:-1], np.float32)
        for p in range(a.shape[-1]):
            v = a[..., p]
            acc = (v.astype(np.float64) * v + acc).astype(np.float32) if fma_squares else acc + v
        return acc
    return np.add.reduce(a * a if fma_squares else a, axis=-1, dtype=np.float32)


def _norm_fp32(x, idn, relu, kind, order, pool=False, n_stat=None, rounder=None):
    """k_stats_b16 + k_apply_b16 (or k_pool_b16) in numpy fp32.  n_stat: the divisor of the statistics (mutant: the padded
    positions); rounder: the final rounding (mutant: truncation)."""
    B, C, H, W = x.shape
    n = np.float32(n_stat or H * W)
    xf = x.reshape(B, C, H * W).astype(np.float32)
    m = _fsum(xf, order) / n
    var = np.maximum(_fsum(xf, order, fma_squares=True) / n - m * m, np.float32(0))
    r = np.float32(1) / np.sqrt(var + np.float32(tc.EPS))
    t = (xf - m[..., None]) * r[..., None]
    if idn is not None:
        t = t + idn.reshape(B, C, H * W).astype(np.float32)
    if relu:
        t = np.maximum(t, np.float32(0))
    assert t.dtype == np.float32
    if pool:
        return _fsum(t, order) / np.float32(H * W)
    return (rounder or tc.rne16)(t, kind).reshape(B, C, H, W)


VARIANTS = [("plain", False, False), ("relu", False, True), ("residual", True, True)]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("name", [c[0] for c in tc.NORM_CASES])
def test_norm_reference_arithmetic_meets_the_bar(name, order, kind):
    x, idn = tc.norm_inputs(name, kind)
    assert np.array_equal(tc.rne16(x, kind), x) and np.array_equal(tc.rne16(idn, kind), idn)
    for vname, res, relu in VARIANTS:
        got = _norm_fp32(x, idn if res else None, relu, kind, order)
        ref, lim = tc.norm_reference(x, idn if res else None, relu, kind)
        err = np.abs(got.astype(np.float64) - ref)
        print(f"{name} {kind} {order} {vname}: worst err / bar {tc.worst(err, lim):.3f}")
        assert np.all(err <= lim)
    if x.shape[2] * x.shape[3] <= 200:          # the constant channel: reference exactly 0, bar small against the other channels' O(1)
        ref, lim = tc.norm_reference(x, None, False, kind)
        assert not ref[:, tc.CONST_CH].any() and lim[:, tc.CONST_CH].max() < 0.05
        assert lim[:, tc.SHIFT_CH].max() < 0.25     # mean 20, spread 0.5: the bar still says something


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("name", [c[0] for c in tc.POOL_CASES])
def test_pool_reference_arithmetic_meets_the_bar(name, order, kind):
    x, idn = tc.norm_inputs(name, kind)
    got = _norm_fp32(x, idn, True, kind, order, pool=True)
    ref, lim = tc.norm_reference(x, idn, True, kind, pool=True)
    err = np.abs(got.astype(np.float64) - ref)
    print(f"{name} {kind} {order}: worst err / bar {tc.worst(err, lim):.3f}")
    assert np.all(err <= lim)


# ---- the bars see the mutants -----------------------------------------------------------------------------------------------
def _wrapped(x, w16, stride):
    """3x3 pad-1 conv in fp64 whose zero right of the last column is the next row's first pixel (what reading a border
    position that was not kept zero gives in the shared-border layout)."""
    xp = np.pad(np.asarray(x, np.float64), ((0, 0), (0, 0), (1, 1), (1, 1)))
    xp[:, :, 1:-2, -1] = x[:, :, 1:, 0]
    return F.conv2d(torch.from_numpy(xp), torch.from_numpy(np.asarray(w16, np.float64)), stride=stride).numpy()


# one small shape per kernel family; the 1x1 conv has a single tap and reads no border
MUTANT_SHAPES = [("n_2x9x7", True, True), ("w_32_128", True, True), ("v_64_192", True, True), ("g3_64_128_9x7", True, True),
                 ("g1_128_256_9x7", False, False)]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name,wraps,taps", MUTANT_SHAPES)
def test_conv_bar_sees_the_mutants(name, wraps, taps, kind):
    _, B, Hi, Wi, Cin, Cout, ks, stride, pad = tc.CONV_BY_NAME[name]
    x, w, s, S = tc.conv_case(name, kind)
    w16 = tc.rne16(w, kind)
    lim = tc.conv_bar(s, S, Cin * ks * ks, kind)
    mutants = {}
    if wraps:
        mutants["wrapped right-border pixel"] = tc.rne16(_wrapped(x, w16, stride), kind)
    if taps:
        wt = w16.copy()
        wt[:, :, 0, 2] = 0
        mutants["dropped tap"] = tc.rne16(tc.conv_reference(x, wt, stride, pad)[0], kind)
    wc = w16.copy()
    wc[:, 16:32] = 0
    mutants["dropped 16-channel chunk"] = tc.rne16(tc.conv_reference(x, wc, stride, pad)[0], kind)
    mutants["truncation"] = tc.trunc16(np.float32(s), kind)
    mutants["unrounded weights"] = tc.rne16(tc.conv_reference(x, w, stride, pad)[0], kind)
    assert np.all(np.abs(tc.rne16(s, kind) - s) <= lim)                                   # (the unmutated reference is inside)
    for what, got in mutants.items():
        err = np.abs(got.astype(np.float64) - s)
        out = err > lim
        print(f"{name} {kind} {what}: worst err / bar {tc.worst(err, lim):.2f}, {int(out.sum())} of {out.size} outside")
        assert out.any(), what


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", ["c512_7", "c256_14"])
def test_norm_bar_sees_the_mutants(name, kind):
    _, B, H, W, C = tc.NORM_BY_NAME[name]
    x, idn = tc.norm_inputs(name, kind)
    for vname, res, relu in VARIANTS:
        ref, lim = tc.norm_reference(x, idn if res else None, relu, kind)
        mutants = {"statistics over the padded positions": _norm_fp32(x, idn if res else None, relu, kind, "sequential", n_stat=(H + 1) * (W + 1)),
                   "truncation": _norm_fp32(x, idn if res else None, relu, kind, "sequential", rounder=tc.trunc16)}
        for what, got in mutants.items():
            err = np.abs(got.astype(np.float64) - ref)
            print(f"{name} {kind} {vname} {what}: worst err / bar {tc.worst(err, lim):.2f}")
            assert np.any(err > lim), (vname, what)


@pytest.mark.parametrize("kind", KINDS)
def test_pool_bar_sees_padded_statistics(kind):
    _, B, H, W, C = tc.POOL_BY_NAME["p512_7"]
    x, idn = tc.norm_inputs("p512_7", kind)
    ref, lim = tc.norm_reference(x, idn, True, kind, pool=True)
    got = _norm_fp32(x, idn, True, kind, "sequential", pool=True, n_stat=(H + 1) * (W + 1))
    err = np.abs(got.astype(np.float64) - ref)
    print(f"p512_7 {kind} statistics over the padded positions: worst err / bar {tc.worst(err, lim):.2f}")
    assert np.any(err > lim)
