"""The arithmetic of the fp32-class trunk's kernels restated in numpy — the two-plane round-to-nearest fp16 cut, the three exact
plane products, fp32 accumulation in two different orders, the Winograd transforms in fp32, the per-tile (mean, M2) partials and
their merge, the fp32 pool and tail — shown (a) to meet every bar of tests/trunk32_cases.py on every case, the exact cases bit
for bit, and (b) to MISS a bar or an exact case once it is mutated the way a kernel could be wrong.  So the bars are reachable
by a correct kernel and tight enough to see the mutants.  CPU only: nothing here calls the library."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import trunk32_cases as tc
from trunk32_cases import PRECISIONS

f32 = np.float32
WS, OS = f32(256.0), f32(1.0 / 256.0)


# ---- the arithmetic ---------------------------------------------------------------------------------------------------------
def cut(a, precision):
    """fp32 -> (h0, h1) fp16 planes held as fp32; one plane for "half"."""
    a = np.asarray(a, f32)
    h0 = a.astype(np.float16).astype(f32)
    h1 = (a - h0).astype(np.float16).astype(f32) if precision == "fp32" else np.zeros_like(a)
    return h0, h1


def stage(x, in_stats, mut=None):
    """The staged conv input in fp32: x, or max((x - m) r, 0)."""
    x = np.asarray(x, f32)
    if in_stats is None:
        return x
    m, r = (np.asarray(t, f32)[:, :, None, None] for t in in_stats)
    v = (x - m) * r
    return v if mut == "no_relu" else np.maximum(v, f32(0))


def padded(xs, pad, mut=None):
    """Zero padding; the wrapped-border mutant reads column -1 as the previous row's last pixel."""
    B, C, H, W = xs.shape
    xp = np.zeros((B, C, H + 2 * pad, W + 2 * pad), f32)
    xp[:, :, pad:pad + H, pad:pad + W] = xs
    if mut == "wrap_border" and pad:
        xp[:, :, pad + 1:pad + H, pad - 1] = xs[:, :, :H - 1, W - 1]
    return xp


def planes_dot(a, b, precision, order, mut, drop_k0=16):
    """sum_k a[.., k] b[k, ..] as the kernels form it: the plane products h1 w0, h0 w1, h0 w0, each an exact fp32 product,
    added in fp32.  order 0: 16-wide chunks of k, the three products of a chunk in turn (the MFMA schedule); order 1: each
    product over the whole of k (reversed), the small ones added first."""
    a0, a1 = cut(a, precision)
    b0, b1 = cut(b, precision)
    prods = [(a1, b0), (a0, b1), (a0, b0)] if precision == "fp32" else [(a0, b0)]
    if mut == "drop_h1w0":
        prods = [p for p in prods if p[0] is not a1]
    if mut == "drop_h0w1":
        prods = [p for p in prods if p[1] is not b1]
    K = a.shape[-1]
    if order == 1:
        acc = None
        for pa, pb in prods:
            t = np.matmul(pa[..., ::-1], pb[::-1], dtype=f32)
            acc = t if acc is None else acc + t
        return acc
    acc = np.zeros(a.shape[:-1] + (b.shape[-1],), f32)
    for k0 in range(0, K, 16):
        if mut == "drop_chunk" and k0 == drop_k0:              # channels 16..31 (of the centre tap)
            continue
        for pa, pb in prods:
            acc = acc + np.matmul(pa[..., k0:k0 + 16], pb[k0:k0 + 16], dtype=f32)
    return acc


def rescale(acc, mut):
    out = acc * OS
    if mut == "no_rescale_block":
        out[..., 32:64] = acc[..., 32:64]
    return out


def emu_direct(x, w, stride, pad, in_stats, precision, order=0, mut=None, xs=None):
    """k_conv_s6 -> NCHW fp32.  k is (tap, channel) with the channels of a tap contiguous (16-channel chunks)."""
    xs = stage(x, in_stats, mut) if xs is None else xs
    B, C, H, W = xs.shape
    Co, _, ks, _ = w.shape
    Ho, Wo = tc.out_size(H, ks, stride, pad), tc.out_size(W, ks, stride, pad)
    xp = padded(xs, pad, mut)
    cols = np.empty((B, Ho, Wo, ks * ks, C), f32)
    for kh in range(ks):
        for kw in range(ks):
            cols[:, :, :, kh * ks + kw] = xp[:, :, kh:kh + stride * Ho:stride, kw:kw + stride * Wo:stride].transpose(0, 2, 3, 1)
    wk = (np.asarray(w, f32) * WS).transpose(2, 3, 1, 0).reshape(ks * ks, C, Co).copy()
    if mut == "drop_tap":
        wk[ks * ks // 2] = 0
    y = planes_dot(cols.reshape(B, Ho, Wo, ks * ks * C), wk.reshape(ks * ks * C, Co), precision, order, mut, (ks * ks // 2) * C + 16)
    return np.ascontiguousarray(rescale(y, mut).transpose(0, 3, 1, 2))


def emu_wino_tiles(x, w, in_stats, precision, order=0, mut=None):
    """k_conv_wino_s3 / _w1 -> the 2x2 output tiles [B, TY, TX, 2, 2, Cout] fp32 (before the map's edge is cut)."""
    xs = stage(x, in_stats, mut)
    B, C, H, W = xs.shape
    TY, TX = (H + 1) // 2, (W + 1) // 2
    xp = np.zeros((B, C, 2 * TY + 2, 2 * TX + 2), f32)
    xp[:, :, :H + 2, :W + 2] = padded(xs, 1, mut)
    d = np.empty((B, TY, TX, 4, 4, C), f32)                 # the 4x4 input patches of the 2x2 output tiles
    for i in range(4):
        for j in range(4):
            d[:, :, :, i, j, :] = xp[:, :, i:i + 2 * TY:2, j:j + 2 * TX:2].transpose(0, 2, 3, 1)

    def bt(v, ax):                                          # B^T along one axis, the kernel's four differences
        r = [np.take(v, i, ax) for i in range(4)]
        return np.stack([r[0] - r[2], r[1] + r[2], r[2] - r[1], r[1] - r[3]], ax)

    def gg(v, ax):                                          # G along one axis, as k_pack_wino_s3: 0.5 (a + b + c), 0.5 (a - b + c)
        r = [np.take(v, i, ax) for i in range(3)]
        return np.stack([r[0], f32(0.5) * (r[0] + r[1] + r[2]), f32(0.5) * (r[0] - r[1] + r[2]), r[2]], ax)

    def at(v, ax):                                          # A^T along one axis
        r = [np.take(v, i, ax) for i in range(4)]
        return np.stack([r[0] + r[1] + r[2], r[1] - r[2] - r[3]], ax)

    g = np.asarray(w, f32).copy()
    if mut == "drop_tap":
        g[:, :, 1, 1] = 0
    V = bt(bt(d, 3), 4) if order == 0 else bt(bt(d, 4), 3)
    U = (gg(gg(g, 2), 3) if order == 0 else gg(gg(g, 3), 2)) * WS           # [Co, C, 4, 4]
    M = np.empty(V.shape[:5] + (g.shape[0],), f32)
    for i in range(4):
        for j in range(4):
            M[:, :, :, i, j] = planes_dot(V[:, :, :, i, j], np.ascontiguousarray(U[:, :, i, j].T), precision, order, mut)
    Y = at(at(M, 4), 3) if order == 0 else at(at(M, 3), 4)
    return rescale(Y, mut)


def emu_wino(x, w, in_stats, precision, order=0, mut=None):
    return tc.wino_untile(emu_wino_tiles(x, w, in_stats, precision, order, mut), x.shape[2], x.shape[3])


def _fsum(v, order):
    """fp32 sum along the last axis: numpy's pairwise order, or strictly sequential."""
    return v.sum(-1, dtype=f32) if order == 0 else np.cumsum(v, -1, dtype=f32)[..., -1]


def emu_stats(y, order=0, ts=32, flat=True, mut=None, extra=None):
    """(mean, rstd) fp32 [B, C] from per-piece (cnt, mean, M2) partials merged as the finalize kernels do.  flat: the pieces of
    image n are its intersections with the `ts`-pixel tiles of the flattened (image, pixel) axis (tiles straddle images);
    otherwise tiles of `ts` from each image's first pixel.  extra [B, C, k]: values wrongly counted with the last piece."""
    B, C = y.shape[:2]
    v = np.asarray(y, f32).reshape(B, C, -1)
    n = v.shape[2]
    mean, rstd = np.empty((B, C), f32), np.empty((B, C), f32)
    for b in range(B):
        lo, pieces = b * n if flat else 0, []
        p = lo
        while p < lo + n:
            q = min((p // ts + 1) * ts, lo + n)
            pieces.append((p - lo, q - lo, p // ts * ts < lo))          # (from, to, the tile began in the previous image)
            p = q
        parts = []
        for a, e, second in pieces:
            seg = v[b, :, a:e]
            if extra is not None and e == n:
                seg = np.concatenate([seg, extra[b]], 1)
            cnt = f32(seg.shape[1] + (1 if mut == "count_plus_one" and second else 0))
            mt = _fsum(seg, order) / cnt
            dlt = seg - mt[:, None]
            if mut == "skip_second_slot" and second:
                continue
            parts.append((cnt, mt, _fsum(dlt * dlt, order)))
        if not parts:                                       # (a mutant that skipped every piece of the image)
            mean[b], rstd[b] = 0, tc.RSTD0
            continue
        tot = f32(n) if extra is None else f32(sum(p[0] for p in parts))
        mu = _fsum(np.stack([p[0] * p[1] for p in parts], -1), order) / tot
        m2 = _fsum(np.stack([p[2] + p[0] * (p[1] - mu) * (p[1] - mu) for p in parts], -1), order)
        mean[b], rstd[b] = mu, f32(1.0) / np.sqrt(m2 / tot + f32(1e-5))
    return mean, rstd


def emu_conv(name, precision, order=0, mut=None):
    x, w, st, stride, pad, wino = tc.conv_case(name)
    return emu_wino(x, w, st, precision, order, mut) if wino else emu_direct(x, w, stride, pad, st, precision, order, mut)


def stats_ok(mean, rstd, exp):
    m, r, dm, dr = exp
    return tc.worst(np.abs(mean - m), dm), tc.worst(np.abs(rstd - r), dr)


# ---- (a) the arithmetic meets every bar ---------------------------------------------------------------------------------------
ALL_CONV = [c[0] for c in tc.DIRECT_CASES + tc.WINO_CASES]


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("name", ALL_CONV)
def test_conv_arithmetic_meets_the_bar_in_two_orders(name, precision):
    s, bar, st = tc.conv_expected(name, precision)
    for order in (0, 1):
        y = emu_conv(name, precision, order)
        assert y.shape == s.shape
        wy = tc.worst(np.abs(y - s), bar)
        wm, wr = stats_ok(*emu_stats(y, order, ts=32 if order == 0 else 7, flat=order == 0), st)
        print(f"{name} {precision} order {order}: conv {wy:.3f} mean {wm:.3f} rstd {wr:.3f} of the bar")
        assert wy <= 1 and wm <= 1 and wr <= 1
        zr = emu_stats(y, order)[1][:, tc.ZERO_CH]
        assert np.all(y[:, tc.ZERO_CH] == 0) and np.all(np.abs(zr - tc.RSTD0) <= 8 * tc.U32 * tc.RSTD0)


@pytest.mark.parametrize("name", [c[0] for c in tc.EXACT_CASES])
def test_exact_cases_are_exact_in_two_orders(name):
    x, w, stride, pad, wino, s = tc.exact_case(name)
    flav = tc.BY_NAME[name][-1]
    h1x, h1w = cut(x, "fp32")[1], cut(w * WS, "fp32")[1]
    assert np.any(h1x != 0) == (flav == "xwide") and np.any(h1w != 0) == (flav == "wwide")
    for order in (0, 1):
        y = emu_wino(x, w, None, "fp32", order) if wino else emu_direct(x, w, stride, pad, None, "fp32", order)
        assert np.array_equal(y.astype(np.float64), s), (name, order)
    if flav == "plain":                                         # one plane holds these operands: "half" is exact too
        y = emu_wino(x, w, None, "half") if wino else emu_direct(x, w, stride, pad, None, "half")
        assert np.array_equal(y.astype(np.float64), s)


# ---- stem ---------------------------------------------------------------------------------------------------------------------
def emu_stem_conv(x, w, precision, order=0, mut=None):
    x32 = (x.transpose(0, 3, 1, 2).astype(f32) / f32(255.0)) if x.dtype == np.uint8 else x
    return emu_direct(None, w, 2, 3, None, precision, order, mut, xs=np.ascontiguousarray(x32, f32))


def emu_pool(y, mean, rstd, mut=None):
    """relu((window extreme - mean) rstd), NCHW fp32: the maximum, or the minimum where rstd < 0."""
    B, C, H1, W1 = y.shape
    t = torch.from_numpy(np.ascontiguousarray(y))
    mx = F.max_pool2d(t, 3, 2, 1).numpy()
    if mut == "skip_halo":                                      # pool rows py % 8 == 0 (py > 0) lose the conv row above them
        Hp = mx.shape[2]
        for py in range(8, Hp, 8):
            rows = t[:, :, 2 * py:2 * py + 2]
            mx[:, :, py] = F.max_pool2d(rows, (rows.shape[2], 3), (1, 2), (0, 1)).numpy()[:, :, 0]
    mn = -F.max_pool2d(-t, 3, 2, 1).numpy()
    r = rstd[:, :, None, None]
    ext = mx if mut == "max_negative_r" else np.where(r >= 0, mx, mn)
    return np.maximum((ext - mean[:, :, None, None]) * r, f32(0))


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("name", [c[0] for c in tc.STEM_CASES])
def test_stem_arithmetic_meets_the_bar(name, precision):
    x, w, fz = tc.stem_case(name)
    ref, bar, m, r, dm, dr = tc.stem_expected(name, precision)
    for order in (0, 1):
        y = emu_stem_conv(x, w, precision, order)
        B = y.shape[0]
        mean, rstd = (np.tile(fz[0], (B, 1)), np.tile(fz[1], (B, 1))) if fz else emu_stats(y, order, flat=False)
        got = emu_pool(y, mean, rstd)
        wp, (wm, wr) = tc.worst(np.abs(got - ref), bar), stats_ok(mean, rstd, (m, r, dm, dr))
        print(f"{name} {precision} order {order}: pooled {wp:.3f} mean {wm:.3f} rstd {wr:.3f} of the bar")
        assert got.shape == ref.shape and wp <= 1 and wm <= 1 and wr <= 1


@pytest.mark.parametrize("name", [c[0] for c in tc.STEM_EXACT])
def test_stem_exact_cases_are_exact(name):
    x, w, s = tc.stem_exact_case(name)
    for order in (0, 1):
        assert np.array_equal(emu_stem_conv(x, w, "fp32", order).astype(np.float64), s)


# ---- tail ---------------------------------------------------------------------------------------------------------------------
def emu_tail(kind, y2, st, idn, dst, fma):
    m, r = (t[:, None, :] for t in st)
    i = idn if dst is None else (idn - dst[0][:, None, :]) * dst[1][:, None, :]
    d = y2 - m
    t = (d.astype(np.float64) * r + i).astype(f32) if fma else d * r + i
    val = np.maximum(t, f32(0))
    if kind != "pool":
        return val
    return np.cumsum(val, 1, dtype=f32)[:, -1] / f32(val.shape[1])


@pytest.mark.parametrize("name", [c[0] for c in tc.TAIL_CASES])
def test_tail_arithmetic_meets_the_bar(name):
    y2, st, idn, dst = tc.tail_case(name)
    kind = tc.BY_NAME[name][1]
    ref, bar = tc.tail_reference(kind, y2, st, idn, dst)
    for fma in (False, True):
        w = tc.worst(np.abs(emu_tail(kind, y2, st, idn, dst, fma) - ref), bar)
        print(f"{name} fma {fma}: {w:.3f} of the bar")
        assert w <= 1
    if kind != "pool":                                          # a stale set of statistics (the previous image's) is seen
        stale = tuple(np.roll(t, 1, 0) for t in st)
        assert tc.worst(np.abs(emu_tail(kind, y2, stale, idn, dst, False) - ref), bar) > 100


# ---- (b) the bars and the exact cases see the mutants -----------------------------------------------------------------------
def _conv_miss(name, precision, mut):
    s, bar, _ = tc.conv_expected(name, precision)
    return tc.worst(np.abs(emu_conv(name, precision, 0, mut) - s), bar)


def _exact_differs(name, mut):
    x, w, stride, pad, wino, s = tc.exact_case(name)
    y = emu_wino(x, w, None, "fp32", 0, mut) if wino else emu_direct(x, w, stride, pad, None, "fp32", 0, mut)
    return not np.array_equal(y.astype(np.float64), s)


@pytest.mark.parametrize("name", ["x42_xwide", "xu_xwide", "xw_xwide"])
def test_mutant_dropped_h1w0_breaks_the_xwide_exact_cases(name):
    assert _exact_differs(name, "drop_h1w0") and not _exact_differs(name, "drop_h0w1")


@pytest.mark.parametrize("name", ["x22_wwide", "xu_wwide", "xw_wwide"])
def test_mutant_dropped_h0w1_breaks_the_wwide_exact_cases(name):
    assert _exact_differs(name, "drop_h0w1") and not _exact_differs(name, "drop_h1w0")


def test_mutant_dropped_cross_products_break_the_stem_exact_cases():
    for name, mut, other in (("sx_xwide", "drop_h1w0", "drop_h0w1"), ("sx_wwide", "drop_h0w1", "drop_h1w0")):
        x, w, s = tc.stem_exact_case(name)
        assert not np.array_equal(emu_stem_conv(x, w, "fp32", 0, mut).astype(np.float64), s)
        assert np.array_equal(emu_stem_conv(x, w, "fp32", 0, other).astype(np.float64), s)


@pytest.mark.parametrize("mut", ["no_rescale_block", "drop_tap", "drop_chunk", "wrap_border", "no_relu"])
@pytest.mark.parametrize("precision", PRECISIONS)
def test_conv_mutants_miss_the_bar_of_every_case_they_apply_to(mut, precision):
    seen = 0
    for c in tc.DIRECT_CASES + tc.WINO_CASES:
        name, wino, norm = c[0], len(c) == 7, c[-1]
        pad = 1 if wino else c[8]
        if (mut == "no_relu" and not norm) or (mut == "wrap_border" and (pad == 0 or c[2] < 2)):
            continue
        miss = _conv_miss(name, precision, mut)
        print(f"{mut} {precision} {name}: {miss:.1f} x the bar")
        assert miss > 2, (mut, name)
        seen += 1
    assert seen >= 6


def test_exact_cases_see_the_structural_mutants_too():
    for name in ("x22", "xu", "xw"):
        for mut in ("no_rescale_block", "drop_tap", "drop_chunk", "wrap_border"):
            assert _exact_differs(name, mut), (name, mut)


def test_mutant_next_images_mean_on_a_straddling_tile():
    """1x1 / stride 1 NORM cases: output pixel = input pixel, so the rows of a 32-pixel tile that belong to the next image are
    the rows staged with the wrong statistics."""
    for name in ("d42_1x1_9x7", "d42_bneck", "d42_hw1"):
        x, w, (m, r), stride, pad, _ = tc.conv_case(name)
        B, C, H, W = x.shape
        first = (np.arange(B * H * W) // 32 * 32) // (H * W)            # the image in which each pixel's tile begins
        mm, rr = m[first].reshape(B, H, W, C).transpose(0, 3, 1, 2), r[first].reshape(B, H, W, C).transpose(0, 3, 1, 2)
        xs = np.maximum((x - mm) * rr, f32(0))
        s, bar, _ = tc.conv_expected(name, "fp32")
        assert tc.worst(np.abs(emu_direct(None, w, stride, pad, None, "fp32", 0, None, xs=xs) - s), bar) > 100, name


@pytest.mark.parametrize("mut", ["count_plus_one", "skip_second_slot"])
def test_statistics_mutants_on_straddling_tiles(mut):
    for name in ("d42_1x1_5x7", "d42_1x1_9x7", "d22_s2_7x5", "d42_bneck", "d24_1x1_9x7"):
        _, _, st = tc.conv_expected(name, "fp32")
        wm, wr = stats_ok(*emu_stats(emu_conv(name, "fp32"), 0, mut=mut), st)
        print(f"{mut} {name}: mean {wm:.1f} rstd {wr:.1f} x the bar")
        assert max(wm, wr) > 2, (mut, name)


def test_statistics_mutant_out_of_map_half_of_an_odd_winograd_tile():
    for name in ("u_1x1", "u_3x3", "u_5x7", "w_5x7", "w_63x2"):
        x, w, ist, _, _, _ = tc.conv_case(name)
        tiles = emu_wino_tiles(x, w, ist, "fp32")
        full = tiles.transpose(0, 5, 1, 3, 2, 4).reshape(tiles.shape[0], tiles.shape[5], 2 * tiles.shape[1], 2 * tiles.shape[2])
        H, W = x.shape[2:]
        B, Co = full.shape[:2]
        extra = np.concatenate([full[:, :, H:, :].reshape(B, Co, -1), full[:, :, :H, W:].reshape(B, Co, -1)], 2)
        assert extra.shape[2] > 0 and np.any(extra != 0)
        _, _, st = tc.conv_expected(name, "fp32")
        wm, wr = stats_ok(*emu_stats(full[:, :, :H, :W], 0, ts=64, flat=False, extra=extra), st)
        print(f"odd half {name}: mean {wm:.1f} rstd {wr:.1f} x the bar")
        assert max(wm, wr) > 2, name


def test_pool_mutants():
    for name, mut in (("s96x80_u8", "skip_halo"), ("s96x80_f", "skip_halo"), ("s34x38_f_bn", "max_negative_r"), ("s65x33_u8_bn", "max_negative_r")):
        x, w, fz = tc.stem_case(name)
        ref, bar = tc.stem_expected(name, "fp32")[:2]
        y = emu_stem_conv(x, w, "fp32")
        B = y.shape[0]
        mean, rstd = (np.tile(fz[0], (B, 1)), np.tile(fz[1], (B, 1))) if fz else emu_stats(y, 0, flat=False)
        miss = tc.worst(np.abs(emu_pool(y, mean, rstd, mut) - ref), bar)
        print(f"{mut} {name}: {miss:.1f} x the bar")
        assert miss > 10, (name, mut)
