"""dsmil_simclr_views_host (the kernel's per-pixel functions compiled for the host) against the Pillow oracle of
simclr_aug_cases.py, stage by stage and as a chain; draw_view_params' distributions; the rejections.  No GPU."""
import math

import numpy as np
import pytest
import torch

import dsmil  # noqa: F401  (registers the dsmil_wsi_amd package)
import simclr_aug_cases as C
from dsmil_wsi_amd import ops, simclr


def params(recs):
    g = lambda k: [r[k] for r in recs]      # noqa: E731
    f = lambda bit: [bool(r["flags"] & bit) for r in recs]      # noqa: E731
    return simclr.ViewParams(g("tile"), g("i"), g("j"), g("h"), g("w"), f(C.FLIP), f(C.JITTER), f(C.GREY), f(C.BLUR),
                             [list(r["order"]) for r in recs], g("brightness"), g("contrast"), g("saturation"), g("hue"), g("sigma"))


def run(tile_batch, recs, S, out="uint8"):
    return ops.simclr_views(torch.from_numpy(tile_batch), params(recs), S, out=out).numpy()


def check(what, got, ref, recs, S):
    """Prints the share of differing bytes and the largest difference, then holds every record to its bar."""
    d = np.abs(got.astype(np.int32) - ref.astype(np.int32))
    print(f"{what}: {np.mean(d != 0):.3e} of the bytes differ, by at most {d.max()}")
    for k, r in enumerate(recs):
        assert d[k].max() <= C.bar(r, S), (what, k, r, int(d[k].max()))


@pytest.fixture(scope="module", params=C.SHAPES, ids=C.SHAPE_IDS)
def shape(request):
    name, H, W, S, _ = request.param
    return request.param, C.tiles(3, H, W, seed=len(name) + S)


STAGES = [("resize", {}), ("flip", dict(flags=C.FLIP)), ("grey", dict(flags=C.GREY)),
          ("blur_narrow", dict(flags=C.BLUR, sigma=0.1)), ("blur", dict(flags=C.BLUR, sigma=1.3)),
          ("blur_wide", dict(flags=C.BLUR, sigma=2.0))]
for _name, _op in (("brightness", C.BRIGHTNESS), ("contrast", C.CONTRAST), ("saturation", C.SATURATION)):
    for _f in (0.0, 0.2, 1.0, 1.8):
        # the blend under test runs second, behind the hue round trip at shift 0 that a jittered view always has
        STAGES.append((f"{_name}_{_f}", dict(flags=C.JITTER, order=[C.HUE, _op] + [o for o in range(3) if o != _op], **{_name: _f})))
for _h in (0, 1, 128, 255):
    STAGES.append((f"hue_{_h}", dict(flags=C.JITTER, hue=_h)))


@pytest.mark.parametrize("stage", STAGES, ids=[s[0] for s in STAGES])
def test_each_stage_alone(shape, stage):
    (name, H, W, S, _), tl = shape
    recs = C.crops(shape[0], **stage[1])
    check(f"{name} {stage[0]}", run(tl, recs, S), C.views(tl, recs, S), recs, S)


def test_contrast_mean_is_pillows(shape):
    """Contrast at factor 0 leaves the degenerate image: the constant int(mean(L) + 0.5) of the view at that stage."""
    (name, H, W, S, _), tl = shape
    recs = C.crops(shape[0], flags=C.JITTER, contrast=0.0, order=(C.CONTRAST, C.BRIGHTNESS, C.SATURATION, C.HUE))
    got = run(tl, recs, S)
    for k, r in enumerate(recs):
        assert (got[k] == C.contrast_mean(C.crop_resize(tl[r["tile"]], r, S))).all()


def test_full_chain_in_all_24_orders(shape):
    (name, H, W, S, _), tl = shape
    recs = C.full_chain_records(shape[0], seed=S)
    assert sorted(r["order"] for r in recs if r["flags"] == 15) == sorted(C.ORDERS)          # all flags on, every order
    assert sorted(r["order"] for r in recs if r["flags"] == 15 - C.GREY) == sorted(C.ORDERS)
    check(f"{name} chain", run(tl, recs, S), C.views(tl, recs, S), recs, S)


def test_mixed_flags(shape):
    (name, H, W, S, _), tl = shape
    recs = C.mixed_flag_records(shape[0], 3, seed=S + 1)
    check(f"{name} mixed", run(tl, recs, S), C.views(tl, recs, S), recs, S)


def test_float_output_is_the_bytes_over_255(shape):
    (name, H, W, S, _), tl = shape
    recs = C.mixed_flag_records(shape[0], 3, seed=S + 2)
    u8, f32 = run(tl, recs, S), run(tl, recs, S, out="float")
    assert f32.dtype == np.float32 and f32.shape == (len(recs), 3, S, S)
    assert np.array_equal(f32, u8.transpose(0, 3, 1, 2).astype(np.float32) / np.float32(255.0))


def test_L_and_hsv_round_trip_over_the_rgb_cube():
    """The shared per-pixel functions on every 5th level per channel (52^3 colours), through an identity crop."""
    cube, n = C.rgb_cube(5)
    assert n == 52 ** 3
    for flags in (C.GREY, C.JITTER):
        recs = [C.record(tile=k, h=224, w=224, flags=flags) for k in range(len(cube))]
        assert np.array_equal(run(cube, recs, 224), C.views(cube, recs, 224))


# ---- draw_view_params ----------------------------------------------------------------------------------------------------
def _draw(n, H, W, seed, **kw):
    return simclr.draw_view_params(n, H, W, 224, generator=torch.Generator().manual_seed(seed), **kw)


def test_draw_is_seeded_and_pairs_views_with_tiles():
    a, b, c = _draw(50, 224, 224, 7), _draw(50, 224, 224, 7), _draw(50, 224, 224, 8)
    assert torch.equal(a.records, b.records) and not torch.equal(a.records, c.records)
    assert a.records.shape == (100, 12) and a.records.dtype == torch.int32 and a.floats.dtype == torch.float32
    assert a.ints[:, 0].tolist() == [k // 2 for k in range(100)]
    assert a.floats.data_ptr() == a.records.data_ptr() + 32       # one buffer: struct dsmil_simclr_view per row


def test_draw_distributions():
    n = 10000                                                      # 20 000 records
    p = _draw(n, 200, 256, 11)
    t, i, j, h, w, flags, order, hue = (p.ints[:, k].long() for k in range(8))
    assert ((h >= 1) & (w >= 1) & (i >= 0) & (j >= 0) & (i + h <= 200) & (j + w <= 256)).all()
    area, ratio = (h * w).double() / (200 * 256), w.double() / h.double()
    assert area.min() > 0.07 and area.max() <= 1.0 and area.mean() > 0.4 and ratio.min() > 0.70 and ratio.max() < 1.40
    for bit, prob in ((C.FLIP, 0.5), (C.JITTER, 0.8), (C.GREY, 0.2), (C.BLUR, 0.5)):
        rate = ((flags & bit) != 0).double().mean().item()
        assert abs(rate - prob) <= 4 * math.sqrt(prob * (1 - prob) / (2 * n)), (bit, rate)
    f = p.floats
    eps = 1e-6
    assert (f[:, :3] >= 0.2 - eps).all() and (f[:, :3] <= 1.8 + eps).all()
    assert (f[:, 3] >= 0.1 - eps).all() and (f[:, 3] <= 2.0 + eps).all()
    assert 0.95 < f[:, 0].mean() < 1.05 and 1.0 < f[:, 3].mean() < 1.1
    assert ((hue <= 50) | (hue >= 206)).all()                      # trunc(U(-0.2, 0.2) * 255) mod 256
    assert (hue <= 50).any() and (hue >= 206).any()
    seen = {tuple(o) for o in p.order().tolist()}
    assert seen == set(C.ORDERS)
    half = _draw(100, 224, 224, 3, s=0.5).floats
    assert (half[:, :3] >= 0.6 - eps).all() and (half[:, :3] <= 1.4 + eps).all()


def test_draw_falls_back_to_the_centre_crop():
    """H = 8, W = 256: h = sqrt(a / r) <= 8 needs a <= 64 r <= 86 pixels, below 0.08 * 2048: every try fails."""
    p = _draw(40, 8, 256, 5)
    assert (p.ints[:, 3] == 8).all() and (p.ints[:, 4] == 11).all()          # h = H, w = round(8 * 4 / 3)
    assert (p.ints[:, 1] == 0).all() and (p.ints[:, 2] == (256 - 11) // 2).all()
    tall = _draw(40, 256, 8, 5)
    assert (tall.ints[:, 4] == 8).all() and (tall.ints[:, 3] == 11).all() and (tall.ints[:, 1] == (256 - 11) // 2).all()


def test_two_view_augment_on_cpu_tiles():
    tl = C.tiles(4, 64, 64, seed=9)
    aug = simclr.TwoViewAugment(size=64, generator=torch.Generator().manual_seed(1), out="uint8")
    xis, xjs = aug(torch.from_numpy(tl))
    recs = [C.record(**dict(zip(("tile", "i", "j", "h", "w", "flags"), row[:6])), order=o, hue=row[7], brightness=f[0],
                     contrast=f[1], saturation=f[2], sigma=f[3])
            for row, o, f in zip(aug.last_params.ints.tolist(), aug.last_params.order().tolist(), aug.last_params.floats.tolist())]
    ref = C.views(tl, recs, 64)
    assert xis.shape == xjs.shape == (4, 64, 64, 3) and xis.dtype == torch.uint8
    check("TwoViewAugment xis", xis.numpy(), ref[0::2], recs[0::2], 64)
    check("TwoViewAugment xjs", xjs.numpy(), ref[1::2], recs[1::2], 64)


# ---- rejections ----------------------------------------------------------------------------------------------------------
def test_rejections():
    tl = torch.from_numpy(C.tiles(2, 40, 56, seed=1))
    ok = [C.record(tile=1, h=40, w=56)]
    assert ops.simclr_views(tl, params(ok), 20, out="uint8").shape == (1, 20, 20, 3)
    for S in (100, 16, 257):                                       # ksize 6, ksize 0, too large
        with pytest.raises(ValueError):
            ops.simclr_views(tl, params(ok), S)
    for bad in (dict(tile=2, h=40, w=56), dict(tile=-1, h=40, w=56), dict(i=1, h=40, w=56), dict(j=1, h=40, w=56),
                dict(h=0, w=56), dict(h=40, w=57), dict(i=-1, h=4, w=4)):
        with pytest.raises(ValueError):
            ops.simclr_views(tl, params([C.record(**bad)]), 20)
    with pytest.raises(ValueError):
        ops.simclr_views(torch.zeros((1, 300, 224, 3), dtype=torch.uint8), params([C.record(h=8, w=8)]), 224)
    with pytest.raises(ValueError):
        simclr.TwoViewAugment(size=100)
    from dsmil_wsi_amd import _native
    L = _native.lib()
    assert L.dsmil_simclr_views_workspace_bytes(8, 224, 224, 100) == 0 and L.dsmil_simclr_views_workspace_bytes(8, 300, 224, 224) == 0
    assert L.dsmil_simclr_views_workspace_bytes(8192, 224, 224, 224) > 0
    rec, out = params(ok).records, np.zeros((100, 100, 3), np.uint8)
    assert L.dsmil_simclr_views_host(tl.data_ptr(), 2, 40, 56, rec.data_ptr(), 1, 100, None, out.ctypes.data, None, 0) == \
        _native.DSMIL_E_UNSUPPORTED
    bad = params([C.record(tile=5, h=40, w=56)]).records           # the C entry validates too: nothing is read for it
    assert L.dsmil_simclr_views_host(tl.data_ptr(), 2, 40, 56, bad.data_ptr(), 1, 20, None, out.ctypes.data, None, 0) == \
        _native.DSMIL_E_INVALID
