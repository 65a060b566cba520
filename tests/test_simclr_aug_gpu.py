"""dsmil_simclr_views on the device against the Pillow oracle of simclr_aug_cases.py and against dsmil_simclr_views_host (the
same per-pixel functions compiled for the host): stages, chains, both output forms, TwoViewAugment behind ops.jpeg_decode,
determinism across launches and streams, and the edges of the input and output buffers."""
import io

import numpy as np
import pytest
import torch
from PIL import Image

import dsmil  # noqa: F401
import simclr_aug_cases as C
from dsmil_wsi_amd import ops, simclr

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def params(recs):
    g = lambda k: [r[k] for r in recs]      # noqa: E731
    f = lambda bit: [bool(r["flags"] & bit) for r in recs]      # noqa: E731
    return simclr.ViewParams(g("tile"), g("i"), g("j"), g("h"), g("w"), f(C.FLIP), f(C.JITTER), f(C.GREY), f(C.BLUR),
                             [list(r["order"]) for r in recs], g("brightness"), g("contrast"), g("saturation"), g("hue"), g("sigma"))


def records_of(p):
    return [C.record(**dict(zip(("tile", "i", "j", "h", "w", "flags"), row[:6])), order=o, hue=row[7], brightness=f[0],
                     contrast=f[1], saturation=f[2], sigma=f[3])
            for row, o, f in zip(p.ints.tolist(), p.order().tolist(), p.floats.tolist())]


def device(tile_batch, recs, S, out="uint8"):
    return ops.simclr_views(torch.from_numpy(tile_batch).to(DEV), params(recs), S, out=out).cpu().numpy()


def host(tile_batch, recs, S, out="uint8"):
    return ops.simclr_views(torch.from_numpy(tile_batch), params(recs), S, out=out).numpy()


def check(what, got, ref, recs, S):
    d = np.abs(got.astype(np.int32) - ref.astype(np.int32))
    print(f"{what}: {np.mean(d != 0):.3e} of the bytes differ, by at most {d.max()}")
    for k, r in enumerate(recs):
        assert d[k].max() <= C.bar(r, S), (what, k, r, int(d[k].max()))


@pytest.fixture(scope="module", params=C.SHAPES, ids=C.SHAPE_IDS)
def shape(request):
    name, H, W, S, _ = request.param
    return request.param, C.tiles(3, H, W, seed=len(name) + S)


def test_stages_alone(shape):
    """Every (stage, crop) pair of the host test's list, in launches of at most 48 views."""
    (name, H, W, S, cs), tl = shape
    kws = [{}, dict(flags=C.FLIP), dict(flags=C.GREY), dict(flags=C.BLUR, sigma=0.1), dict(flags=C.BLUR, sigma=1.3),
           dict(flags=C.BLUR, sigma=2.0)]
    for nm, op in (("brightness", C.BRIGHTNESS), ("contrast", C.CONTRAST), ("saturation", C.SATURATION)):
        kws += [dict(flags=C.JITTER, order=[C.HUE, op] + [o for o in range(3) if o != op], **{nm: f}) for f in (0.0, 0.2, 1.0, 1.8)]
    kws += [dict(flags=C.JITTER, hue=h) for h in (0, 1, 128, 255)]
    recs = [r for kw in kws for r in C.crops(shape[0], **kw)]      # C.crops is what the host test runs per stage
    assert len(recs) == len(kws) * len(cs)
    ref = C.views(tl, recs, S)
    for a in range(0, len(recs), 48):
        check(f"{name} stages {a}..", device(tl, recs[a:a + 48], S), ref[a:a + 48], recs[a:a + 48], S)


def test_full_chain_matches_oracle_and_host(shape):
    (name, H, W, S, _), tl = shape
    recs = C.full_chain_records(shape[0], seed=S)
    got = device(tl, recs, S)
    check(f"{name} chain", got, C.views(tl, recs, S), recs, S)
    assert np.array_equal(got, host(tl, recs, S)), "device and host disagree: a contraction or ordering difference"


def test_six_tiles_two_views_every_flag_on_and_off():
    sh = C.SHAPES[3]
    tl = C.tiles(6, 224, 224, seed=21)
    recs = C.mixed_flag_records(sh, 6, seed=22)
    assert all(any(r["flags"] & b for r in recs) and any(not r["flags"] & b for r in recs) for b in (1, 2, 4, 8))
    got = device(tl, recs, 224)
    check("6 x 2 views", got, C.views(tl, recs, 224), recs, 224)
    assert np.array_equal(got, host(tl, recs, 224))


def test_size_256_the_form_that_is_not_lds_resident():
    sh = ("256_to_256", 256, 256, 256, [(0, 0, 256, 256), (3, 9, 200, 131), (255, 255, 1, 1), (0, 100, 256, 17)])
    tl = C.tiles(3, 256, 256, seed=31)
    recs = [dict(r, flags=fl) for r, fl in zip(C.full_chain_records(sh, seed=32)[:4], (15, 11, 15, 6))]
    got = device(tl, recs, 256)
    check("S = 256", got, C.views(tl, recs, 256), recs, 256)
    assert np.array_equal(got, host(tl, recs, 256))


def test_more_views_than_workgroups_reuse_lds_tables_and_slot():
    """The grid is at most 512 persistent workgroups: with 1300 views each takes two or three, one after another, through the
    same LDS view, coefficient tables, blur weights, contrast sum and workspace slot.  Mixed flags (contrast and blur among
    them) at 40 x 56 -> 64, byte for byte against the host form; record 600 is one the kernel must refuse (workgroup 88 takes
    88, 600 and 1112: a good view, the refused one, a good view)."""
    from dsmil_wsi_amd import _native
    sh = C.SHAPES[1]
    _, H, W, S, _ = sh
    n_tiles = 650
    tl = C.tiles(n_tiles, H, W, seed=71)
    recs = C.mixed_flag_records(sh, n_tiles, seed=72)
    assert len(recs) == 1300 and any(r["flags"] & C.JITTER and r["flags"] & C.BLUR for r in recs)
    want = torch.from_numpy(host(tl, recs, S))
    want[600] = 0
    p = params(recs)
    p.ints[600, 0] = n_tiles                                     # a tile outside the batch
    L = _native.lib()
    d_tl, d_rec = torch.from_numpy(tl).to(DEV), p.records.to(DEV)
    got = torch.full((len(recs), S, S, 3), 9, dtype=torch.uint8, device=DEV)
    ws = torch.empty(L.dsmil_simclr_views_workspace_bytes(len(recs), H, W, S), dtype=torch.uint8, device=DEV)
    for _ in range(2):                                            # the second launch starts from what the first left in ws
        rc = L.dsmil_simclr_views(d_tl.data_ptr(), n_tiles, H, W, d_rec.data_ptr(), len(recs), S, None, got.data_ptr(),
                                  ws.data_ptr(), ws.numel(), torch.cuda.current_stream().cuda_stream)
        assert rc == 0
    torch.cuda.synchronize()
    diff = (got.cpu() != want).reshape(len(recs), -1).any(1).nonzero().reshape(-1).tolist()
    assert not diff, f"views that differ from the host form: {diff[:20]}"
    # and the same records, all good, through ops (fp32 planes)
    f32 = ops.simclr_views(d_tl, params(recs), S, out="float").cpu()
    assert torch.equal(f32, torch.from_numpy(host(tl, recs, S, out="float")))


def test_float_output_is_the_bytes_over_255(shape):
    (name, H, W, S, _), tl = shape
    recs = C.mixed_flag_records(shape[0], 3, seed=S + 2)
    u8 = torch.from_numpy(device(tl, recs, S))
    f32 = torch.from_numpy(device(tl, recs, S, out="float"))
    assert f32.dtype == torch.float32 and f32.shape == (len(recs), 3, S, S)
    assert torch.equal(f32, u8.permute(0, 3, 1, 2).to(torch.float32) / 255.0)


def _jpeg(a, **kw):
    b = io.BytesIO()
    Image.fromarray(a).save(b, "JPEG", **kw)
    return b.getvalue()


def test_two_view_augment_behind_jpeg_decode():
    blobs = [_jpeg(t, quality=70) for t in C.tiles(8, 224, 224, seed=41)]
    decoded = ops.jpeg_decode(blobs, DEV)
    tl = decoded.cpu().numpy()
    for out, shp, dt in (("float", (8, 3, 224, 224), torch.float32), ("uint8", (8, 224, 224, 3), torch.uint8)):
        aug = simclr.TwoViewAugment(size=224, generator=torch.Generator().manual_seed(42), out=out)
        xis, xjs = aug(decoded)
        assert xis.shape == xjs.shape == shp and xis.dtype == xjs.dtype == dt and xis.device == decoded.device
        assert xis.data_ptr() != xjs.data_ptr() and xis._base is xjs._base          # views of one output
        recs = records_of(aug.last_params)
        assert [r["tile"] for r in recs] == [k // 2 for k in range(16)]
        ref = C.views(tl, recs, 224)
        xis, xjs = xis.cpu(), xjs.cpu()
        if out == "float":       # back to the bytes, on the host: byte / 255 * 255 is within 1e-4 of the byte
            xis, xjs = (torch.round(x * 255.0).to(torch.uint8).permute(0, 2, 3, 1) for x in (xis, xjs))
        check(f"TwoViewAugment {out} xis", xis.numpy(), ref[0::2], recs[0::2], 224)
        check(f"TwoViewAugment {out} xjs", xjs.numpy(), ref[1::2], recs[1::2], 224)


def test_deterministic_across_launches_and_streams():
    sh = C.SHAPES[3]
    tl = torch.from_numpy(C.tiles(6, 224, 224, seed=51)).to(DEV)
    p = params(C.mixed_flag_records(sh, 6, seed=52))
    a = ops.simclr_views(tl, p, 224, out="uint8")
    b = ops.simclr_views(tl, p, 224, out="uint8")
    pool = ops.StreamPool(2)
    c = pool.run(ops.simclr_views, tl, p, 224, out="uint8")
    d = pool.run(ops.simclr_views, tl, p, 224, out="uint8")
    pool.join()
    torch.cuda.synchronize()
    assert torch.equal(a, b) and torch.equal(a, c) and torch.equal(a, d)


def test_edges_of_the_input_and_output_buffers():
    """The last tile's bottom-right corner, with the tiles flush against a sentinel region that must stay as it is, and the
    output's neighbours in an over-allocated buffer untouched."""
    H = W = 224
    S = 96
    n_in = 2 * H * W * 3
    big = torch.full((n_in + 4096,), 0xA5, dtype=torch.uint8, device=DEV)
    tl_np = C.tiles(2, H, W, seed=61)
    big[:n_in] = torch.from_numpy(tl_np).reshape(-1).to(DEV)
    tl = big[:n_in].view(2, H, W, 3)
    recs = [C.record(tile=1, i=H - 1, j=W - 1, h=1, w=1), C.record(tile=1, i=H - 50, j=W - 96, h=50, w=96, flags=C.BLUR, sigma=1.0),
            C.record(tile=1, i=0, j=0, h=H, w=W, flags=15, hue=77, contrast=1.5, order=(3, 1, 0, 2))]
    got = ops.simclr_views(tl, params(recs), S, out="uint8")
    check("corner", got.cpu().numpy(), C.views(tl_np, recs, S), recs, S)
    assert (big[n_in:] == 0xA5).all() and torch.equal(big[:n_in].cpu(), torch.from_numpy(tl_np).reshape(-1))
    # the C entry with an output placed inside a larger buffer
    from dsmil_wsi_amd import _native
    L = _native.lib()
    n_out = len(recs) * S * S * 3
    for dtype, fill in ((torch.uint8, 0x5A), (torch.float32, -7.0)):
        buf = torch.full((n_out + 2048,), fill, dtype=dtype, device=DEV)
        mid = buf[1024:1024 + n_out]
        d_rec = params(recs).records.to(DEV)
        ws = torch.empty(L.dsmil_simclr_views_workspace_bytes(len(recs), H, W, S), dtype=torch.uint8, device=DEV)
        of, ou = (mid.data_ptr(), None) if dtype == torch.float32 else (None, mid.data_ptr())
        rc = L.dsmil_simclr_views(tl.data_ptr(), 2, H, W, d_rec.data_ptr(), len(recs), S, of, ou, ws.data_ptr(), ws.numel(),
                                  torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        assert rc == 0
        assert (buf[:1024] == fill).all() and (buf[1024 + n_out:] == fill).all()
        # (the quotient on the host: torch's device kernels divide by a scalar with a reciprocal multiply)
        want = got.cpu().reshape(-1) if dtype == torch.uint8 else (got.cpu().permute(0, 3, 1, 2).to(torch.float32) / 255.0).reshape(-1)
        assert torch.equal(mid.cpu(), want)
    # a record the host validation would refuse reads nothing and yields zeros
    bad = params([C.record(tile=2, h=H, w=W), C.record(tile=1, i=H - 10, j=0, h=11, w=5)]).records.to(DEV)
    out = torch.full((2 * S * S * 3,), 9, dtype=torch.uint8, device=DEV)
    rc = L.dsmil_simclr_views(tl.data_ptr(), 2, H, W, bad.data_ptr(), 2, S, None, out.data_ptr(), ws.data_ptr(), ws.numel(),
                              torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert rc == 0 and (out == 0).all()
