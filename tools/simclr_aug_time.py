"""Times SimCLR's two-view augmentation on one GPU: simclr.TwoViewAugment (csrc/simclr_aug.hip) at S = 224 from 224 x 224 tiles
  (a) from decoded tiles on the device, 512 and 8192 views per call (256 and 4096 tiles),
  (b) from JPEG bytes through ops.jpeg_decode (host parse + copy + device decode + augmentation), wall clock,
  (c) the reference's PIL chain (the tests' Pillow oracle, tests/simclr_aug_cases.py) on ONE host thread, same parameters,
      timed beside them in the same run.
(a): hipEvents around one call (parameter draw, record upload and launch included), 5 warm-up calls, the median, minimum and
maximum of 25 timed calls, 4 distinct tile batches in rotation.  (b): wall clock with a device synchronise, 2 warm-up and 7
timed calls.  (c): wall clock over 256 views, once as a warm-up, then the median, minimum and maximum of 5 repeats.
--stages adds ops.simclr_views alone with one stage enabled at a time (2048 views per launch, hipEvents, median of 15).  Also
reported: the bytes a view moves (its crop read once, its output written once) as a fraction of the HBM roofline at the
measured rate.

    python tools/simclr_aug_time.py [--out profiles/simclr_aug/times.json] [--views 512 8192] [--output float|uint8] [--stages]
"""
import argparse
import io
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import dsmil  # noqa: E402,F401
import simclr_aug_cases as C  # noqa: E402
from dsmil_wsi_amd import ops  # noqa: E402
from dsmil_wsi_amd.simclr import TwoViewAugment, draw_view_params  # noqa: E402

HBM_BYTES_PER_S = 8.0e12      # MI355X peak


def stats(times):
    times = sorted(times)
    return {"median_ms": times[len(times) // 2], "min_ms": times[0], "max_ms": times[-1], "runs": len(times)}


def device_from_tiles(aug, batches, warmup=5, runs=25):
    times = []
    for k in range(warmup + runs):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        aug(batches[k % len(batches)])
        e1.record()
        e1.synchronize()
        if k >= warmup:
            times.append(e0.elapsed_time(e1))
    return stats(times)


def device_from_jpeg(aug, blob_batches, warmup=2, runs=7):
    times = []
    for k in range(warmup + runs):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        aug(ops.jpeg_decode(blob_batches[k % len(blob_batches)], "cuda:0"))
        torch.cuda.synchronize()
        if k >= warmup:
            times.append((time.perf_counter() - t0) * 1e3)
    return stats(times)


def stages(tiles, S, output, warmup=3, runs=15):
    """ops.simclr_views alone (no draw) on 2048 views of the 1024 tiles given, median ms per launch: the drawn mix, then every
    view with one set of flags; `full crop` takes the whole tile, so both resample passes are skipped."""
    n = tiles.shape[0]
    res = {"views": 2 * n}
    for name, flags, full in (("drawn_mix", None, False), ("resize_only", 0, False), ("full_crop_output_only", 0, True),
                              ("full_crop_flip", 1, True), ("full_crop_jitter", 2, True), ("full_crop_grey", 4, True),
                              ("full_crop_blur", 8, True)):
        p = draw_view_params(n, tiles.shape[1], tiles.shape[2], S, generator=torch.Generator().manual_seed(1))
        if flags is not None:
            p.ints[:, 5] = flags
        if full:
            p.ints[:, 1:3] = 0
            p.ints[:, 3] = tiles.shape[1]
            p.ints[:, 4] = tiles.shape[2]
        times = []
        for k in range(warmup + runs):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            ops.simclr_views(tiles, p, S, out=output)
            e1.record()
            e1.synchronize()
            if k >= warmup:
                times.append(e0.elapsed_time(e1))
        res[name] = stats(times)
        print("stage", name, json.dumps(res[name]), flush=True)
    return res


def records_of(p):
    return [C.record(**dict(zip(("tile", "i", "j", "h", "w", "flags"), row[:6])), order=o, hue=row[7], brightness=f[0],
                     contrast=f[1], saturation=f[2], sigma=f[3])
            for row, o, f in zip(p.ints.tolist(), p.order().tolist(), p.floats.tolist())]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "simclr_aug", "times.json"))
    ap.add_argument("--views", type=int, nargs="*", default=[512, 8192])
    ap.add_argument("--output", default="float", choices=["float", "uint8"])
    ap.add_argument("--pil-views", type=int, default=256)
    ap.add_argument("--pil-repeats", type=int, default=5)
    ap.add_argument("--stages", action="store_true", help="also time ops.simclr_views with one stage enabled at a time")
    args = ap.parse_args()
    S = H = W = 224
    torch.set_num_threads(1)
    base = C.tiles(64, H, W, seed=1)
    blobs = []
    for t in base:
        b = io.BytesIO()
        from PIL import Image
        Image.fromarray(t).save(b, "JPEG", quality=70)
        blobs.append(b.getvalue())
    aug = TwoViewAugment(size=S, generator=torch.Generator().manual_seed(0), out=args.output)
    out = {"device": torch.cuda.get_device_name(0), "S": S, "tile": [H, W], "output": args.output,
           "method": __doc__.split("\n\n")[0], "views": {}}

    # (c) the PIL chain, one thread: the parameters of a real draw
    pil_tiles = base[np.arange(args.pil_views // 2) % len(base)]
    aug(torch.from_numpy(pil_tiles).to("cuda:0"))
    recs = records_of(aug.last_params)
    C.views(pil_tiles, recs, S)                                                     # warm-up: the whole set once
    pil_s = []
    for _ in range(args.pil_repeats):
        t0 = time.perf_counter()
        ref = C.views(pil_tiles, recs, S)
        (torch.from_numpy(ref).permute(0, 3, 1, 2).to(torch.float32) / 255.0)   # ToTensor
        pil_s.append(time.perf_counter() - t0)
    pil_s.sort()
    med = pil_s[len(pil_s) // 2]
    out["pil_one_thread"] = {"views": len(recs), "repeats": len(pil_s), "median_s": med, "min_s": pil_s[0], "max_s": pil_s[-1],
                             "views_per_s": len(recs) / med, "views_per_s_range": [len(recs) / pil_s[-1], len(recs) / pil_s[0]]}
    print("pil", json.dumps(out["pil_one_thread"]), flush=True)
    if args.stages:
        out["stages"] = stages(torch.from_numpy(base[np.arange(1024) % len(base)]).to("cuda:0"), S, args.output)

    for n_views in args.views:
        n = n_views // 2
        idx = [np.arange(k, k + n) % len(base) for k in range(4)]
        batches = [torch.from_numpy(base[i]).to("cuda:0") for i in idx]
        res = {"from_tiles": device_from_tiles(aug, batches)}
        res["from_tiles"]["views_per_s"] = n_views / (res["from_tiles"]["median_ms"] * 1e-3)
        p = aug.last_params
        crop_bytes = float((p.ints[:, 3].long() * p.ints[:, 4].long() * 3).sum())
        out_bytes = n_views * S * S * 3 * (4 if args.output == "float" else 1)
        res["bytes_per_call"] = crop_bytes + out_bytes
        res["hbm_roofline_fraction"] = (crop_bytes + out_bytes) / (res["from_tiles"]["median_ms"] * 1e-3) / HBM_BYTES_PER_S
        blob_batches = [[blobs[j] for j in i] for i in idx]
        res["from_jpeg"] = device_from_jpeg(aug, blob_batches)
        res["from_jpeg"]["views_per_s"] = n_views / (res["from_jpeg"]["median_ms"] * 1e-3)
        res["ratio_to_pil_one_thread"] = res["from_tiles"]["views_per_s"] / out["pil_one_thread"]["views_per_s"]
        res["ratio_to_16_pil_threads"] = res["ratio_to_pil_one_thread"] / 16
        out["views"][str(n_views)] = res
        print(n_views, json.dumps(res), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
