"""The oracle and the case table of the SimCLR augmentation tests (test_simclr_aug_host.py, test_simclr_aug_gpu.py).

The oracle is the reference's chain (simclr/data_aug/dataset_wrapper.py:48-58) written out with the Pillow calls that
torchvision's PIL backend executes (F.resized_crop, F.hflip, F.adjust_*, F.to_grayscale) and, for the blur, a float64 numpy
separable convolution with a reflect-101 border: the real-arithmetic definition, not cv2's fixed-point one (OpenCV is not a
dependency of this repository).  It takes explicit records (dicts) and never touches the code under test.

Bars (see bar()): every Pillow stage, integer or float, is held to byte equality; the blur to 1 level (its real-valued result
is off by << 1, only the rounding at a boundary can differ); a chain gets the sum over its enabled stages."""
import itertools

import numpy as np
from PIL import Image, ImageEnhance, ImageStat

FLIP, JITTER, GREY, BLUR = 1, 2, 4, 8
BRIGHTNESS, CONTRAST, SATURATION, HUE = 0, 1, 2, 3


def img(rng, h, w, kind):
    """The three styles of tests/test_jpeg_gpu.py::_img: noise, ramps, blocky + noise."""
    if kind == 0:
        a = rng.integers(0, 256, (h, w, 3))
    elif kind == 1:
        yy, xx = np.mgrid[0:h, 0:w]
        a = np.stack([(xx * 3 + yy) % 256, (yy * 5) % 256, (xx ^ yy) % 256], -1)
    else:
        base = rng.integers(0, 256, (h // 8 + 2, w // 8 + 2, 3)).repeat(8, 0).repeat(8, 1)[:h, :w]
        a = np.clip(base + rng.normal(0, 12, (h, w, 3)), 0, 255)
    return a.astype(np.uint8)


def tiles(n, h, w, seed):
    rng = np.random.default_rng(seed)
    return np.stack([img(rng, h, w, k % 3) for k in range(n)])


def record(tile=0, i=0, j=0, h=1, w=1, flags=0, order=(0, 1, 2, 3), brightness=1.0, contrast=1.0, saturation=1.0, hue=0,
           sigma=1.0):
    """A record as a dict; the factors are rounded to float32, which is what a record holds."""
    return dict(tile=tile, i=i, j=j, h=h, w=w, flags=flags, order=tuple(order), brightness=float(np.float32(brightness)),
                contrast=float(np.float32(contrast)), saturation=float(np.float32(saturation)), hue=int(hue),
                sigma=float(np.float32(sigma)))


def blur_ksize(S):
    return int(0.06 * S)


# ---- the stages -----------------------------------------------------------------------------------------------------------
def crop_resize(tile, r, S):
    im = Image.fromarray(tile).crop((r["j"], r["i"], r["j"] + r["w"], r["i"] + r["h"]))
    return im.resize((S, S), Image.BILINEAR)


def contrast_mean(im):
    return int(ImageStat.Stat(im.convert("L")).mean[0] + 0.5)


def jitter_op(im, op, r):
    if op == BRIGHTNESS:
        return ImageEnhance.Brightness(im).enhance(r["brightness"])
    if op == CONTRAST:
        return ImageEnhance.Contrast(im).enhance(r["contrast"])
    if op == SATURATION:
        return ImageEnhance.Color(im).enhance(r["saturation"])
    h, s, v = im.convert("HSV").split()
    np_h = (np.array(h, dtype=np.uint8).astype(np.int32) + r["hue"]).astype(np.uint8)     # uint8 wrap-around
    return Image.merge("HSV", (Image.fromarray(np_h, "L"), s, v)).convert("RGB")


def grey(im):
    l = np.array(im.convert("L"))
    return Image.fromarray(np.stack([l, l, l], -1), "RGB")


def blur(a, sigma, k):
    """float64, separable, reflect-101, rounded to nearest at the end."""
    if k == 1:
        return a
    t = np.arange(k) - (k - 1) / 2.0
    w = np.exp(-t * t / (2.0 * sigma * sigma))
    w /= w.sum()
    x = a.astype(np.float64)
    p = k // 2
    xp = np.pad(x, ((0, 0), (p, p), (0, 0)), mode="reflect")
    x = sum(w[q] * xp[:, q:q + a.shape[1]] for q in range(k))
    xp = np.pad(x, ((p, p), (0, 0), (0, 0)), mode="reflect")
    x = sum(w[q] * xp[q:q + a.shape[0]] for q in range(k))
    return np.clip(np.rint(x), 0, 255).astype(np.uint8)


def chain(tile, r, S):
    """The view of record r from its tile, uint8 [S, S, 3]."""
    im = crop_resize(tile, r, S)
    if r["flags"] & FLIP:
        im = im.transpose(Image.FLIP_LEFT_RIGHT)
    if r["flags"] & JITTER:
        for op in r["order"]:
            im = jitter_op(im, op, r)
    if r["flags"] & GREY:
        im = grey(im)
    a = np.array(im)
    if r["flags"] & BLUR:
        a = blur(a, r["sigma"], blur_ksize(S))
    return a


def views(tile_batch, records, S):
    return np.stack([chain(tile_batch[r["tile"]], r, S) for r in records])


def bar(r, S):
    """The largest byte difference allowed on record r.  The derived bars are 0 for the integer stages, 1 per blend, 7 for the
    hue round trip and 1 for the blur; with ordered, uncontracted arithmetic the blends and the hue stage reproduce Pillow
    byte for byte (measured: no differing byte on any case here, host or device), so they are held to equality.  What is left
    is the blur: fp32 sums against this oracle's float64 ones can round a value next to .5 the other way."""
    return 1 if r["flags"] & BLUR and blur_ksize(S) > 1 else 0


# ---- the case table: (name, H, W, S, crops (i, j, h, w)) -----------------------------------------------------------------
SHAPES = [
    ("40x56_to_20", 40, 56, 20, [(0, 0, 40, 56), (3, 5, 17, 31), (39, 55, 1, 1), (10, 0, 20, 56), (0, 36, 40, 20)]),
    ("40x56_to_64", 40, 56, 64, [(0, 0, 40, 56), (7, 9, 11, 13), (2, 1, 33, 50), (0, 0, 1, 56)]),
    ("224_to_96", 224, 224, 96, [(0, 0, 224, 224), (100, 3, 96, 200)]),
    ("224_to_224", 224, 224, 224, [(5, 7, 1, 1), (0, 0, 224, 224), (0, 60, 224, 50), (120, 0, 50, 224), (17, 30, 111, 160)]),
]
SHAPE_IDS = [s[0] for s in SHAPES]
ORDERS = list(itertools.permutations(range(4)))


def crops(shape, **kw):
    """One record per crop of a shape's list, tiles dealt round-robin over three."""
    _, H, W, S, cs = shape
    return [record(tile=k % 3, i=c[0], j=c[1], h=c[2], w=c[3], **kw) for k, c in enumerate(cs)]


def full_chain_records(shape, seed):
    """48 records: the 24 jitter orders with ALL flags on (records 0..23), then the 24 orders again with everything but the
    greyscale on (24..47: the colour output of the jitter stays visible in the result).  Seeded factors inside the draw's
    intervals, over the shape's crops."""
    rng = np.random.default_rng(seed)
    _, H, W, S, cs = shape
    out = []
    for flags in (FLIP | JITTER | GREY | BLUR, FLIP | JITTER | BLUR):
        for k, order in enumerate(ORDERS):
            c = cs[(k + len(out) // 24) % len(cs)]
            out.append(record(tile=k % 3, i=c[0], j=c[1], h=c[2], w=c[3], flags=flags, order=order,
                              brightness=rng.uniform(0.2, 1.8), contrast=rng.uniform(0.2, 1.8), saturation=rng.uniform(0.2, 1.8),
                              hue=int(rng.integers(0, 256)), sigma=rng.uniform(0.1, 2.0)))
    return out


def mixed_flag_records(shape, n_tiles, seed):
    """Two views per tile that between them have every flag on and off."""
    rng = np.random.default_rng(seed)
    _, H, W, S, cs = shape
    out = []
    for k in range(2 * n_tiles):
        c = cs[k % len(cs)]
        out.append(record(tile=k // 2, i=c[0], j=c[1], h=c[2], w=c[3], flags=(k * 7 + 5) % 16, order=ORDERS[(5 * k) % 24],
                          brightness=rng.uniform(0.2, 1.8), contrast=rng.uniform(0.2, 1.8), saturation=rng.uniform(0.2, 1.8),
                          hue=int(rng.integers(0, 256)), sigma=rng.uniform(0.1, 2.0)))
    return out


def rgb_cube(step=5):
    """Every step-th level per channel as [n, 224, 224, 3] tiles (the tail is zero) and the number of colours."""
    lv = np.arange(0, 256, step)
    cube = np.stack(np.meshgrid(lv, lv, lv, indexing="ij"), -1).reshape(-1, 3).astype(np.uint8)
    n = -(-len(cube) // (224 * 224))
    buf = np.zeros((n * 224 * 224, 3), np.uint8)
    buf[:len(cube)] = cube
    return buf.reshape(n, 224, 224, 3), len(cube)
