"""Shapes, seeded inputs, fp64 references and bars of the STAGES of the fp32-class embedder trunk (csrc/resnet_fwd.hip and
csrc/wino_w1.h behind the dsmil_trunk32_* entries), shared by tests/test_trunk32_host.py (the bars are reachable by the
reference arithmetic and see the mutants), tests/test_trunk32_cabi.py (the plan of every case is pinned) and
tests/test_trunk32_gpu.py (the kernels meet them).  Nothing here is tuned on a GPU or taken from the code under test.

u = 2^-24 is half a unit in the last place of fp32, relative to the value.  All roundings are to nearest even.  "1.01" pays for
the second-order terms (n u)^2 of every linear bound below (n u < 2^-9 in every case here).

Operand model, precision "fp32" (NPD = 3).  A conv operand a (fp32) is cut into two fp16 planes h0 = rne16(a), h1 = rne16(a -
h0).  a - h0 is exact in fp32, at most half a unit of h0's 11 bits (|h1| <= 2^-11 |a|), and a multiple of a's last place: it has
at most 12 significant bits where |a - h0| >= 2^-12 2^e (a in [2^e, 2^(e+1))), so rne16 loses at most its last bit:
    |a - (h0 + h1)| <= 2^-23 |a|  = 2 u |a|      while h1 is a normal fp16 value, and <= 2^-25 absolutely below that
(fp16's subnormal spacing is 2^-24; gfx950's conversions and f16 MFMA keep subnormals).  This is TWICE the "2^-24" the comments of
resnet_fwd.hip quote: a = 1 + 2^-11 + 2^-23 gives h0 = 1 + 2^-10, a - h0 = -(2^-11 - 2^-23), h1 = -2^-11, error 2^-23.  Weights are
multiplied by 2^8 before the cut (exact) and the accumulators by 2^-8 behind the K loop (exact): relative 2 u, floor 2^-33.
The three kept products h0 w0, h0 w1, h1 w0 have at most 22 significant bits: exact in fp32.  The dropped h1 w1 is at most
2^-22 |a w| = 4 u |a w| (again above the quoted 2^-24, which is its typical size).  So one product is off by at most
(2 + 2 + 4) u |a w| = 8 u |a w| before any addition.

Direct convs (k_conv_s6), K = Cin ks^2, S = sum |x| |w| over the taps of an output.  The 3 K plane products are added to the fp32
accumulator by MFMAs whose internal order is not documented: any order of at most 3 K roundings, each at most u times a partial
sum that never exceeds (1 + 2^-10) S, gives 3 K u S.  With the operand error:
    |got - s| <= 1.01 (3 K + 8) u S + floor,        floor = 2^-25 sum_{x != 0} |w| + 2^-33 sum_{w != 0} |x|
    precision "half" (one plane: a^ = rne16(a), |a - a^| <= 2^-11 |a|):
    |got - s| <= 1.01 ((2 2^-11 + 2^-22) S + K u S) + floor
NORM input.  The kernel stages v = max((x - m) r, 0) in fp32: one rounding in the subtraction, one in the product, the sign is
kept, so |v^ - v| <= 2.01 u v, taken as 3 u v: the operand constant 8 becomes 11 (and "half" gains 3 u S).  The reference is
fp64 relu((x - m) r) of the given fp32 m, r.

Winograd convs (k_conv_wino_s3, k_conv_wino_w1), F(2x2, 3x3): Y = A^T [ sum_c (G g G^T) .* (B^T d B) ] A.
    V = B^T d B in fp32 before the cut: two levels of additions of four inputs, 2.01 u |B^T| |d| |B|   (3 more with NORM)
    U = G g G^T in fp32 at pack time: four levels (the halvings are exact), 4.04 u |G| |g| |G^T|
    cuts 2 u each, dropped h1 w1 4 u, 3 Cin roundings in the accumulation over the channels of one transform position,
    the inverse transform: nine accumulators through at most four levels of additions, 4.04 u
All of it scales with the transform-domain magnitudes, so the bar is formed by the same algebra in fp64 on absolute values,
    T = |A^T| [ sum_c (|G| |g| |G^T|) .* (|B^T| |d| |B|) ] |A|          (not from S)
    |got - s| <= 1.01 (3 Cin + 16) u T + floor   (+ 3 u T with NORM);   "half": 1.01 ((2 2^-11 + 2^-22) T + (Cin + 10) u T) + floor
    floor = 2^-25 |A^T| [sum_c |G||g||G^T|] |A| + 2^-33 |A^T| [sum_c |B^T||d||B|] |A|.

Statistics (k_in_finalize_flat / _cnt / _stem behind the conv epilogues), per (image, channel) over n pixels of the computed
output y^ = y + delta, |delta| <= bar_y.  A partial holds (cnt_t, mean_t, M2_t about mean_t) of at most cmax values (32 rows of a
direct or stem tile, 64 of a Winograd unit's output row); P partials are merged: mean = sum cnt_t mean_t / n, M2 = sum (M2_t +
cnt_t (mean_t - mean)^2).  Every value passes through at most N = min(n, cmax) + P + 12 rounded operations on either route.
    e    = 1.01 (cmax + 1) u max |y^|                         (any partial's mean against its exact mean)
    dm_a = 1.01 N u mean |y^| + u |m|                         (the merged mean against the exact mean of y^)
    dm   = dm_a + mean(bar_y)
    The identity  sum_i (y_i - mu)^2 = sum_t [ sum_i (y_i - c_t)^2 - cnt_t (c_t - m_t)^2 + cnt_t (m_t - mu)^2 ]  with the kernels'
    c_t = mean_t^ and (mean_t^ - mean^)^2 in place of (m_t - mu)^2, and sum_t cnt_t |m_t - mu| / n <= sqrt(v) (Cauchy-Schwarz):
    ds   = sqrt(mean(bar_y^2)),  sv = sqrt(v) + ds                   (the spread of y^ is at most sv)
    X    = e^2 + (e + dm_a)(2 sv + e + dm_a)
    dv   = 1.01 N u (sv^2 + X) + X + ds (2 sqrt(v) + ds)              (roundings of the positive sum; centres; y^ against y)
    dr   = 1/2 r_hi^3 dv + 8 u r_hi,    r_hi = 1 / sqrt(max(v - dv, 0) + 1e-5)
(r is decreasing and convex in v; 8 u: the division by n, the addition of eps, a square root and a division, with room, as in
trunk16_cases.)  mean / rstd are compared with the fp64 mean and 1 / sqrt(var + 1e-5) of the fp64 conv output.  A channel with
all-zero weights has y^ = 0 exactly: mean 0 and rstd = fp32(1 / sqrt(fp32(1e-5))) within 8 u.

Stem (k_stem_s6 and its pool).  A direct conv with K = 147 (the zero padding of K to 176 adds exact zeros); uint8 input is
divided by 255 in fp32 first (one more rounding: 8 -> 9 u).  pooled = relu((max - m^) r^) of the kernel's OWN statistics:
    dt  = r_hi (max_window bar_y + dm) + |ymax - m| dr + 3 u |t|,   bar = 1.01 (dt + 2 u |ref|)
frozen statistics are exact inputs: dt = |r| max_window bar_y + 3 u |t|, and r < 0 takes the window MINIMUM.

Tail (k_norm_add_relu, k_norm_add_relu_pool): out = relu((y - m) r + idn') in fp32, idn' = idn or (idn - md) rd; subtraction,
product, addition (or one fma), the downsample's two roundings on idn':
    bar = 4.04 u (|t| + |idn'|);     pool: mean(bar) + 1.01 n u mean |val| + u |ref|    (n sequential additions, one division).

EXACT cases.  x in multiples of 2^-k, w in {-1, 0, 1} 2^-j: U = G g G^T is a multiple of 2^-(j+2) with at most 10 bits, V a sum
of four x; every plane product and — checked by exact_margin() on the case's own data — every partial sum in any order is an
integer below 2^24 in units of the smallest product: fp32 holds them exactly, so the output equals the fp64 result bit for bit.
"x wide": x has 12 significant bits, w at most 11: h1 != 0, w1 = 0, exact only if h1 w0 is kept.  "w wide": the mirror, 2^8 w
has 12 or more bits: exact only if h0 w1 is kept."""
import functools

import numpy as np
import torch
import torch.nn.functional as F

PRECISIONS = ("fp32", "half")
U32 = 2.0 ** -24
EPS = 1e-5
RSTD0 = float(np.float32(1.0) / np.sqrt(np.float32(1e-5)))          # rstd of a constant channel
ZERO_CH, SHIFT_CH = 3, 5        # output channel with all-zero weights; output channel whose mean is ~40 times its spread
SHIFT_LEVEL = 8.0

BT = np.array([[1, 0, -1, 0], [0, 1, 1, 0], [0, -1, 1, 0], [0, 1, 0, -1]], np.float64)
G = np.array([[1, 0, 0], [.5, .5, .5], [.5, -.5, .5], [0, 0, 1]], np.float64)
AT = np.array([[1, 1, 1, 0], [0, 1, -1, -1]], np.float64)


def out_size(n, ks, stride, pad):
    return (n + 2 * pad - ks) // stride + 1


# ---- case tables ------------------------------------------------------------------------------------------------------------
# Direct convs: (name, B, H, W, Cin, Cout, ks, stride, pad, norm) -> expected plan (tile, Ho, Wo, nslots, grid_x, grid_y).
# nslots = 31 // (Ho Wo) + 2: the images a 32-pixel tile can touch.
DIRECT_CASES = [
    ("d42_1x1_5x7", 3, 5, 7, 64, 64, 1, 1, 0, False),        # 105 pixels: one partial 128-pixel workgroup, HW = 35
    ("d42_1x1_9x7", 5, 9, 7, 64, 64, 1, 1, 0, True),         # HW = 63: a tile touches 2 images; 315 pixels: three workgroups
    ("d42_bneck", 3, 3, 4, 256, 64, 1, 1, 0, True),          # the Bottleneck width 256 -> 64; HW = 12: a tile touches 3-4 images
    ("d42_hw2", 33, 1, 2, 64, 64, 1, 1, 0, False),           # HW = 2: 16 images per tile, 17 slots
    ("d42_hw1", 37, 1, 1, 64, 64, 1, 1, 0, True),            # HW = 1: 32 images per tile, 33 slots, a partial second tile
    ("d22_ds_7x5", 3, 7, 5, 64, 128, 1, 2, 0, False),        # the downsample: 7 x 5 -> 4 x 3
    ("d22_s2_7x5", 3, 7, 5, 64, 128, 3, 2, 1, True),         # 3x3 / 2 on an odd map: 7 x 5 -> 4 x 3
    ("d22_s2_8x6", 2, 8, 6, 64, 128, 3, 2, 1, False),        # ... on an even map
    ("d22_slots33", 40, 2, 2, 64, 128, 3, 2, 1, True),       # 2 x 2 -> 1 x 1, B = 40: nslots = 33
    ("d24_s2_7x5", 5, 7, 5, 128, 256, 3, 2, 1, True),        # 60 pixels: one partial 64-pixel workgroup
    ("d24_1x1_9x7", 3, 9, 7, 64, 256, 1, 1, 0, False),       # 189 pixels: three workgroups, the last partial
    ("d24_ds_8x6", 2, 8, 6, 128, 256, 1, 2, 0, True),
]
DIRECT_PLANS = {   # name: (tile, Ho, Wo, nslots, grid_x, grid_y)
    "d42_1x1_5x7": (42, 5, 7, 2, 1, 1), "d42_1x1_9x7": (42, 9, 7, 2, 3, 1), "d42_bneck": (42, 3, 4, 4, 1, 1),
    "d42_hw2": (42, 1, 2, 17, 1, 1), "d42_hw1": (42, 1, 1, 33, 1, 1), "d22_ds_7x5": (22, 4, 3, 4, 1, 1),
    "d22_s2_7x5": (22, 4, 3, 4, 1, 1), "d22_s2_8x6": (22, 4, 3, 4, 1, 1), "d22_slots33": (22, 1, 1, 33, 1, 1),
    "d24_s2_7x5": (24, 4, 3, 4, 1, 1), "d24_1x1_9x7": (24, 9, 7, 2, 3, 1), "d24_ds_8x6": (24, 4, 3, 4, 1, 1),
}
# Winograd convs (3x3 / 1 / pad 1): (name, B, H, W, Cin, Cout, norm) -> expected plan (kernel, IB, TYB, TXB, nby, nbx, grid_x, grid_y)
WINO_CASES = [
    ("u_1x1", 3, 1, 1, 64, 64, False),           # one half-covered tile per image, three images per unit
    ("u_2x2", 3, 2, 2, 64, 64, True),
    ("u_3x3", 2, 3, 3, 64, 64, False),           # odd both ways
    ("u_5x7", 3, 5, 7, 64, 64, True),            # odd both ways; IB = 2 with B = 3: a unit with a missing image
    ("u_4x4_b5", 5, 4, 4, 64, 64, False),        # IB = 5
    ("u_2x2_b40", 40, 2, 2, 64, 64, True),       # IB = 14: three units, the last with 12 images
    ("u192_5x7", 3, 5, 7, 64, 192, False),       # Cout % 64 == 0, % 128 != 0: three cout blocks of k_conv_wino_s3
    ("u_2x61", 2, 2, 61, 64, 64, False),         # TXB = 31: the raw region is 4 x 64 = WRAW_MAX pixels exactly
    ("u_2x63", 1, 2, 63, 64, 64, True),          # the narrowest map with nbx > 1: TXB = 32 would need 4 x 66 > WRAW_MAX raw pixels
    ("u_63x2", 1, 63, 2, 64, 64, False),         # the shortest map with nby > 1; the last unit row holds one half-covered tile row
    ("w_1x1", 3, 1, 1, 64, 128, False),
    ("w_5x7", 3, 5, 7, 64, 128, True),
    ("w128_4x4_b5", 5, 4, 4, 128, 128, False),
    ("w32_3x3", 2, 3, 3, 32, 128, True),         # cin < 64: the unit of the non-"rounds" choice, IB = 2
    ("w32_4x4_b5", 5, 4, 4, 32, 128, False),     # ... IB = 5
    ("w_2x63", 2, 2, 63, 64, 128, True),
    ("w_63x2", 1, 63, 2, 64, 128, False),
    ("w256_14_g8", 2, 14, 14, 64, 256, True),    # grid 8: the (L & 7) block-to-cout map of wino_w1.h
    ("w256_5x7_g6", 3, 5, 7, 64, 256, False),    # grid 6: the plain map
]
WINO_PLANS = {
    "u_1x1": ("unit", 3, 1, 1, 1, 1, 1, 1), "u_2x2": ("unit", 3, 1, 1, 1, 1, 1, 1), "u_3x3": ("unit", 2, 2, 2, 1, 1, 1, 1),
    "u_5x7": ("unit", 2, 3, 4, 1, 1, 2, 1), "u_4x4_b5": ("unit", 5, 2, 2, 1, 1, 1, 1), "u_2x2_b40": ("unit", 14, 1, 1, 1, 1, 3, 1),
    "u192_5x7": ("unit", 2, 3, 4, 1, 1, 2, 3), "u_2x61": ("unit", 1, 1, 31, 1, 1, 2, 1), "u_2x63": ("unit", 1, 1, 16, 1, 2, 2, 1),
    "u_63x2": ("unit", 1, 31, 1, 2, 1, 2, 1), "w_1x1": ("w1", 1, 1, 1, 1, 1, 3, 1), "w_5x7": ("w1", 1, 3, 4, 1, 1, 3, 1),
    "w128_4x4_b5": ("w1", 1, 2, 2, 1, 1, 5, 1), "w32_3x3": ("w1", 2, 2, 2, 1, 1, 1, 1), "w32_4x4_b5": ("w1", 5, 2, 2, 1, 1, 1, 1),
    "w_2x63": ("w1", 1, 1, 16, 1, 2, 4, 1), "w_63x2": ("w1", 1, 31, 1, 2, 1, 2, 1), "w256_14_g8": ("w1", 1, 7, 4, 1, 2, 8, 1),
    "w256_5x7_g6": ("w1", 1, 3, 4, 1, 1, 6, 1),
}
# exact cases: (name, B, H, W, Cin, Cout, ks, stride, pad, flavour); flavour "plain", "xwide" (h1 w0) or "wwide" (h0 w1)
EXACT_CASES = [
    ("x42", 3, 5, 7, 64, 64, 1, 1, 0, "plain"), ("x22", 3, 7, 5, 64, 128, 3, 2, 1, "plain"), ("x24", 3, 7, 5, 64, 256, 1, 2, 0, "plain"),
    ("x42_xwide", 3, 5, 7, 32, 64, 1, 1, 0, "xwide"), ("x22_wwide", 3, 7, 5, 32, 128, 3, 2, 1, "wwide"),
    ("xu", 3, 5, 7, 64, 64, 3, 1, 1, "plain"), ("xw", 3, 5, 7, 64, 128, 3, 1, 1, "plain"),
    ("xu_xwide", 3, 5, 7, 16, 64, 3, 1, 1, "xwide"), ("xw_xwide", 3, 5, 7, 16, 128, 3, 1, 1, "xwide"),
    ("xu_wwide", 3, 5, 7, 16, 64, 3, 1, 1, "wwide"), ("xw_wwide", 3, 5, 7, 16, 128, 3, 1, 1, "wwide"),
]
# stem: (name, B, H, W, u8, frozen)
STEM_CASES = [
    ("s32_f", 1, 32, 32, False, False),          # one tile row
    ("s34x38_u8", 3, 34, 38, True, False),       # H1 = 17: a second tile row of one conv row; the pool row it feeds comes from the halo
    ("s34x38_f_bn", 3, 34, 38, False, True),
    ("s65x33_f", 1, 65, 33, False, False),
    ("s65x33_u8_bn", 3, 65, 33, True, True),
    ("s96x80_u8", 1, 96, 80, True, False),       # Hp = 24: halo rows at py = 8 and 16
    ("s96x80_f", 3, 96, 80, False, False),
]
STEM_EXACT = [("sx_plain", 2, 34, 38, "plain"), ("sx_xwide", 1, 34, 38, "xwide"), ("sx_wwide", 1, 65, 33, "wwide")]
# tail: (name, kind, B, HW, C).  k_norm_add_relu: 256 / min(C / 4, 256) pixels per workgroup, at most 8192 workgroups
TAIL_CASES = [
    ("t64_id", "identity", 7, 12, 64), ("t64_down", "down", 7, 12, 64), ("t64_pool", "pool", 7, 12, 64),
    ("t64_hw1", "identity", 37, 1, 64), ("t512_down", "down", 5, 12, 512), ("t512_id_hw1", "identity", 5, 1, 512),
    ("t512_pool", "pool", 5, 12, 512), ("t2048_id", "identity", 3, 12, 2048), ("t2048_down_hw1", "down", 3, 1, 2048),
    ("t2048_pool", "pool", 3, 1, 2048),
    ("t64_cap", "identity", 5, 168 * 168, 64),   # 141120 pixels > 8192 x 16: the grid-stride branch, images of different statistics
    ("t64_cap_down", "down", 5, 168 * 168, 64),
]
BY_NAME = {c[0]: c for c in DIRECT_CASES + WINO_CASES + EXACT_CASES + STEM_CASES + STEM_EXACT + TAIL_CASES}


def _seed(name):
    return 3200 + sum((i + 1) * ord(ch) for i, ch in enumerate(name))


# ---- fp64 references --------------------------------------------------------------------------------------------------------
def conv64(x, w, stride, pad):
    return F.conv2d(torch.from_numpy(np.asarray(x, np.float64)), torch.from_numpy(np.asarray(w, np.float64)), stride=stride, padding=pad).numpy()


def staged64(x, in_stats):
    """What the conv multiplies: x, or relu((x - m) r) of the given fp32 statistics [B, Cin], in fp64."""
    x = np.asarray(x, np.float64)
    if in_stats is None:
        return x
    m, r = (np.asarray(t, np.float64)[:, :, None, None] for t in in_stats)
    return np.maximum((x - m) * r, 0.0)


def wino_tiles(x):
    """NCHW [B,C,H,W] -> the 4x4 input patches of the 2x2 output tiles, [B, TY, TX, 4, 4, C] (zero padded)."""
    B, C, H, W = x.shape
    TY, TX = (H + 1) // 2, (W + 1) // 2
    xp = np.zeros((B, C, 2 * TY + 2, 2 * TX + 2), x.dtype)
    xp[:, :, 1:H + 1, 1:W + 1] = x
    d = np.empty((B, TY, TX, 4, 4, C), x.dtype)
    for i in range(4):
        for j in range(4):
            d[:, :, :, i, j, :] = xp[:, :, i:i + 2 * TY:2, j:j + 2 * TX:2].transpose(0, 2, 3, 1)
    return d


def wino_untile(y, H, W):
    """[B, TY, TX, 2, 2, Cout] -> NCHW [B, Cout, H, W] (the out-of-map half of an odd map's last tiles is dropped)."""
    B, TY, TX, _, _, Co = y.shape
    return np.ascontiguousarray(y.transpose(0, 5, 1, 3, 2, 4).reshape(B, Co, 2 * TY, 2 * TX)[:, :, :H, :W])


def wino_abs(xs, w):
    """T = |A^T| [sum_c (|G||g||G^T|) .* (|B^T||d||B|)] |A| and the two floor sums, fp64 NCHW."""
    B, C, H, W = xs.shape
    d = wino_tiles(np.abs(np.asarray(xs, np.float64)))
    Va = np.einsum("ik,btxklc,jl->btxijc", np.abs(BT), d, np.abs(BT))
    Ua = np.einsum("ik,ockl,jl->ocij", np.abs(G), np.abs(np.asarray(w, np.float64)), np.abs(G))
    inv = lambda M: wino_untile(np.einsum("ik,btxklo,jl->btxijo", np.abs(AT), M, np.abs(AT)), H, W)
    T = inv(np.einsum("btxijc,ocij->btxijo", Va, Ua))
    fl = 2.0 ** -25 * inv(np.broadcast_to(Ua.sum(1).transpose(1, 2, 0), Va.shape[:3] + (4, 4, w.shape[0]))) + \
         2.0 ** -33 * inv(np.broadcast_to(Va.sum(-1, keepdims=True), Va.shape[:5] + (w.shape[0],)))
    return T, fl


def conv_reference(x, w, stride, pad, in_stats, precision, wino):
    """(s, bar): the fp64 conv of the staged input and the module docstring's bar, NCHW [B, Cout, Ho, Wo]."""
    xs = staged64(x, in_stats)
    s = conv64(xs, w, stride, pad)
    Cin, ks = w.shape[1], w.shape[2]
    nrm = 3 if in_stats is not None else 0
    if wino:
        T, floor = wino_abs(xs, w)
        if precision == "fp32":
            return s, 1.01 * (3 * Cin + 16 + nrm) * U32 * T + floor
        return s, 1.01 * ((2 * 2.0 ** -11 + 2.0 ** -22) * T + (Cin + 10 + nrm) * U32 * T) + floor
    K = Cin * ks * ks
    aw = np.abs(np.asarray(w, np.float64))
    S = conv64(np.abs(xs), aw, stride, pad)
    floor = 2.0 ** -25 * conv64((xs != 0).astype(np.float64), aw, stride, pad) + 2.0 ** -33 * conv64(np.abs(xs), (aw != 0).astype(np.float64), stride, pad)
    if precision == "fp32":
        return s, 1.01 * (3 * K + 8 + nrm) * U32 * S + floor
    return s, 1.01 * ((2 * 2.0 ** -11 + 2.0 ** -22) * S + (K + nrm) * U32 * S) + floor


def stats_reference(s, bar, cmax, P):
    """(m, r, dm, dr, r_hi) per (image, channel) [B, C] of the fp64 conv output s with elementwise bar (module docstring)."""
    B, C = s.shape[:2]
    y = s.reshape(B, C, -1)
    b = bar.reshape(B, C, -1)
    n = y.shape[2]
    m = y.mean(2)
    v = ((y - m[:, :, None]) ** 2).mean(2)
    ymax = (np.abs(y) + b).max(2)
    ybar = (np.abs(y) + b).mean(2)
    N = min(n, cmax) + P + 12
    e = 1.01 * (cmax + 1) * U32 * ymax
    dm_a = 1.01 * N * U32 * ybar + U32 * np.abs(m)
    dm = dm_a + b.mean(2)
    ds = np.sqrt((b * b).mean(2))
    sv = np.sqrt(v) + ds
    cross = e * e + (e + dm_a) * (2 * sv + e + dm_a)
    dv = 1.01 * N * U32 * (sv * sv + cross) + cross + ds * (2 * np.sqrt(v) + ds)
    r = 1.0 / np.sqrt(v + EPS)
    r_hi = 1.0 / np.sqrt(np.maximum(v - dv, 0.0) + EPS)
    return m, r, dm, 0.5 * r_hi ** 3 * dv + 8 * U32 * r_hi, r_hi


# ---- inputs -----------------------------------------------------------------------------------------------------------------
def relu_map(rng, B, C, H, W):
    return np.maximum(rng.standard_normal((B, C, H, W)), 0).astype(np.float32)


def conv_weights(rng, cout, cin, ks):
    """fp32 OIHW at kaiming-normal(fan_out) scale, with the two degenerate output channels: ZERO_CH all zero; SHIFT_CH reads
    SHIFT_LEVEL from the constant input channel 0 through its centre tap beside weights of a fifth the scale."""
    w = (rng.standard_normal((cout, cin, ks, ks)) * (2.0 / (cout * ks * ks)) ** 0.5).astype(np.float32)
    w[ZERO_CH] = 0
    w[SHIFT_CH] *= np.float32(0.2)
    w[SHIFT_CH, 0, ks // 2, ks // 2] = 1.0
    return w


@functools.lru_cache(maxsize=None)
def conv_case(name):
    """(x NCHW fp32, w OIHW fp32, in_stats or None, stride, pad, wino) of a DIRECT_CASES / WINO_CASES entry.  With norm, x is a
    raw map (zero-mean, O(1)) and in_stats = (m, r) [B, Cin] are seeded values, not x's statistics: the test controls them.
    Channel 0 of the staged input is the constant SHIFT_LEVEL."""
    c = BY_NAME[name]
    if len(c) == 7:
        _, B, H, W, Cin, Cout, norm = c
        ks, stride, pad, wino = 3, 1, 1, True
    else:
        _, B, H, W, Cin, Cout, ks, stride, pad, norm = c
        wino = False
    rng = np.random.default_rng(_seed(name))
    w = conv_weights(rng, Cout, Cin, ks)
    if not norm:
        x = relu_map(rng, B, Cin, H, W)
        x[:, 0] = SHIFT_LEVEL
        return x, w, None, stride, pad, wino
    x = (rng.standard_normal((B, Cin, H, W)) * 1.5).astype(np.float32)
    m = (rng.standard_normal((B, Cin)) * 0.3).astype(np.float32)
    r = rng.uniform(0.5, 2.0, (B, Cin)).astype(np.float32)
    m[:, 0], r[:, 0] = 0.0, 1.0
    x[:, 0] = SHIFT_LEVEL
    return x, w, (m, r), stride, pad, wino


@functools.lru_cache(maxsize=None)
def conv_expected(name, precision):
    """(s, bar, (m, r, dm, dr)) of a bar case, computed once."""
    x, w, st, stride, pad, wino = conv_case(name)
    s, bar = conv_reference(x, w, stride, pad, st, precision, wino)
    if wino:
        cmax, P = 64, 2 * WINO_PLANS[name][4] * WINO_PLANS[name][5]
    else:
        cmax, P = 32, (s.shape[2] * s.shape[3] + 31) // 32 + 1
    return s, bar, stats_reference(s, bar, cmax, P)[:4]


def _exact_xw(rng, flavour, B, Cin, H, W, Cout, ks):
    """plain: x in {0..3}, w in {-1, 0, 1} 2^-j.  xwide: x = n 2^-8, n < 2^12 (12 bits: h1 != 0).  wwide: 2^8 w = n 2^-4 with
    |n| < 2^12 (12 bits: w1 != 0), x in {0..3}.  Half of x and half of w are zero, as behind a ReLU / to bound the sums."""
    if flavour == "xwide":
        x = rng.integers(2 ** 11, 2 ** 12, (B, Cin, H, W)) * 2.0 ** -8
    else:
        x = rng.integers(1, 4, (B, Cin, H, W)).astype(np.float64)
    x = np.where(rng.random(x.shape) < 0.5, 0.0, x).astype(np.float32)
    if flavour == "wwide":
        w = rng.integers(2 ** 11, 2 ** 12, (Cout, Cin, ks, ks)) * 2.0 ** -12 * rng.choice([-1.0, 1.0], (Cout, Cin, ks, ks))
    else:
        w = rng.choice([-1.0, 1.0], (Cout, Cin, ks, ks)) * 2.0 ** -(np.arange(Cout) % 3)[:, None, None, None]
    w = np.where(rng.random(w.shape) < 0.5, 0.0, w).astype(np.float32)
    return x, w


def exact_margin(xs, w, stride, pad, wino, flavour):
    """Largest sum of |plane products| behind any output, in units of the smallest product's last place: below 2^24 every
    partial sum in any order is an exact fp32 value.  (|h0| + |h1| <= (1 + 2^-10) |a|: the factor 1.01.)"""
    xs, w = np.asarray(xs, np.float64), np.asarray(w, np.float64)
    unit = (2.0 ** -8 if flavour == "xwide" else 1.0) * (2.0 ** -12 if flavour == "wwide" else 2.0 ** -2)
    if wino:
        V = np.einsum("ik,btxklc,jl->btxijc", BT, wino_tiles(xs), BT)
        U = np.einsum("ik,ockl,jl->ocij", G, w, G)
        M = np.einsum("btxijc,ocij->btxijo", np.abs(V), np.abs(U))
        return 1.01 * np.einsum("ik,btxklo,jl->btxijo", np.abs(AT), M, np.abs(AT)).max() / (unit / 4)    # U: quarters of w's unit
    return 1.01 * conv64(np.abs(xs), np.abs(w), stride, pad).max() / unit


@functools.lru_cache(maxsize=None)
def exact_case(name):
    """(x, w, stride, pad, wino, s fp64 == its fp32 value) of an EXACT_CASES entry."""
    _, B, H, W, Cin, Cout, ks, stride, pad, flavour = BY_NAME[name]
    rng = np.random.default_rng(_seed(name))
    x, w = _exact_xw(rng, flavour, B, Cin, H, W, Cout, ks)
    wino = ks == 3 and stride == 1
    assert exact_margin(x, w, stride, pad, wino, flavour) < 2.0 ** 24, name
    s = conv64(x, w, stride, pad)
    assert np.array_equal(s.astype(np.float32).astype(np.float64), s)
    return x, w, stride, pad, wino, s


# ---- stem -------------------------------------------------------------------------------------------------------------------
def stem_dims(H, W):
    H1, W1 = out_size(H, 7, 2, 3), out_size(W, 7, 2, 3)
    return H1, W1, out_size(H1, 3, 2, 1), out_size(W1, 3, 2, 1)


def maxpool64(t, negate=None):
    """3x3 / 2 / pad 1 max-pool of NCHW fp64 (window minimum where `negate` [C] is set)."""
    tt = torch.from_numpy(t)
    mx = F.max_pool2d(tt, 3, 2, 1).numpy()
    if negate is None:
        return mx
    mn = -F.max_pool2d(-tt, 3, 2, 1).numpy()
    return np.where(negate[None, :, None, None], mn, mx)


@functools.lru_cache(maxsize=None)
def stem_case(name):
    """(x as the entry takes it: fp32 NCHW in [0, 1) or uint8 NHWC; conv1_w; frozen (m, r) [64] or None)."""
    _, B, H, W, u8, frozen = BY_NAME[name]
    rng = np.random.default_rng(_seed(name))
    x = rng.integers(0, 256, (B, H, W, 3), dtype=np.uint8) if u8 else rng.random((B, 3, H, W), dtype=np.float32)
    w = (rng.standard_normal((64, 3, 7, 7)) * (2.0 / (64 * 49)) ** 0.5).astype(np.float32)
    w[ZERO_CH] = 0
    fz = None
    if frozen:
        r = rng.uniform(0.5, 3.0, 64).astype(np.float32) * np.where(np.arange(64) % 3 == 1, -1, 1).astype(np.float32)
        fz = ((rng.standard_normal(64) * 0.1).astype(np.float32), r)
    return x, w, fz


@functools.lru_cache(maxsize=None)
def stem_expected(name, precision):
    """(pooled ref NCHW, its bar, m, r, dm, dr) of a STEM_CASES entry."""
    x, w, fz = stem_case(name)
    u8 = x.dtype == np.uint8
    x64 = x.transpose(0, 3, 1, 2).astype(np.float64) / 255.0 if u8 else x.astype(np.float64)
    s = conv64(x64, w, 2, 3)
    aw = np.abs(w.astype(np.float64))
    S = conv64(np.abs(x64), aw, 2, 3)
    floor = 2.0 ** -25 * conv64((x64 != 0).astype(np.float64), aw, 2, 3) + 2.0 ** -33 * conv64(np.abs(x64), (aw != 0).astype(np.float64), 2, 3)
    one = 1 if u8 else 0
    if precision == "fp32":
        bar = 1.01 * (3 * 147 + 8 + one) * U32 * S + floor
    else:
        bar = 1.01 * ((2 * 2.0 ** -11 + 2.0 ** -22) * S + (147 + one) * U32 * S) + floor
    wbar = maxpool64(bar)
    if fz is not None:
        m, r = (np.asarray(t, np.float64) for t in fz)
        ext = maxpool64(s, negate=r < 0)
        t = (ext - m[None, :, None, None]) * r[None, :, None, None]
        dt = np.abs(r)[None, :, None, None] * wbar + 3 * U32 * np.abs(t)
        ref = np.maximum(t, 0)
        B = s.shape[0]
        return ref, 1.01 * (dt + 2 * U32 * ref), np.tile(m, (B, 1)), np.tile(r, (B, 1)), np.zeros((B, 64)), np.zeros((B, 64))
    H1, W1 = s.shape[2:]
    P = ((W1 + 15) // 16) * ((H1 + 15) // 16) * 8
    m, r, dm, dr, r_hi = stats_reference(s, bar, 32, P)
    ext = maxpool64(s)
    e4 = lambda a: a[:, :, None, None]
    t = (ext - e4(m)) * e4(r)
    dt = e4(r_hi) * (wbar + e4(dm)) + np.abs(ext - e4(m)) * e4(dr) + 3 * U32 * np.abs(ext - e4(m)) * e4(r_hi)
    ref = np.maximum(t, 0)
    return ref, 1.01 * (dt + 2 * U32 * ref), m, r, dm, dr


@functools.lru_cache(maxsize=None)
def stem_exact_case(name):
    """(x fp32 NCHW in multiples of 2^-8 (plain), of 2^-4 (wwide: 2^8 w has 12 bits) or of 2^-12 with 12 bits (xwide), w, s fp64
    exact in fp32)."""
    _, B, H, W, flavour = BY_NAME[name]
    rng = np.random.default_rng(_seed(name))
    if flavour == "xwide":
        x = (rng.integers(2 ** 11, 2 ** 12, (B, 3, H, W)) * 2.0 ** -12).astype(np.float32)
    else:
        x = (rng.integers(0, 256, (B, 3, H, W)) * 2.0 ** -8).astype(np.float32)
    if flavour == "wwide":
        x = (rng.integers(0, 16, (B, 3, H, W)) * 2.0 ** -4).astype(np.float32)
        w = rng.integers(2 ** 11, 2 ** 12, (64, 3, 7, 7)) * 2.0 ** -12 * rng.choice([-1.0, 1.0], (64, 3, 7, 7))
    else:
        w = rng.choice([-1.0, 0.0, 1.0], (64, 3, 7, 7)) * 2.0 ** -(np.arange(64) % 3)[:, None, None, None]
    w = w.astype(np.float32)
    unit = {"plain": 2.0 ** -8 * 2.0 ** -2, "xwide": 2.0 ** -12 * 2.0 ** -2, "wwide": 2.0 ** -4 * 2.0 ** -12}[flavour]
    assert 1.01 * conv64(np.abs(x), np.abs(w), 2, 3).max() / unit < 2.0 ** 24, name
    s = conv64(x, w, 2, 3)
    assert np.array_equal(s.astype(np.float32).astype(np.float64), s), name
    return x, w, s


# ---- tail -------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def tail_case(name):
    """(y2, (m, r), idn, (md, rd) or None) of a TAIL_CASES entry, y2 / idn fp32 [B, HW, C]; every image has statistics of its
    own (scale and offset differ by image), so a stale cached set shows."""
    _, kind, B, HW, C = BY_NAME[name]
    rng = np.random.default_rng(_seed(name))
    sc = (1.0 + np.arange(B, dtype=np.float32))[:, None, None]
    y2 = (rng.standard_normal((B, HW, C), dtype=np.float32) * sc + sc)
    m = (sc[:, 0] + 0.1 * rng.standard_normal((B, C))).astype(np.float32)
    r = (1.0 / sc[:, 0] * rng.uniform(0.8, 1.25, (B, C))).astype(np.float32)
    if kind == "down":
        idn = (rng.standard_normal((B, HW, C), dtype=np.float32) * sc[::-1] - sc)
        md = (-sc[:, 0] + 0.1 * rng.standard_normal((B, C))).astype(np.float32)
        rd = (1.0 / sc[::-1][:, 0] * rng.uniform(0.8, 1.25, (B, C))).astype(np.float32)
        return y2, (m, r), idn, (md, rd)
    return y2, (m, r), np.maximum(rng.standard_normal((B, HW, C), dtype=np.float32), 0), None


def tail_reference(kind, y2, st, idn, dst):
    """(ref, bar) in fp64."""
    y, i = y2.astype(np.float64), idn.astype(np.float64)
    m, r = (t.astype(np.float64)[:, None, :] for t in st)
    t = (y - m) * r
    if dst is not None:
        i = (i - dst[0].astype(np.float64)[:, None, :]) * dst[1].astype(np.float64)[:, None, :]
    val = np.maximum(t + i, 0)
    d = 4.04 * U32 * (np.abs(t) + np.abs(i))
    if kind != "pool":
        return val, d
    n = y.shape[1]
    ref = val.mean(1)
    return ref, d.mean(1) + 1.01 * n * U32 * val.mean(1) + U32 * np.abs(ref)


# ---- wiring -----------------------------------------------------------------------------------------------------------------
def wiring_inputs(depth, B=3, H=40, W=56):
    """(x uint8 NHWC, conv weights in state_dict order) of the wiring test."""
    from dsmil_wsi_amd.ops import resnet_conv_shapes
    rng = np.random.default_rng(4100 + depth)
    x = rng.integers(0, 256, (B, H, W, 3), dtype=np.uint8)
    ws = [(rng.standard_normal(s) * (2.0 / (s[0] * s[2] * s[3])) ** 0.5).astype(np.float32) for s in resnet_conv_shapes(depth)]
    return x, ws


def worst(err, lim):
    """Largest err / bar over the elements with a positive bar (inf where a zero bar is exceeded)."""
    err, lim = np.asarray(err, np.float64), np.asarray(lim, np.float64)
    if np.any((lim == 0) & (err > 0)):
        return float("inf")
    return float((err[lim > 0] / lim[lim > 0]).max()) if np.any(lim > 0) else 0.0
