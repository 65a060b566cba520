"""Shapes, seeded inputs, fp64 references and bars of the STAGES of the 16-bit activation trunk (csrc/resnet_b16.h behind the
dsmil_trunk16_* entries), shared by tests/test_trunk16_host.py (the bars are reachable by the reference arithmetic and see the
mutants) and tests/test_trunk16_gpu.py (the kernels meet them).

Formats.  kind "bf16": 8 significant bits, u = 2^-8 (half a unit in the last place, relative to the value); "fp16": 11 bits,
u = 2^-11, plus 2^-24 absolute for its subnormal range.  u32 = 2^-24 is the same figure for fp32.  All roundings are to
nearest even.  For any fp32 value a within e of the exact ref,  |rne16(a) - ref| <= u |a| + e <= u |ref| + (1 + u) e:  the
accumulation error can carry a across a rounding boundary, which the (1 + u) — inside the 1.01 factors below — pays for.

Convolution (k_conv_b16n / k_conv_b16w / k_conv_b16g).  Operands are 16-bit values, so every product is exact in fp32; the
K = Cin ks^2 products are added in fp32 in SOME order (MFMA blocks of 16, then across stages).  Any order of K - 1 roundings
gives |a - s| <= (K - 1) u32 S (1 + O(K u32)),  S = sum |x| |w|,  so

    |got - s| <= u |s| + 1.01 K 2^-24 S   (+ 2^-24 for fp16)

which is the bar of tests/test_value_b16_host.py.  Every interior element is compared; border positions and the closing row
must be exactly 0.  The EXACT cases (x in {0, 1, 2}, w in {-1, 0, 1} 2^-k) make every partial sum an integer multiple of
2^-k below 2^24 2^-k: exact in fp32 in any order, so got == rne16(s) bit for bit, ties included.

InstanceNorm (k_stats_b16 + k_apply_b16), per (image, channel) over n = H W pixels, A = sum |x|, Q = sum x^2, exact mean m,
variance v = Q / n - m^2, r = 1 / sqrt(v + 1e-5).  The kernels form, in fp32, sum and sum of squares (n terms each, any
order of partials; the squares by fma or by a rounded product), m^ = sum / n, v^ = max(0, sumsq / n - m^ m^), r^ = 1 /
sqrt(v^ + 1e-5), y = rne16([relu]((x - m^) r^ [+ idn])):
    d_sum   <= 1.01 n u32 A                          d_sumsq <= 1.01 (n + 1) u32 Q
    dm      =  d_sum / n + u32 |m|                   (the division)
    dv      =  d_sumsq / n + 2 |m| dm + 2 u32 (Q / n + m^2)     (division, product, subtraction; the clamp at 0 only helps:
                                                                  v >= 0)
    dr      =  1/2 r_hi^3 dv + 8 u32 r_hi,   r_hi = 1 / sqrt(max(v - dv, 0) + 1e-5)
               (r is decreasing and convex in v, so |r(v^) - r(v)| <= |r'(v - dv)| dv — this is a bound, not only first
               order; 8 u32: the add, a square root and a division of at most 1 ulp = 2 u32 each, with room)
    dt      =  r_hi dm + |x - m| dr + 3 u32 |t|,   t = (x - m) r      (subtraction, product)
    bar     =  u |ref| + 1.01 (dt + 2 u32 |ref|)   (+ 2^-24 for fp16)       ref = [relu](t [+ idn])
(the residual add rounds once more: u32 |ref|; ReLU is 1-Lipschitz).  A constant channel has v = 0 and x - m = 0: ref = 0
[+ idn] and the bar is r_hi dm ~ 316 n u32 |m|.  Border positions must be exactly 0.

Pool (k_stats_b16 + k_pool_b16): feats = (fp32 sum over the n pixels of relu(t + idn)) / n, no 16-bit rounding:
    bar     =  mean(1.01 (dt + 2 u32 |val|)) + 1.01 n u32 mean |val| + u32 |ref|,    val = relu(t + idn)."""
import functools

import numpy as np
import torch
import torch.nn.functional as F

KINDS = ("bf16", "fp16")
U16 = {"bf16": 2.0 ** -8, "fp16": 2.0 ** -11}
ABS16 = {"bf16": 0.0, "fp16": 2.0 ** -24}
U32 = 2.0 ** -24
EPS = 1e-5


# ---- 16-bit formats ---------------------------------------------------------------------------------------------------------
def to_bits(a, kind):
    """fp32 array -> uint16 bits of its round-to-nearest-even 16-bit value (integer arithmetic for bf16, as cvt16 of
    csrc/resnet_b16.h; IEEE conversion for fp16)."""
    a = np.ascontiguousarray(a, np.float32)
    if kind == "fp16":
        return a.astype(np.float16).view(np.uint16)
    u = a.view(np.uint32).astype(np.uint64)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def from_bits(b, kind):
    """uint16 bits -> fp32 values."""
    b = np.ascontiguousarray(b).view(np.uint16)
    if kind == "fp16":
        return b.view(np.float16).astype(np.float32)
    return (b.astype(np.uint32) << 16).view(np.float32)


def rne16(a, kind):
    """fp32 (or fp64 values exact in fp32) -> the nearest-even 16-bit value, as fp32."""
    return from_bits(to_bits(np.asarray(a, np.float32), kind), kind)


def trunc16(a, kind):
    """The truncation mutant: round toward zero."""
    a = np.ascontiguousarray(a, np.float32)
    if kind == "bf16":
        return (a.view(np.uint32) & np.uint32(0xFFFF0000)).view(np.float32)
    r = a.astype(np.float16).astype(np.float32)
    over = np.abs(r) > np.abs(a)                       # rounded away from zero: step one 16-bit value back
    h = a.astype(np.float16).view(np.uint16)
    return np.where(over, (h - over.astype(np.uint16)).view(np.float16).astype(np.float32), r)


def torch_round(a, kind):
    """torch's cast, the independent check of rne16."""
    dt = torch.bfloat16 if kind == "bf16" else torch.float16
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(dt).to(torch.float32).numpy()


# ---- the shared-border layout -----------------------------------------------------------------------------------------------
def npos(B, H, W):
    return B * (H + 1) * (W + 1) + (W + 1)


def interior_index(B, H, W):
    """Flat positions of the pixels, [B, H, W]: image n, pixel (y, x) is position (n (H+1) + y + 1)(W+1) + x."""
    n, y, x = np.meshgrid(np.arange(B), np.arange(H), np.arange(W), indexing="ij")
    return (n * (H + 1) + y + 1) * (W + 1) + x


def border_mask(B, H, W):
    """bool [npos]: row 0 of every image, column W of every row, the closing row."""
    m = np.ones(npos(B, H, W), bool)
    m[interior_index(B, H, W).ravel()] = False
    return m


def pad_bits(x_nchw, kind):
    """A representable NCHW map -> the uint16 buffer [npos, C] the kernels read."""
    B, C, H, W = x_nchw.shape
    buf = np.zeros((npos(B, H, W), C), np.uint16)
    buf[interior_index(B, H, W)] = to_bits(x_nchw, kind).transpose(0, 2, 3, 1)
    return buf


def unpad(buf, B, H, W, kind):
    """uint16 / int16 buffer [npos, C] -> (NCHW fp64 [B, C, H, W], the raw uint16 rows of the border positions)."""
    buf = np.ascontiguousarray(buf).view(np.uint16)
    assert buf.shape[0] == npos(B, H, W), (buf.shape, B, H, W)
    vals = from_bits(buf[interior_index(B, H, W)], kind).astype(np.float64)
    return np.ascontiguousarray(vals.transpose(0, 3, 1, 2)), buf[border_mask(B, H, W)]


# ---- inputs -----------------------------------------------------------------------------------------------------------------
def relu_map(seed, B, C, H, W, kind):
    """Non-negative O(1) representable NCHW fp32: what a ReLU leaves (half of it zero)."""
    x = np.random.default_rng(seed).standard_normal((B, C, H, W)).astype(np.float32)
    return rne16(np.maximum(x, 0), kind)


def conv_weights(seed, cout, cin, ks):
    """fp32 OIHW at kaiming-normal(fan_out) scale — NOT representable: the kernel's pack rounds them."""
    w = np.random.default_rng(seed).standard_normal((cout, cin, ks, ks)).astype(np.float32)
    return w * np.float32((2.0 / (cout * ks * ks)) ** 0.5)


# ---- convolution ------------------------------------------------------------------------------------------------------------
# (name, B, Hi, Wi, Cin, Cout, ks, stride, pad).  run_conv's launch conditions: 3x3/1 with Cout % 128 == 0 -> k_conv_b16w<256,128>
# (256 positions x 128 channels per workgroup, window (256 + 2 (W+1) + 2) x 2 pieces <= 6 x 256: W <= 254); 64 -> 64 ->
# k_conv_b16n (window x 8 pieces <= 16 x 256: W <= 126); other Cout % 64 == 0 -> k_conv_b16w<512,64>; strided -> k_conv_b16g.
CONV_CASES = [
    # k_conv_b16n
    ("n_2x9x7", 2, 9, 7, 64, 64, 3, 1, 1),              # 174 positions: one partial workgroup
    ("n_3x17x13", 3, 17, 13, 64, 64, 3, 1, 1),          # 770 positions: four workgroups, tiles straddle images
    ("n_1x56x56", 1, 56, 56, 64, 64, 3, 1, 1),          # the real map
    ("n_1x3x126", 1, 3, 126, 64, 64, 3, 1, 1),          # W + 1 = 127: the staging budget exactly
    # k_conv_b16w<256,128,2,2>
    ("w_32_128", 2, 6, 5, 32, 128, 3, 1, 1),            # smallest K: one chunk pair
    ("w_128_28", 2, 28, 28, 128, 128, 3, 1, 1),
    ("w_256_14", 3, 14, 14, 256, 256, 3, 1, 1),
    ("w_256_5x9", 3, 5, 9, 256, 256, 3, 1, 1),
    ("w_512_7", 5, 7, 7, 512, 512, 3, 1, 1),
    ("w_512_2", 3, 2, 2, 512, 512, 3, 1, 1),
    ("w_32_128_w254", 1, 3, 254, 32, 128, 3, 1, 1),     # W + 1 = 255: the window budget exactly
    # k_conv_b16w<512,64,4,1>
    ("v_128_64", 2, 9, 7, 128, 64, 3, 1, 1),
    ("v_64_192", 3, 17, 13, 64, 192, 3, 1, 1),          # 770 positions: two workgroups of 512, three channel blocks
    # k_conv_b16g: 3x3/2 pad 1 and 1x1/2 pad 0, even and odd maps
    ("g3_64_128_9x7", 2, 9, 7, 64, 128, 3, 2, 1),       # 9 x 7 -> 5 x 4
    ("g3_64_128_57", 1, 57, 57, 64, 128, 3, 2, 1),      # 57 -> 29
    ("g3_128_256_7", 5, 7, 7, 128, 256, 3, 2, 1),       # 7 -> 4
    ("g3_256_512_8", 2, 8, 8, 256, 512, 3, 2, 1),       # 8 -> 4
    ("g1_64_128_8", 1, 8, 8, 64, 128, 1, 2, 0),
    ("g1_64_128_57", 1, 57, 57, 64, 128, 1, 2, 0),
    ("g1_128_256_9x7", 2, 9, 7, 128, 256, 1, 2, 0),
    ("g1_256_512_7", 5, 7, 7, 256, 512, 1, 2, 0),
]
CONV_BY_NAME = {c[0]: c for c in CONV_CASES}
# maps one pixel wider than a kernel's budget: (B, Hi, Wi, Cin, Cout) of a 3x3/1 conv that must answer DSMIL_E_UNSUPPORTED
CONV_REFUSED = [(1, 3, 128, 64, 64), (1, 3, 127, 64, 64), (1, 3, 256, 32, 128), (1, 3, 255, 32, 128), (1, 3, 255, 128, 64)]

# exact cases: (name, B, Hi, Wi, Cin, Cout, ks, stride, pad, kinds whose sums pass the format's integer range and must tie)
EXACT_CASES = [
    ("x_n", 2, 9, 7, 64, 64, 3, 1, 1, ("bf16",)),                  # K = 576: sums to ~1000
    ("x_w", 2, 5, 5, 512, 512, 3, 1, 1, ("bf16", "fp16")),         # K = 4608: sums to ~5000
    ("x_v", 1, 9, 7, 128, 64, 3, 1, 1, ("bf16",)),
    ("x_g3", 1, 9, 7, 256, 512, 3, 2, 1, ("bf16", "fp16")),        # K = 2304
    ("x_g1", 2, 7, 7, 256, 512, 1, 2, 0, ("bf16",)),               # K = 256: sums to ~400
]
EXACT_BY_NAME = {c[0]: c for c in EXACT_CASES}


def out_size(n, ks, stride, pad):
    return (n + 2 * pad - ks) // stride + 1


@functools.lru_cache(maxsize=None)
def conv_case(name, kind):
    """(x NCHW fp32 representable, w fp32 OIHW unrounded, s fp64, S fp64) of a CONV_CASES entry."""
    _, B, Hi, Wi, Cin, Cout, ks, stride, pad = CONV_BY_NAME[name]
    seed = 1000 + sum(map(ord, name))
    x = relu_map(seed, B, Cin, Hi, Wi, kind)
    w = conv_weights(seed + 1, Cout, Cin, ks)
    s, S = conv_reference(x, rne16(w, kind), stride, pad)
    return x, w, s, S


@functools.lru_cache(maxsize=None)
def exact_case(name):
    """(x in {0, 1, 2}, w in {-1, 0, 1} 2^-k per output channel, s fp64): exact in fp32 in any order.  The share of +1 among
    the weights grows with the output channel, so the sums sweep from about -K/2 to about +K."""
    _, B, Hi, Wi, Cin, Cout, ks, stride, pad, _ = EXACT_BY_NAME[name]
    rng = np.random.default_rng(77 + sum(map(ord, name)))
    x = rng.choice(np.array([0, 1, 2], np.float32), (B, Cin, Hi, Wi), p=(0.1, 0.2, 0.7))
    p_plus = np.linspace(0.05, 0.9, Cout)[:, None, None, None]
    r = rng.random((Cout, Cin, ks, ks))
    w = np.where(r < p_plus, 1.0, np.where(r < p_plus + 0.1, 0.0, -1.0))
    w = (w * 2.0 ** -(np.arange(Cout) % 4)[:, None, None, None]).astype(np.float32)
    s, _ = conv_reference(x, w, stride, pad)
    return x, w, s


def conv_reference(x, w16, stride, pad):
    """s = conv(x, w16) and S = conv(|x|, |w16|) in fp64 (operands as the kernel multiplies them: both representable)."""
    xt, wt = torch.from_numpy(np.asarray(x, np.float64)), torch.from_numpy(np.asarray(w16, np.float64))
    return (F.conv2d(xt, wt, stride=stride, padding=pad).numpy(), F.conv2d(xt.abs(), wt.abs(), stride=stride, padding=pad).numpy())


def conv_bar(s, S, K, kind):
    """|got - s| <= u |s| + 1.01 K 2^-24 S (+ 2^-24 for fp16), elementwise."""
    return U16[kind] * np.abs(s) + 1.01 * K * U32 * S + ABS16[kind]


def is_tie(s, kind):
    """Elements of a sum (exact in fp32) that lie exactly half way between two neighbouring 16-bit values."""
    s32 = np.asarray(s, np.float32)
    assert np.array_equal(s32.astype(np.float64), s)
    lo = trunc16(s32, kind).astype(np.float64)                  # the neighbour toward zero
    return np.abs(s - lo) == spacing16(lo, kind) / 2


def spacing16(v, kind):
    """Distance from |v| to the next 16-bit value away from zero (v a normal 16-bit value or 0)."""
    bits = 8 if kind == "bf16" else 11
    with np.errstate(divide="ignore"):
        e = np.floor(np.log2(np.maximum(np.abs(v), 2.0 ** -14)))
    return 2.0 ** (e - (bits - 1))


# ---- InstanceNorm and pool --------------------------------------------------------------------------------------------------
# (name, B, H, W, C).  stat_chunks(H W) = 1 (< 128), 2 (< 512), 4 (< 2048), 8; k_stats_b16 steps four pixels per lane.
NORM_CASES = [
    ("c64_56", 1, 56, 56, 64),          # 3136 pixels: 8 chunks
    ("c64_47x45", 2, 47, 45, 64),       # 2115 pixels: 8 chunks, odd
    ("c128_28", 2, 28, 28, 128),        # 784: 4 chunks
    ("c128_23", 3, 23, 23, 128),        # 529: 4 chunks, odd
    ("c256_14", 3, 14, 14, 256),        # 196: 2 chunks
    ("c256_11x13", 2, 11, 13, 256),     # 143: 2 chunks, odd
    ("c512_7", 5, 7, 7, 512),           # 49: 1 chunk
    ("c512_3x3", 3, 3, 3, 512),
    ("c512_2x2", 3, 2, 2, 512),         # H W = 4, 2, 1
    ("c512_1x2", 2, 1, 2, 512),
    ("c512_1x1", 2, 1, 1, 512),
]
NORM_BY_NAME = {c[0]: c for c in NORM_CASES}
CONST_CH, SHIFT_CH = 3, 5               # maps up to 200 pixels: a constant channel; a channel with mean 20 and spread ~0.5
POOL_CASES = [("p512_7", 5, 7, 7, 512), ("p512_3x4", 3, 3, 4, 512), ("p512_1x1", 2, 1, 1, 512)]
POOL_BY_NAME = {c[0]: c for c in POOL_CASES}


@functools.lru_cache(maxsize=None)
def norm_inputs(name, kind):
    """(x zero-mean O(1) representable NCHW fp32 — a conv's output —, idn non-negative representable) of a NORM / POOL case."""
    _, B, H, W, C = (NORM_BY_NAME.get(name) or POOL_BY_NAME[name])
    seed = 5000 + sum(map(ord, name))
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal((B, C, H, W)) * rng.uniform(0.3, 2.0, (1, C, 1, 1)) + rng.uniform(-0.5, 0.5, (B, C, 1, 1))).astype(np.float32)
    if H * W <= 200:
        x[:, CONST_CH] = 1.3359375                                   # representable in both kinds, not a power of two
        x[:, SHIFT_CH] = 20.0 + 0.5 * rng.standard_normal((B, H, W))
    return rne16(x, kind), relu_map(seed + 1, B, C, H, W, kind)


def norm_reference(x, idn, relu, kind, pool=False):
    """fp64 reference and bar (module docstring) of [relu]((x - m) r [+ idn]) over the pixels of every (image, channel); pool:
    the mean over pixels of relu(. + idn) and the pool bar.  Returns (ref, bar)."""
    x = np.asarray(x, np.float64)
    n = x.shape[2] * x.shape[3]
    ax = (2, 3)
    A, Q = np.abs(x).sum(ax, keepdims=True), (x * x).sum(ax, keepdims=True)
    m = x.sum(ax, keepdims=True) / n
    v = np.maximum(((x - m) ** 2).sum(ax, keepdims=True) / n, 0.0)
    r = 1.0 / np.sqrt(v + EPS)
    dm = 1.01 * n * U32 * A / n + U32 * np.abs(m)
    dv = 1.01 * (n + 1) * U32 * Q / n + 2 * np.abs(m) * dm + 2 * U32 * (Q / n + m * m)
    r_hi = 1.0 / np.sqrt(np.maximum(v - dv, 0.0) + EPS)
    dr = 0.5 * r_hi ** 3 * dv + 8 * U32 * r_hi
    t = (x - m) * r
    dt = r_hi * dm + np.abs(x - m) * dr + 3 * U32 * np.abs(x - m) * r_hi
    val = t if idn is None else t + np.asarray(idn, np.float64)
    if relu:
        val = np.maximum(val, 0.0)
    d = 1.01 * (dt + 2 * U32 * np.abs(val))
    if pool:
        ref = val.mean(ax)
        return ref, d.mean(ax) + 1.01 * n * U32 * np.abs(val).mean(ax) + U32 * np.abs(ref)
    return val, U16[kind] * np.abs(val) + d + ABS16[kind]


# ---- the trunk wiring case --------------------------------------------------------------------------------------------------
def trunk_inputs(depth, kind, B=3, Hp=9, Wp=9):
    """(x fp32 NHWC [B,Hp,Wp,64] as a ReLU + max pool leaves it, conv weights in state_dict order as fp32 arrays)."""
    from dsmil_wsi_amd.ops import resnet_conv_shapes
    x = relu_map(900 + depth, B, 64, Hp, Wp, kind).transpose(0, 2, 3, 1)
    ws = [conv_weights(910 + depth + i, s[0], s[1], s[2]) for i, s in enumerate(resnet_conv_shapes(depth))]
    return np.ascontiguousarray(x), ws


def worst(err, lim):
    """Largest err / bar over the elements with a positive bar (inf where a zero bar is exceeded)."""
    err, lim = np.asarray(err, np.float64), np.asarray(lim, np.float64)
    if np.any((lim == 0) & (err > 0)):
        return float("inf")
    return float((err[lim > 0] / lim[lim > 0]).max()) if np.any(lim > 0) else 0.0
