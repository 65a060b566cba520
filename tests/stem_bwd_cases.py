"""Shapes, seeded inputs, fp64 references, bars, a numpy emulation and mutants of the stem's InstanceNorm / ReLU / max-pool backward
(csrc/stem_bwd.hip behind dsmil_stem_pool_bwd) and of the winner rule of the training stem's pool (dsmil_trunk32_stem_train),
shared by tests/test_stem_bwd_host.py (the emulation of the stated arithmetic meets the bars, the mutants do not),
tests/test_stem_bwd_cabi.py (the plan of every case is pinned) and tests/test_stem_bwd_gpu.py (the kernels meet them).  Nothing
here is tuned on a GPU or taken from the code under test; chunk, run_len, lanes and n_partials come from the declared plan.

The function.  y [B, H1, W1, C] is a raw map with statistics (m, r) [B, C], pooled = maxpool3x3/2/1(relu((y - m) r)) is
[B, Hp, Wp, C] and g is its gradient.  With a = fl(fl(y - m) r) in fp32, the window of pooled pixel (oy, ox) is rows
2 oy - 1 .. 2 oy + 1 and columns 2 ox - 1 .. 2 ox + 1 clipped to the map, and its WINNER is the first pixel in row-major order
whose a equals the window's largest a (winners()).  Then
    q[n,p,c] = sum over the windows whose winner is p of g[n,w,c]   if a[n,p,c] > 0, else 0
    gy       = INB(q; y, m, r) = r (q - mean_p q - x^ mean_p (q x^)),   x^ = (y - m) r
The fp64 reference (closed_form) routes in fp32 exactly as specified — winners and ReLU mask from the float32 a — and computes q
and INB in fp64 over the same fp32 inputs; autograd_check() holds it against fp64 torch autograd of
max_pool2d(relu(instance_norm(y))).

The bar, per element: norm_bwd_cases' bar with D = run_len + lanes + n_partials from the declared plan, plus the rounding of
q's own additions.  A pixel collects at most four windows, added from + 0 in window row-major order: three roundings at most,
each at most u times a partial sum of absolute values, so |q' - q| <= 3 u G with G = the sum of the |g| the pixel collects (0
where it is masked).  Carried through norm_bwd_cases' chain (A1 = mean |q|, A2 = mean |q x^|, a = mean q, b = mean (q x^),
t = q - a - x^ b):
    |a' - a| <= (D + 1) u A1 + 3 u mean G
    |b' - b| <= (D + 3) u A2 + 3 u mean (G |x^|)
    |fl(q' - a') - (q - a)| <= 3 u G + |a' - a| + u |q - a|
    bar = 1.01 u r [ (D + 1) A1 + 3 mean G + 3 G + |q - a| + |x^| ((D + 3) A2 + 3 mean (G |x^|) + 2 |b|) + 2 |t| ]
          + 4 * 2^-149 max(r, 1)
Where q, a and b vanish (H1 W1 = 1 with m = y, a fully masked channel, g = 0) every operation is exact and so is the zero.

EXACT cases.  y, m and g are small integers drawn from a handful of values, so that MANY windows tie at the top, r is a power
of two and H1 W1 a power of two: every x^, q, product, partial sum in any order, mean and the final fma is a dyadic rational of
fewer than 24 significant bits (checked by the builder), so the result must equal the fp64 reference bit for bit — which holds
only under the first-in-scan-order rule."""
import functools

import numpy as np
import torch
import torch.nn.functional as F

import norm_bwd_cases as nc
from trunk32_cases import U32, worst  # noqa: F401

EPS = 1e-5
# (name, B, H1, W1, C, g magnitude)
CASES = [
    ("p_1x1", 3, 1, 1, 64, 1.0), ("p_2x2", 1, 2, 2, 64, 1e-6),
    ("p_5x7", 2, 5, 7, 64, 1.0),                     # odd sizes: the last window hangs over the edge
    ("p_16x16", 1, 16, 16, 64, 1e-6),                # exactly one 256-pixel chunk
    ("p_16x17", 3, 16, 17, 64, 1.0),                 # a chunk and a row
    ("p_27x26", 1, 27, 26, 64, 1e-6),                # three partials
    ("p_9x9_128", 1, 9, 9, 128, 1.0),
]
# name: (Hp, Wp, chunk, n_partials, run_len, lanes, grid_partial, grid_finish, grid_apply, groups)
PLANS = {
    "p_1x1": (1, 1, 256, 1, 1, 16, 3, 2, 1, 1), "p_2x2": (1, 1, 256, 1, 1, 16, 1, 1, 1, 1),
    "p_5x7": (3, 4, 256, 1, 3, 16, 2, 1, 5, 1), "p_16x16": (8, 8, 256, 1, 16, 16, 1, 1, 16, 1),
    "p_16x17": (8, 9, 256, 2, 16, 16, 6, 2, 51, 1), "p_27x26": (14, 13, 256, 3, 16, 16, 3, 1, 44, 1),
    "p_9x9_128": (5, 5, 256, 1, 11, 8, 1, 1, 11, 1),
}
# (name, B, H1, W1, C)
EXACT_CASES = [("x_8x8", 2, 8, 8, 64), ("x_16x16", 1, 16, 16, 64)]
BY_NAME = {c[0]: c for c in CASES + EXACT_CASES}
MASKED_CH = 5                    # in image 0 every element of this channel is masked
MUTANTS = ("last_winner_on_ties", "no_relu_mask", "windows_from_2o", "first_window_only", "drop_xhat_term", "drop_mean_q")


def _seed(name):
    return 8300 + sum((i + 1) * ord(ch) for i, ch in enumerate(name))


def pooled_dims(H1, W1):
    return (H1 - 1) // 2 + 1, (W1 - 1) // 2 + 1


def plan_of(B, H1, W1, C, chunk=256):
    """(Hp, Wp, chunk, n_partials, run_len, lanes) the documented rule gives for a case whose chunk is ``chunk``."""
    return pooled_dims(H1, W1) + nc.plan_of("relu", B, H1 * W1, C, chunk)


# ---- routing: the winner rule ------------------------------------------------------------------------------------------------
def a_of(y, m, r, dtype=np.float32):
    """fl(fl(y - m) r) in ``dtype`` for y [B, H1, W1, C], m, r [B, C]."""
    y, m, r = (np.asarray(t, dtype) for t in (y, m, r))
    return ((y - m[:, None, None, :]).astype(dtype) * r[:, None, None, :]).astype(dtype)


def _windows(a, off=-1):
    """[9, B, Hp, Wp, C]: the windows' values in row-major position order, -inf outside the map.  ``off``: the first row and
    column of window 0 (-1 for padding 1)."""
    B, H1, W1, C = a.shape
    Hp, Wp = pooled_dims(H1, W1)
    pad = np.full((B, 2 * Hp + 2, 2 * Wp + 2, C), -np.inf, a.dtype)
    pad[:, -off:-off + H1, -off:-off + W1] = a
    return np.stack([pad[:, dy:dy + 2 * Hp - 1:2, dx:dx + 2 * Wp - 1:2] for dy in range(3) for dx in range(3)])


def winners(a, last=False, off=-1):
    """uint8 [B, Hp, Wp, C]: dy * 3 + dx of the first (``last``: the last) pixel of each window holding its largest a."""
    w = _windows(a, off)
    return (8 - np.argmax(w[::-1], 0) if last else np.argmax(w, 0)).astype(np.uint8)


def top_two_gap(a):
    """[B, Hp, Wp, C]: largest minus second largest value of each window (inf for a one-pixel window)."""
    w = np.sort(_windows(a), 0)
    return w[8] - w[7]


def scatter(g, win, H1, W1, off=-1, dtype=np.float64):
    """[B, H1, W1, C]: every window's g added onto the pixel its winner names (window-major; fp64: the order is immaterial).
    Returns (the sum, the sum of |g|)."""
    B, Hp, Wp, C = g.shape
    q = np.zeros((B, H1 + 3, W1 + 3, C), dtype)
    G = np.zeros_like(q)
    b, oy, ox, c = np.meshgrid(np.arange(B), np.arange(Hp), np.arange(Wp), np.arange(C), indexing="ij")
    iy, ix = 2 * oy + off + win // 3, 2 * ox + off + win % 3
    assert iy.min() >= 0 and ix.min() >= 0
    np.add.at(q, (b, iy, ix, c), np.asarray(g, dtype))
    np.add.at(G, (b, iy, ix, c), np.abs(np.asarray(g, dtype)))
    return q[:, :H1, :W1], G[:, :H1, :W1]


def gather32(g, win, H1, W1, first_only=False):
    """[B, H1, W1, C] fp32: what each pixel collects by the stated gather — its (at most four) windows in row-major order, a
    window's g where win names the pixel's position, an exact 0 elsewhere, added in fp32 from + 0."""
    B, Hp, Wp, C = g.shape
    g = np.asarray(g, np.float32)
    py, px = np.arange(H1), np.arange(W1)
    q = np.zeros((B, H1, W1, C), np.float32)
    for sy in range(2):
        oy = (py >> 1) + sy
        vy = (oy < Hp) & ((py & 1) == 1 if sy else True) & (not (first_only and sy))
        dy = py - 2 * oy + 1
        for sx in range(2):
            ox = (px >> 1) + sx
            vx = (ox < Wp) & ((px & 1) == 1 if sx else True) & (not (first_only and sx))
            dx = px - 2 * ox + 1
            oyc, oxc = np.minimum(oy, Hp - 1), np.minimum(ox, Wp - 1)
            pos = (dy[:, None] * 3 + dx[None, :])[None, :, :, None]
            take = (vy[:, None] & vx[None, :])[None, :, :, None] & (win[:, oyc][:, :, oxc] == pos)
            q = (q + np.where(take, g[:, oyc][:, :, oxc], np.float32(0))).astype(np.float32)
    return q


# ---- fp64 -------------------------------------------------------------------------------------------------------------------
def closed_form(inp, run_len=1, lanes=1, n_partials=1, route=np.float32):
    """(gy in fp64, its bar) over the fp32 inputs of ``inp`` (g, y, m, r): winners and ReLU mask from a in ``route``."""
    D = run_len + lanes + n_partials
    y = np.asarray(inp["y"])
    B, H1, W1, C = y.shape
    a = a_of(y, inp["m"], inp["r"], route)
    q, G = scatter(inp["g"], winners(a), H1, W1)
    q, G = np.where(a > 0, q, 0.0), np.where(a > 0, G, 0.0)
    r = np.asarray(inp["r"], np.float64)[:, None, None, :]
    xh = (y.astype(np.float64) - np.asarray(inp["m"], np.float64)[:, None, None, :]) * r
    mean = lambda t: t.mean((1, 2), keepdims=True)
    am, b, A1, A2 = mean(q), mean(q * xh), mean(np.abs(q)), mean(np.abs(q * xh))
    t = q - am - xh * b
    bar = 1.01 * U32 * r * ((D + 1) * A1 + 3 * mean(G) + 3 * G + np.abs(q - am) +
                            np.abs(xh) * ((D + 3) * A2 + 3 * mean(G * np.abs(xh)) + 2 * np.abs(b)) + 2 * np.abs(t)) + \
        4 * 2.0 ** -149 * np.maximum(r, 1.0)
    return r * t, bar


def autograd_check(B=2, H1=9, W1=7, C=8, seed=3):
    """Largest |closed form - fp64 autograd| relative to the largest gradient: statistics computed in fp64 from y itself, the
    function max_pool2d(relu(instance_norm(y)), 3, 2, 1) differentiated by torch in float64 on the CPU."""
    rng = np.random.default_rng(seed)
    y = rng.standard_normal((B, H1, W1, C)) * 1.5 + 0.3
    g = rng.standard_normal((B,) + pooled_dims(H1, W1) + (C,))
    ty = torch.from_numpy(np.ascontiguousarray(y.transpose(0, 3, 1, 2))).requires_grad_(True)
    out = F.max_pool2d(torch.relu(F.instance_norm(ty, eps=EPS)), 3, 2, 1)
    grad = torch.autograd.grad(out, ty, torch.from_numpy(np.ascontiguousarray(g.transpose(0, 3, 1, 2))))[0].numpy().transpose(0, 2, 3, 1)
    flat = y.reshape(B, -1, C)
    inp = dict(g=g, y=y, m=flat.mean(1), r=1.0 / np.sqrt(flat.var(1) + EPS))
    return float(np.abs(closed_form(inp, route=np.float64)[0] - grad).max() / np.abs(grad).max())


# ---- inputs -----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def case(name):
    """The fp32 inputs of a CASES entry as a dict: g [B,Hp,Wp,C], y [B,H1,W1,C], m, r [B,C], win uint8 [B,Hp,Wp,C] (the winner
    rule applied to y, m, r).  y is normal at 1.5 around 0.3, its statistics are its own (fp64, rounded to fp32); with H1 W1 = 1
    the mean is y itself.  g is normal at the case's magnitude with a tenth of its elements exactly zero.  In image 0 channel
    MASKED_CH is fully masked (its mean lies above every element).  y is moved off its mean until |x^| >= 1e-3, so that an fp32
    and an fp64 evaluation of the mask agree on every sign, and no window has its top two fp32 a equal — both asserted here."""
    _, B, H1, W1, C, mag = BY_NAME[name]
    Hp, Wp = pooled_dims(H1, W1)
    rng = np.random.default_rng(_seed(name))
    y = (rng.standard_normal((B, H1, W1, C)) * 1.5 + 0.3).astype(np.float32)
    m, r = nc._f32(*nc._stats64(y.reshape(B, -1, C)))
    g = rng.standard_normal((B, Hp, Wp, C)) * mag
    g = np.where(rng.random(g.shape) < 0.1, 0.0, g).astype(np.float32)
    xh64 = lambda: (y.astype(np.float64) - m.astype(np.float64)[:, None, None, :]) * r.astype(np.float64)[:, None, None, :]
    if H1 * W1 > 1:
        m[0, MASKED_CH] = y[0, :, :, MASKED_CH].max() + 1.0
        xh = xh64()
        near = np.abs(xh) < 2e-3
        step = np.where(xh >= 0, 1.0, -1.0) * (4e-3 + 1e-3 * rng.random(xh.shape))
        y[near] = (m[:, None, None, :] + step / r[:, None, None, :]).astype(np.float32)[near]
    xh, a = xh64(), a_of(y, m, r)
    assert np.all((np.abs(xh) >= 1e-3) | (xh == 0)) and np.array_equal(a > 0, xh > 0), name
    assert H1 * W1 == 1 or not (a[0, :, :, MASKED_CH] > 0).any()
    assert H1 * W1 == 1 or top_two_gap(a).min() > 0, name                # no window's top two fp32 a are equal
    inp = dict(g=g, y=y, m=m, r=r, win=winners(a))
    for t in inp.values():
        t.setflags(write=False)
    return inp


@functools.lru_cache(maxsize=None)
def expected(name):
    _, _, chunk, n_partials, run_len, lanes = PLANS[name][:6]
    return closed_form(case(name), run_len, lanes, n_partials)


@functools.lru_cache(maxsize=None)
def exact_case(name):
    """(inputs, gy fp64 == its fp32 value) of an EXACT_CASES entry; the builder asserts that many windows tie at the top and
    that the last-winner rule would give another result."""
    _, B, H1, W1, C = BY_NAME[name]
    Hp, Wp = pooled_dims(H1, W1)
    rng = np.random.default_rng(_seed(name))
    ints = lambda lo, hi, shape: rng.integers(lo, hi + 1, shape).astype(np.float32)
    inp = dict(g=ints(-3, 3, (B, Hp, Wp, C)), y=ints(-2, 2, (B, H1, W1, C)), m=ints(-1, 1, (B, C)),
               r=(2.0 ** rng.integers(-1, 2, (B, C))).astype(np.float32))
    a = a_of(inp["y"], inp["m"], inp["r"])
    inp["win"] = winners(a)
    assert (top_two_gap(a) == 0).mean() > 0.5, name                      # more than half the windows tie at the top
    ref = closed_form(inp)[0]
    assert np.array_equal(ref.astype(np.float32).astype(np.float64), ref), name
    # every intermediate is a multiple of 2^-10 below 2^10 (x^ of 2^-1 below 2^3, |q| <= 12, the means of 2^-9 below 2^7): < 24 bits
    HW = H1 * W1
    assert HW & (HW - 1) == 0 and HW <= 256
    for t in inp.values():
        t.setflags(write=False)
    return inp, ref


# ---- the numpy emulation of the stated arithmetic ---------------------------------------------------------------------------
def emulate(inp, chunk=256, mutant=None, win=None):
    """gy (fp32) by the stated arithmetic and order.  ``win``: the winners to read (default: the winner rule applied to y, under
    the mutant's rule where the mutant changes it)."""
    y = np.asarray(inp["y"], np.float32)
    B, H1, W1, C = y.shape
    m, r = np.asarray(inp["m"], np.float32), np.asarray(inp["r"], np.float32)
    a = a_of(y, m, r)
    if mutant == "windows_from_2o":                                      # the windows at 2 o .. 2 o + 2: no padding
        qc = scatter(inp["g"], winners(a, off=0), H1, W1, off=0, dtype=np.float32)[0]
    else:
        if win is None:
            win = winners(a, last=mutant == "last_winner_on_ties")
        qc = gather32(inp["g"], win, H1, W1, first_only=mutant == "first_window_only")
    q = qc if mutant == "no_relu_mask" else np.where(a > 0, qc, np.float32(0)).astype(np.float32)
    lanes = nc.lanes_of(C)
    flat = lambda t: np.ascontiguousarray(t.reshape(B, H1 * W1, C))
    q, xh = flat(q), flat(a)
    hw = np.float32(H1 * W1)
    mq = (nc._sum_pixels(q, chunk, lanes, C) / hw).astype(np.float32)[:, None, :]
    mqx = (nc._sum_pixels(q, chunk, lanes, C, fma_with=xh) / hw).astype(np.float32)[:, None, :]
    if mutant == "drop_mean_q":
        mq = np.zeros_like(mq)
    if mutant == "drop_xhat_term":
        mqx = np.zeros_like(mqx)
    t = nc._fma32(-xh, np.broadcast_to(mqx, xh.shape), (q - mq).astype(np.float32))
    return (r[:, None, :] * t).astype(np.float32).reshape(B, H1, W1, C)


def worst_ratio(got, exp):
    ref, bar = exp
    a = np.asarray(got, np.float64)
    assert a.shape == ref.shape
    return worst(np.abs(a - ref), bar)


# ---- the stem alone and the whole model -------------------------------------------------------------------------------------
# Winners come from the forward's own fp32-class map, the fp64 model's from its own: the comparison is meaningful only where no
# decision can flip between the two.  MARGIN, in normalised units: in the fp64 model no live window (largest a > 0) has its top
# two values closer than this, and no winner lies closer to zero.  The seeds below were chosen on the CPU for that; the builders
# assert it.
MARGIN = 1e-4
# (name, B, H, W, seed): uniform [0, 1) inputs, kaiming-normal(fan_out) conv1 weights
STEMS = [("stem_32", 2, 32, 32, 0)]                 # margin 3.2e-4 (seeds 0 .. 39: 15 of them reach 1e-4)
# conv_bwd_cases.MODEL_SEED = 5 puts a window at 2.6e-5; of the seeds 0 .. 399 three reach 1e-4 over the 32768 windows of
# 2 x 64 x 64 (188: 1.6e-4, 258, 352), and of those 188 has the cleanest fp32 yardstick (4.0e-5 .. 5.6e-5; 258 flips a later
# decision between fp32 and fp64: 5.8e-3)
MODEL_SEED = 188


def stem_margin(y):
    """The smaller of (the smallest top-two gap over the live windows, the smallest |winner|) of IN(y) for y NCHW fp64 torch."""
    a = F.instance_norm(y, eps=EPS).numpy().transpose(0, 2, 3, 1)
    w = np.sort(_windows(a), 0)
    live = w[8] > 0
    gap = np.where(live, w[8] - w[7], np.inf).min()
    return float(min(gap, np.abs(w[8]).min()))


def _stem_tensors(B, H, W, seed):
    gen = torch.Generator().manual_seed(seed)
    x = torch.rand(B, 3, H, W, generator=gen)
    w = torch.randn(64, 3, 7, 7, generator=gen) * (2.0 / (64 * 49)) ** 0.5
    Hp, Wp = pooled_dims(*pooled_dims(H, W))
    return x, w, torch.randn(B, 64, Hp, Wp, generator=gen)


@functools.lru_cache(maxsize=None)
def stem_inputs(name):
    """(x NCHW fp32 in [0, 1), conv1_w, c NCHW fp32: loss = <c, stem(x)>) of a STEMS entry, its margin asserted."""
    _, B, H, W, seed = {s[0]: s for s in STEMS}[name]
    x, w, c = _stem_tensors(B, H, W, seed)
    assert stem_margin(F.conv2d(x.double(), w.double(), None, 2, 3)) >= MARGIN, name
    return x, w, c


def stem_weight_grad(x, w, c, dtype):
    """d <c, maxpool(relu(IN(conv(x, w))))> / dw by torch on the CPU in ``dtype``, as fp64 numpy."""
    w = w.to(dtype).requires_grad_(True)
    out = F.max_pool2d(torch.relu(F.instance_norm(F.conv2d(x.to(dtype), w, None, 2, 3), eps=EPS)), 3, 2, 1)
    return torch.autograd.grad((out * c.to(dtype)).sum(), w)[0].numpy().astype(np.float64)


def model_stem_margin(seed):
    """stem_margin of the whole-model check's fp64 stem map at ``seed`` (conv_bwd_cases.model_weight_grads' weights and inputs)."""
    import conv_bwd_cases as cc
    import dsmil  # noqa: F401
    from dsmil_wsi_amd.synthetic import make_patches, make_resnet18_weights
    w = torch.as_tensor(np.asarray(make_resnet18_weights(seed)["conv1.weight"])).double()
    x = torch.from_numpy(make_patches(seed + 1, cc.MODEL_B, cc.MODEL_HW, cc.MODEL_HW)).double()
    return stem_margin(F.conv2d(x, w, None, 2, 3))


def model_weight_grads_native(device, seed):
    """conv_bwd_cases.model_weight_grads (same seeded weights, inputs and functional) with use_native_stem + use_native_blocks."""
    import conv_bwd_cases as cc
    import dsmil  # noqa: F401
    from dsmil_wsi_amd import simclr
    from dsmil_wsi_amd.synthetic import make_patches
    model = nc._seeded_resnet18(seed).to(device).train()
    assert simclr.use_native_stem(model) == 1 and simclr.use_native_blocks(model) == 8
    x = torch.from_numpy(make_patches(seed + 1, cc.MODEL_B, cc.MODEL_HW, cc.MODEL_HW)).to(device)
    c = torch.from_numpy(np.random.default_rng(seed + 2).standard_normal((cc.MODEL_B, 512))).to(device=device, dtype=torch.float32)
    out = model(x)
    convs = [p for n, p in model.named_parameters() if p.dim() == 4]
    assert len(convs) == 20
    return [g.detach().cpu().numpy().astype(np.float64) for g in torch.autograd.grad((out * c).sum(), convs)]


# ---- the training stem's forward --------------------------------------------------------------------------------------------
# (B, H, W): one tile row; a second tile row whose pool row comes from the halo; odd sizes both ways.  Each as fp32 and as uint8.
FWD_SHAPES = [(1, 32, 32), (3, 34, 38), (2, 65, 33)]


@functools.lru_cache(maxsize=None)
def fwd_case(B, H, W, u8):
    """(x as the entry takes it, conv1_w with channel trunk32_cases.ZERO_CH zero — a constant channel, every window a tie —,
    the raw map's fp64 reference NHWC and its bar: trunk32_cases' stem bar before the pool)."""
    import trunk32_cases as tc
    rng = np.random.default_rng(_seed(f"fwd{B}x{H}x{W}{u8}"))
    x = rng.integers(0, 256, (B, H, W, 3), dtype=np.uint8) if u8 else rng.random((B, 3, H, W), dtype=np.float32)
    w = (rng.standard_normal((64, 3, 7, 7)) * (2.0 / (64 * 49)) ** 0.5).astype(np.float32)
    w[tc.ZERO_CH] = 0
    x64 = x.transpose(0, 3, 1, 2).astype(np.float64) / 255.0 if u8 else x.astype(np.float64)
    aw = np.abs(w.astype(np.float64))
    s = tc.conv64(x64, w, 2, 3)
    S = tc.conv64(np.abs(x64), aw, 2, 3)
    floor = 2.0 ** -25 * tc.conv64((x64 != 0).astype(np.float64), aw, 2, 3) + \
        2.0 ** -33 * tc.conv64(np.abs(x64), (aw != 0).astype(np.float64), 2, 3)
    bar = 1.01 * (3 * 147 + 8 + (1 if u8 else 0)) * U32 * S + floor
    return x, w, np.ascontiguousarray(s.transpose(0, 2, 3, 1)), np.ascontiguousarray(bar.transpose(0, 2, 3, 1))
