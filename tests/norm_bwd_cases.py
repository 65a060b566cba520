"""Shapes, seeded inputs, fp64 references, bars and a numpy emulation of the InstanceNorm / ReLU / residual-add backward kernels
(csrc/norm_bwd.hip behind dsmil_norm_bwd), shared by tests/test_norm_bwd_host.py (the emulation of the stated arithmetic meets
the bars, the mutants do not), tests/test_norm_bwd_cabi.py (the plan of every case is pinned) and tests/test_norm_bwd_gpu.py (the
kernels meet them).  Nothing here is tuned on a GPU or taken from the code under test; chunk, run_len, lanes and n_partials come
from the declared plan.

The function.  Maps are [B, HW, C] (NHWC), statistics [B, C].  For a raw map t with statistics (m, r), x^ = (t - m) r and a
masked upstream gradient q,
    INB(q; t, m, r) = r (q - mean_p q - x^ mean_p (q x^))
"relu": q = g where x^ > 0, gy = INB(q; y, m, r).  "add": q = g where the saved out > 0, gy as before, gres = q.  "add_down": as
"add", and gyd = INB(q; yd, md, rd).  The fp64 reference is this closed form over the SAME fp32 inputs, statistics and mask
included (closed_form); autograd_check() holds it against fp64 torch autograd with statistics computed in fp64.

The bar, per element.  u = 2^-24.  The kernel is specified (include/dsmil_hip.h) to compute, all in fp32,
    x^' = fl(fl(t - m) r)                                  |x^' - x^| <= 2 u |x^|
    S1 = sum q, S2 = sum fma(q, x^', .)                    each sum: a thread adds at most run_len terms serially, `lanes` such
                                                           sums are combined in a tree, n_partials chunk sums are added in order
    a' = fl(S1 / HW), b' = fl(S2 / HW)
    gy' = fl(r fma(-x^', b', fl(q - a')))
A term of a sum passes through at most D = run_len + lanes + n_partials additions, each rounding at most u times a partial sum
of absolute values, so with A1 = mean_p |q|, A2 = mean_p |q x^|, a = mean_p q, b = mean_p (q x^):
    |a' - a| <= (D + 1) u A1                               (the division adds one rounding)
    |b' - b| <= (D + 3) u A2                               (the terms carry x^''s 2 u)
    |fl(q - a') - (q - a)| <= |a' - a| + u |q - a|
    |t' - t| <= that + |x^| |b' - b| + 2 u |x^ b| + u |t|,   t = q - a - x^ b
    |gy' - gy| <= r |t' - t| + u |gy|
    bar = 1.01 u r [ (D + 1) A1 + |q - a| + |x^| ((D + 3) A2 + 2 |b|) + 2 |t| ] + 4 * 2^-149 max(r, 1)
"1.01" pays for the second-order terms (as in trunk32_cases); the last term is a few subnormal steps.  gres = q is a copy: it
must be exact.  Where q, a and b vanish (HW = 1 with m = y, a fully masked channel, g = 0) every operation above is exact and
the result is an exact zero.

EXACT cases.  y, g, m (and out, yd, md) integer-valued, r a power of two, HW a power of two: every x^, product, partial sum in
any order, mean and the final fma are dyadic rationals of fewer than 24 significant bits (checked by the builder), so fp32
holds them exactly and the result equals the fp64 reference bit for bit."""
import functools

import numpy as np
import torch
import torch.nn.functional as F

from trunk32_cases import U32, worst  # noqa: F401

EPS = 1e-5
KINDS = ("relu", "add", "add_down")
# (name, kind, B, HW, C, g magnitude).  The chunk of every case is 256 pixels (pinned in PLANS).
CASES = [
    ("r_hw1", "relu", 3, 1, 64, 1.0), ("a_hw1", "add", 1, 1, 128, 1e-6), ("d_hw1", "add_down", 3, 1, 64, 1.0),
    ("r_35", "relu", 3, 35, 64, 1e-6), ("a_35", "add", 1, 35, 128, 1.0), ("d_35", "add_down", 3, 35, 512, 1e-6),   # 7 x 5
    ("r_256", "relu", 1, 256, 64, 1.0), ("a_256", "add", 3, 256, 128, 1e-6),                      # one full chunk
    ("a_257", "add", 3, 257, 64, 1e-6), ("d_257", "add_down", 1, 257, 128, 1.0),                  # a chunk and one pixel
    ("r_257", "relu", 1, 257, 512, 1e-6),
    ("r_700", "relu", 3, 700, 64, 1.0), ("a_600", "add", 1, 600, 512, 1.0), ("d_700", "add_down", 1, 700, 64, 1e-6),   # 3 partials
    ("r_2048", "relu", 1, 35, 2048, 1.0), ("a_2048", "add", 3, 35, 2048, 1e-6), ("d_2048", "add_down", 1, 257, 2048, 1.0),
]
# name: (chunk, n_partials, run_len, lanes, n_sums, grid_partial, grid_finish, grid_apply, groups)
PLANS = {
    "r_hw1": (256, 1, 1, 16, 2, 3, 2, 1, 1), "a_hw1": (256, 1, 1, 8, 2, 1, 1, 1, 1), "d_hw1": (256, 1, 1, 16, 3, 3, 3, 1, 1),
    "r_35": (256, 1, 3, 16, 2, 3, 2, 7, 1), "a_35": (256, 1, 5, 8, 2, 1, 1, 5, 1), "d_35": (256, 1, 18, 2, 3, 3, 18, 53, 1),
    "r_256": (256, 1, 16, 16, 2, 1, 1, 16, 1), "a_256": (256, 1, 32, 8, 2, 3, 3, 96, 1),
    "a_257": (256, 2, 16, 16, 2, 6, 2, 49, 1), "d_257": (256, 2, 32, 8, 3, 2, 2, 33, 1),
    "r_257": (256, 2, 128, 2, 2, 2, 4, 129, 1),
    "r_700": (256, 3, 16, 16, 2, 9, 2, 132, 1), "a_600": (256, 3, 128, 2, 2, 3, 4, 300, 1), "d_700": (256, 3, 16, 16, 3, 3, 1, 44, 1),
    "r_2048": (256, 1, 35, 1, 2, 1, 16, 35, 2), "a_2048": (256, 1, 35, 1, 2, 3, 48, 105, 2), "d_2048": (256, 2, 256, 1, 3, 2, 24, 257, 2),
}
# (name, kind, B, HW, C)
EXACT_CASES = [("x_relu", "relu", 2, 64, 64), ("x_add", "add", 2, 512, 64), ("x_down", "add_down", 1, 64, 128),
               ("x_relu_2048", "relu", 1, 16, 2048)]
BY_NAME = {c[0]: c for c in CASES + EXACT_CASES}
MASKED_CH = 5                    # in image 0 every element of this channel is masked
MUTANTS = ("drop_xhat_term", "drop_mean_q", "drop_rstd", "mask_from_g", "down_uses_main_stats")


def _seed(name):
    return 7100 + sum((i + 1) * ord(ch) for i, ch in enumerate(name))


def lanes_of(C):
    return 256 // min(C // 4, 256)


def plan_of(kind, B, HW, C, chunk=256):
    """(chunk, n_partials, run_len, lanes) the documented rule gives for a case whose chunk is ``chunk``."""
    lanes = lanes_of(C)
    return chunk, -(-HW // chunk), -(-min(HW, chunk) // lanes), lanes


# ---- fp64 -------------------------------------------------------------------------------------------------------------------
def _xhat64(t, m, r):
    return (np.asarray(t, np.float64) - np.asarray(m, np.float64)[:, None, :]) * np.asarray(r, np.float64)[:, None, :]


def _inb64(q, xh, r, D):
    """(INB in fp64, its bar) for q, x^ [B, HW, C] fp64 and r [B, C]."""
    r = np.asarray(r, np.float64)[:, None, :]
    a, b = q.mean(1, keepdims=True), (q * xh).mean(1, keepdims=True)
    A1, A2 = np.abs(q).mean(1, keepdims=True), np.abs(q * xh).mean(1, keepdims=True)
    t = q - a - xh * b
    bar = 1.01 * U32 * r * ((D + 1) * A1 + np.abs(q - a) + np.abs(xh) * ((D + 3) * A2 + 2 * np.abs(b)) + 2 * np.abs(t)) + \
        4 * 2.0 ** -149 * np.maximum(r, 1.0)
    return r * t, bar


def closed_form(kind, inp, run_len=1, lanes=1, n_partials=1):
    """{"gy": (ref, bar), "gres": (ref, None) | "gyd": (ref, bar)} in fp64 over the fp32 inputs of ``inp``."""
    D = run_len + lanes + n_partials
    g = np.asarray(inp["g"], np.float64)
    xh = _xhat64(inp["y"], inp["m"], inp["r"])
    mask = xh > 0 if kind == "relu" else np.asarray(inp["out"]) > 0
    q = np.where(mask, g, 0.0)
    res = {"gy": _inb64(q, xh, inp["r"], D)}
    if kind == "add":
        res["gres"] = (q, None)
    if kind == "add_down":
        res["gyd"] = _inb64(q, _xhat64(inp["yd"], inp["md"], inp["rd"]), inp["rd"], D)
    return res


def _stats64(t):
    t = np.asarray(t, np.float64)
    return t.mean(1), 1.0 / np.sqrt(t.var(1) + EPS)


def autograd_check(kind, B=2, HW=35, C=8, seed=3):
    """Largest |closed form - fp64 autograd| over the outputs, relative to the largest gradient: statistics computed in fp64
    from y itself (and yd), the function differentiated by torch in float64 on the CPU."""
    rng = np.random.default_rng(seed)
    y, yd, idn = (rng.standard_normal((B, HW, C)) * s + o for s, o in ((1.5, 0.3), (0.7, -0.2), (1.0, 0.0)))
    g = rng.standard_normal((B, HW, C))
    nchw = lambda t: torch.from_numpy(np.ascontiguousarray(t.transpose(0, 2, 1)[..., None])).requires_grad_(True)
    back = lambda t: t.numpy()[..., 0].transpose(0, 2, 1)
    ty, tyd, tid = nchw(y), nchw(yd), nchw(idn)
    ny = F.instance_norm(ty, eps=EPS)
    if kind == "relu":
        out, wrt = torch.relu(ny), (ty,)
    elif kind == "add":
        out, wrt = torch.relu(ny + tid), (ty, tid)
    else:
        out, wrt = torch.relu(ny + F.instance_norm(tyd, eps=EPS)), (ty, tyd)
    grads = [back(t) for t in torch.autograd.grad(out, wrt, nchw(g).detach())]
    m, r = _stats64(y)
    md, rd = _stats64(yd)
    inp = dict(g=g, y=y, m=m, r=r, out=back(out.detach()), yd=yd, md=md, rd=rd)
    res = closed_form(kind, inp)
    mine = [res["gy"][0]] + ([res["gres"][0]] if kind == "add" else [res["gyd"][0]] if kind == "add_down" else [])
    return max(float(np.abs(a - b).max()) for a, b in zip(mine, grads)) / max(float(np.abs(t).max()) for t in grads)


# ---- inputs -----------------------------------------------------------------------------------------------------------------
def _f32(*ts):
    return tuple(np.ascontiguousarray(t, np.float32) for t in ts)


@functools.lru_cache(maxsize=None)
def case(name):
    """The fp32 inputs of a CASES entry as a dict: g, y, m, r (+ out for "add" / "add_down", + yd, md, rd for "add_down").
    y is normal at 1.5 around 0.3, its statistics are its own (fp64, rounded to fp32); with HW = 1 the mean is y itself.  g is
    normal at the case's magnitude with a tenth of its elements exactly zero.  out is the fp32 forward relu(x^ + idn | x^d).
    In image 0 channel MASKED_CH is fully masked (out = 0 there; "relu": its mean lies above every element).
    "relu": y is moved off its mean until |x^| >= 1e-3 (or x^ == 0 exactly, HW = 1), so that an fp32 and an fp64 evaluation of
    the mask agree on every sign — asserted here."""
    _, kind, B, HW, C, mag = BY_NAME[name]
    rng = np.random.default_rng(_seed(name))
    y = (rng.standard_normal((B, HW, C)) * 1.5 + 0.3).astype(np.float32)
    m, r = _f32(*_stats64(y))
    g = rng.standard_normal((B, HW, C)) * mag
    g = np.where(rng.random(g.shape) < 0.1, 0.0, g).astype(np.float32)
    inp = dict(g=g, y=y, m=m, r=r)
    if kind == "relu":
        if HW > 1:
            m[0, MASKED_CH] = y[0, :, MASKED_CH].max() + 1.0
            xh = _xhat64(y, m, r)
            near = np.abs(xh) < 2e-3
            y[near] = (m[:, None, :] + np.where(xh >= 0, 4e-3, -4e-3) / r[:, None, :]).astype(np.float32)[near]
        xh = _xhat64(y, m, r)
        assert np.all((np.abs(xh) >= 1e-3) | (xh == 0)), name
        x32 = ((y - m[:, None, :]).astype(np.float32) * r[:, None, :]).astype(np.float32)
        assert np.array_equal(x32 > 0, xh > 0), name
        assert HW == 1 or not (x32[0, :, MASKED_CH] > 0).any()
    else:
        x32 = ((y - m[:, None, :]).astype(np.float32) * r[:, None, :]).astype(np.float32)
        if kind == "add":
            other = np.maximum(rng.standard_normal((B, HW, C)), 0).astype(np.float32)
        else:
            yd = (rng.standard_normal((B, HW, C)) * 0.7 - 0.2).astype(np.float32)
            md, rd = _f32(*_stats64(yd))
            other = ((yd - md[:, None, :]).astype(np.float32) * rd[:, None, :]).astype(np.float32)
            inp.update(yd=yd, md=md, rd=rd)
        out = np.maximum((x32 + other).astype(np.float32), np.float32(0))
        out[0, :, MASKED_CH] = 0
        inp["out"] = out
    for t in inp.values():
        t.setflags(write=False)
    return inp


@functools.lru_cache(maxsize=None)
def expected(name):
    _, kind, B, HW, C, _ = BY_NAME[name]
    chunk, n_partials, run_len, lanes = PLANS[name][:4]
    return closed_form(kind, case(name), run_len, lanes, n_partials)


@functools.lru_cache(maxsize=None)
def exact_case(name):
    """(inputs, {output: fp64 reference == its fp32 value}) of an EXACT_CASES entry."""
    _, kind, B, HW, C = BY_NAME[name]
    rng = np.random.default_rng(_seed(name))
    ints = lambda lo, hi, shape: rng.integers(lo, hi + 1, shape).astype(np.float32)
    pow2 = lambda shape: (2.0 ** rng.integers(-1, 2, shape)).astype(np.float32)
    inp = dict(g=ints(-3, 3, (B, HW, C)), y=ints(-4, 4, (B, HW, C)), m=ints(-1, 1, (B, C)), r=pow2((B, C)))
    if kind != "relu":
        inp["out"] = np.maximum(ints(-3, 3, (B, HW, C)), 0)
    if kind == "add_down":
        inp.update(yd=ints(-4, 4, (B, HW, C)), md=ints(-1, 1, (B, C)), rd=pow2((B, C)))
    ref = {k: v[0] for k, v in closed_form(kind, inp).items()}
    for k, v in ref.items():
        assert np.array_equal(v.astype(np.float32).astype(np.float64), v), (name, k)
    # every intermediate is a multiple of 2^-11 below 2^12 (x^ of 2^-1 below 2^4, the means of 2^-10 below 2^7): < 24 bits
    assert HW & (HW - 1) == 0 and HW <= 512
    for t in inp.values():
        t.setflags(write=False)
    return inp, ref


# ---- the numpy emulation of the stated arithmetic ---------------------------------------------------------------------------
def _fma32(a, b, c):
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def _sum_pixels(terms, chunk, lanes, C, fma_with=None):
    """[B, C] fp32: sum over the pixels of ``terms`` [B, HW, C] (or of terms * fma_with, fused) in the kernel's order."""
    B, HW, _ = terms.shape
    lanes_c = min(C // 4, 256)
    total = None
    for p0 in range(0, HW, chunk):
        p1 = min(HW, p0 + chunk)
        acc = np.zeros((B, lanes, C), np.float32)
        for i in range(-(-(p1 - p0) // lanes)):                         # a thread's serial run
            sl = slice(p0 + i * lanes, min(p1, p0 + (i + 1) * lanes))
            n = sl.stop - sl.start
            if fma_with is None:
                acc[:, :n] = (acc[:, :n] + terms[:, sl]).astype(np.float32)
            else:
                acc[:, :n] = _fma32(terms[:, sl], fma_with[:, sl], acc[:, :n])
        if lanes_c < 64:                                               # xor shuffles inside each of the 4 waves, nearest first
            acc = acc.reshape(B, 4, lanes // 4, C)
            while acc.shape[2] > 1:
                acc = (acc[:, :, 0::2] + acc[:, :, 1::2]).astype(np.float32)
            acc = acc[:, :, 0]
        part = acc[:, 0]
        for k in range(1, acc.shape[1]):                               # the LDS rows in order
            part = (part + acc[:, k]).astype(np.float32)
        total = part if total is None else (total + part).astype(np.float32)
    return total


def emulate(kind, inp, chunk=256, mutant=None):
    """The outputs (fp32, a dict like closed_form's) by the stated arithmetic and order."""
    g, y = np.asarray(inp["g"], np.float32), np.asarray(inp["y"], np.float32)
    B, HW, C = y.shape
    lanes = lanes_of(C)
    xhat = lambda t, m, r: ((t - np.asarray(m, np.float32)[:, None, :]).astype(np.float32) * np.asarray(r, np.float32)[:, None, :]).astype(np.float32)
    xh = xhat(y, inp["m"], inp["r"])
    mask = g > 0 if mutant == "mask_from_g" else xh > 0 if kind == "relu" else np.asarray(inp["out"]) > 0
    q = np.where(mask, g, np.float32(0)).astype(np.float32)
    hw = np.float32(HW)
    mq = (_sum_pixels(q, chunk, lanes, C) / hw).astype(np.float32)[:, None, :]
    if mutant == "drop_mean_q":
        mq = np.zeros_like(mq)
    d = (q - mq).astype(np.float32)

    def inb(xh, r):
        mqx = (_sum_pixels(q, chunk, lanes, C, fma_with=xh) / hw).astype(np.float32)[:, None, :]
        if mutant == "drop_xhat_term":
            mqx = np.zeros_like(mqx)
        t = _fma32(-xh, np.broadcast_to(mqx, xh.shape), d)
        return t if mutant == "drop_rstd" else (np.asarray(r, np.float32)[:, None, :] * t).astype(np.float32)

    res = {"gy": inb(xh, inp["r"])}
    if kind == "add":
        res["gres"] = q
    if kind == "add_down":
        st = (inp["m"], inp["r"]) if mutant == "down_uses_main_stats" else (inp["md"], inp["rd"])
        res["gyd"] = inb(xhat(np.asarray(inp["yd"], np.float32), *st), st[1])
    return res


def worst_ratio(got, exp):
    """Largest err / bar over the outputs of one call; gres (no bar) must be exact."""
    w = 0.0
    for k, (ref, bar) in exp.items():
        a = np.asarray(got[k], np.float64)
        assert a.shape == ref.shape, k
        if bar is None:
            w = max(w, 0.0 if np.array_equal(a, ref) else float("inf"))
        else:
            w = max(w, worst(np.abs(a - ref), bar))
    return w


# ---- the block- and model-level checks --------------------------------------------------------------------------------------
# (name, inplanes, planes, stride, H, W), B = 2
BLOCKS = [("id_64", 64, 64, 1, 8, 6), ("down_128", 64, 128, 2, 9, 7), ("id_256", 256, 256, 1, 4, 4)]
BLOCK_B = 2


def make_block(name, norm="instance", bias=False):
    """A seeded resnet.BasicBlock (fp32, CPU) of a BLOCKS entry, kaiming-normal(fan_out) weights."""
    import torch.nn as nn
    import dsmil  # noqa: F401
    from dsmil_wsi_amd.resnet import BasicBlock
    _, cin, planes, stride, H, W = {b[0]: b for b in BLOCKS}[name]
    norm_layer = nn.InstanceNorm2d if norm == "instance" else nn.BatchNorm2d
    down = None
    if stride != 1 or cin != planes:
        down = nn.Sequential(nn.Conv2d(cin, planes, 1, stride, bias=False), norm_layer(planes))
    blk = BasicBlock(cin, planes, stride, down, norm_layer)
    if bias:
        blk.conv2 = nn.Conv2d(planes, planes, 3, 1, 1, bias=True)
    gen = torch.Generator().manual_seed(_seed(name))
    with torch.no_grad():
        for p in blk.parameters():
            if p.dim() == 4:
                p.copy_(torch.randn(p.shape, generator=gen) * (2.0 / (p.shape[0] * p.shape[2] * p.shape[3])) ** 0.5)
    return blk


def block_inputs(name):
    """(x NCHW fp32 >= 0 as a block's input is, c NCHW fp32: loss = <c, block(x)>)."""
    _, cin, planes, stride, H, W = {b[0]: b for b in BLOCKS}[name]
    gen = torch.Generator().manual_seed(_seed(name) + 1)
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    return torch.randn(BLOCK_B, cin, H, W, generator=gen).relu_(), torch.randn(BLOCK_B, planes, Ho, Wo, generator=gen)


def grad_fn_names(out):
    """The names of out.grad_fn and of the nodes it reads (the native block's output is an NCHW view of the Function's)."""
    fn = out.grad_fn
    return " ".join([type(fn).__name__] + [type(f[0]).__name__ for f in fn.next_functions if f[0] is not None])


def block_grads(blk, x, c):
    """([dx, dw...] as fp64 numpy in parameter order, grad_fn_names of the output) of loss = <c, blk(x)>."""
    x = x.detach().clone().requires_grad_(True) if not x.requires_grad else x
    out = blk(x)
    params = [p for p in blk.parameters() if p.dim() == 4]
    grads = torch.autograd.grad((out * c).sum(), [x] + params)
    return [t.detach().cpu().numpy().astype(np.float64) for t in grads], grad_fn_names(out)


@functools.lru_cache(maxsize=None)
def block_yardstick(name):
    """(g64, rel) of a BLOCKS entry: the fp64 CPU gradients and ||g32 - g64|| / ||g64|| of the plain fp32 CPU block."""
    blk = make_block(name)
    x, c = block_inputs(name)
    g32, _ = block_grads(blk, x, c)
    g64, _ = block_grads(blk.double(), x.double(), c.double())
    return g64, rel_errors(g32, g64)


def rel_errors(gs, g64):
    return [float(np.linalg.norm(g - r) / np.linalg.norm(r)) for g, r in zip(gs, g64)]


def _seeded_resnet18(seed):
    import torch.nn as nn
    import dsmil  # noqa: F401
    from dsmil_wsi_amd.resnet import resnet18
    from dsmil_wsi_amd.synthetic import make_resnet18_weights
    model = resnet18(norm_layer=nn.InstanceNorm2d)
    model.fc = nn.Identity()
    model.load_state_dict({k: torch.as_tensor(np.asarray(v)) for k, v in make_resnet18_weights(seed).items()}, strict=True)
    return model


def _swap(model):
    import dsmil  # noqa: F401
    from dsmil_wsi_amd import simclr
    assert simclr.use_native_blocks(model) == 8 and simclr.use_native_convs(model) == 20
    return model


def model_weight_grads_native(device):
    """conv_bwd_cases.model_weight_grads (same seeded weights, inputs and functional) with use_native_blocks + use_native_convs."""
    import conv_bwd_cases as cc
    from dsmil_wsi_amd.synthetic import make_patches
    seed = cc.MODEL_SEED
    model = _swap(_seeded_resnet18(seed).to(device).train())
    x = torch.from_numpy(make_patches(seed + 1, cc.MODEL_B, cc.MODEL_HW, cc.MODEL_HW)).to(device)
    c = torch.from_numpy(np.random.default_rng(seed + 2).standard_normal((cc.MODEL_B, 512))).to(device=device, dtype=torch.float32)
    out = model(x)
    convs = [p for n, p in model.named_parameters() if p.dim() == 4]
    assert len(convs) == 20
    return [g.detach().cpu().numpy().astype(np.float64) for g in torch.autograd.grad((out * c).sum(), convs)]


# one SimCLR step: SIMCLR_PAIRS pairs of 64 x 64 views through the trunk, Linear - ReLU - Linear, F.normalize, NT-Xent
SIMCLR_SEED, SIMCLR_PAIRS, SIMCLR_HW, SIMCLR_T = 5, 4, 64, 0.5


def simclr_step(dtype, device="cpu", native=False):
    """(loss as a float, the gradients of the 20 conv weights and the 4 head parameters as fp64 numpy)."""
    import torch.nn as nn
    import dsmil  # noqa: F401
    from dsmil_wsi_amd import simclr
    from dsmil_wsi_amd.synthetic import make_patches
    trunk = _seeded_resnet18(SIMCLR_SEED)
    torch.manual_seed(SIMCLR_SEED)
    head = nn.Sequential(nn.Linear(512, 512), nn.ReLU(), nn.Linear(512, 128))
    model = nn.Sequential(trunk, head).to(device=device, dtype=dtype).train()
    if native:
        _swap(model[0])
    x = torch.from_numpy(make_patches(SIMCLR_SEED + 1, 2 * SIMCLR_PAIRS, SIMCLR_HW, SIMCLR_HW)).to(device=device, dtype=dtype)
    z = F.normalize(model(x), dim=1)
    loss = simclr.NTXentLoss(device, SIMCLR_PAIRS, SIMCLR_T, True)(z[:SIMCLR_PAIRS].contiguous(), z[SIMCLR_PAIRS:].contiguous())
    params = [p for p in model[0].parameters() if p.dim() == 4] + list(model[1].parameters())
    assert len(params) == 24
    grads = torch.autograd.grad(loss, params)
    return float(loss.detach()), [g.detach().cpu().numpy().astype(np.float64) for g in grads]


@functools.lru_cache(maxsize=None)
def simclr_yardstick():
    """(loss64, g64, rel) of the fp64 CPU step and of the plain fp32 CPU step against it."""
    l64, g64 = simclr_step(torch.float64)
    _, g32 = simclr_step(torch.float32)
    return l64, g64, rel_errors(g32, g64)
