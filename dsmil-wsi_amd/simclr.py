"""SimCLR pre-training of the embedder: the NT-Xent loss (simclr/loss/nt_xent.py of the reference) without its
[2N, 2N, D] broadcast product.

With R = cat([zjs, zis]) (nt_xent.py:48), M = 2N, p(a) = (a + N) mod M and S = R^ R^T (cosine similarity, R^ the rows over
max(norm, 1e-8)) or R R^T (dot), the reference's value is

    loss = (1/M) sum_a [ logsumexp_{b != a}(S_ab / T) - S_{a,p(a)} / T ]

(its [positives | negatives] logits with label 0 are exactly "all columns but the diagonal"), and its gradient is
dR^ = (P + P^T - 2 Pi) R^ / (M T) with P_ab = exp(S_ab / T - lse_a), P_aa = 0, Pi the permutation matrix of p, followed for
the cosine form by dR_a = (dR^_a - R^_a (R^_a . dR^_a)) / |R_a|.  Contiguous fp32 device tensors take the fused HIP kernels
(csrc/ntxent.hip: O(N D) memory, no host synchronisation); everything else takes the same closed form from torch ops, in
row blocks, so no path forms more than a [block, M] slab."""
import torch

from . import ops, resnet

_CHUNK = 1024      # rows per slab of the composite path


def _unit_rows(R, cosine):
    if not cosine:
        return R, None
    nrm = R.norm(dim=1, keepdim=True).clamp_min(1e-8)      # torch.nn.CosineSimilarity's eps, per operand
    return R / nrm, nrm


def ntxent_composite(zis, zjs, temperature, cosine=True):
    """The closed form from torch ops, differentiable by autograd, for any device and floating dtype.  Walks the rows in
    blocks of 1024: memory O(1024 x 2N) beside the inputs."""
    R = torch.cat([zjs, zis], dim=0)
    M, N = R.shape[0], zis.shape[0]
    Rh, _ = _unit_rows(R, cosine)
    total = R.new_zeros(())
    for a0 in range(0, M, _CHUNK):
        a1 = min(M, a0 + _CHUNK)
        rows = torch.arange(a0, a1, device=R.device)
        z = (Rh[a0:a1] @ Rh.t()) / temperature
        pos = z[rows - a0, (rows + N) % M]
        z = z.masked_fill(rows[:, None] == torch.arange(M, device=R.device)[None, :], float("-inf"))
        total = total + (torch.logsumexp(z, dim=1) - pos).sum()
    return total / M


class _NTXentNative(torch.autograd.Function):
    """The two native calls; saves the inputs and the rows' log-sum-exp only."""

    @staticmethod
    def forward(ctx, zis, zjs, temperature, cosine):
        loss, lse = ops.ntxent_forward(zis, zjs, temperature, cosine)
        ctx.save_for_backward(zis, zjs, lse)
        ctx.temperature, ctx.cosine = temperature, cosine
        return loss

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_loss):
        zis, zjs, lse = ctx.saved_tensors
        g_zis, g_zjs = ops.ntxent_backward(zis, zjs, ctx.temperature, lse, g_loss.to(torch.float32), ctx.cosine)
        return g_zis, g_zjs, None, None


def _native_ok(zis, zjs):
    return (zis.is_cuda and zjs.is_cuda and zis.device == zjs.device and zis.dtype == torch.float32 and
            zjs.dtype == torch.float32 and zis.dim() == 2 and zis.shape == zjs.shape and zis.is_contiguous() and
            zjs.is_contiguous() and 1 <= zis.shape[0] <= 65536 and 1 <= zis.shape[1] <= 4096)


class NTXentLoss(torch.nn.Module):
    """Drop-in for the reference's ``loss.nt_xent.NTXentLoss(device, batch_size, temperature, use_cosine_similarity)``.

    ``forward(zis, zjs)`` returns the scalar loss.  N is read from the input: the reference builds a fixed
    [2 batch_size, 2 batch_size] mask, which makes a short last batch an error (its loader drops it); this module accepts
    any N >= 1, ``batch_size`` is kept for the signature only."""

    def __init__(self, device, batch_size, temperature, use_cosine_similarity):
        super().__init__()
        self.device = device
        self.batch_size = batch_size
        self.temperature = float(temperature)
        self.use_cosine_similarity = bool(use_cosine_similarity)

    def forward(self, zis, zjs):
        if zis.dim() != 2 or zis.shape != zjs.shape:
            raise ValueError(f"zis and zjs must be [N, D] tensors of one shape (got {tuple(zis.shape)}, {tuple(zjs.shape)})")
        if _native_ok(zis, zjs):
            return _NTXentNative.apply(zis, zjs, self.temperature, self.use_cosine_similarity)
        return ntxent_composite(zis, zjs, self.temperature, self.use_cosine_similarity)


# ---------------------------------------------------------------------------------------------------------------------------
# the two-view augmentation (simclr/data_aug/dataset_wrapper.py:48-58, SimCLRDataTransform :80-87) on decoded tiles
# ---------------------------------------------------------------------------------------------------------------------------
class ViewParams:
    """One record per output view (struct dsmil_simclr_view), held as ONE buffer: ``records`` int32 [n, 12], of which ``ints``
    = columns 0..7 (tile, i, j, h, w, flags, order, hue byte) and ``floats`` = columns 8..11 seen as float32 (brightness,
    contrast, saturation, sigma) are views.  Pinned when CUDA is available, so the upload is one asynchronous copy.

    The constructor takes explicit values, each a scalar or a sequence of n: ``order`` is the jitter's order, [4] or [n, 4], a
    permutation of 0 brightness, 1 contrast, 2 saturation, 3 hue; ``hue`` is the BYTE added to H, trunc(hue_factor * 255)
    mod 256."""

    def __init__(self, tile, i, j, h, w, flip=False, jitter=False, grey=False, blur=False, order=(0, 1, 2, 3), brightness=1.0,
                 contrast=1.0, saturation=1.0, hue=0, sigma=1.0):
        tile = torch.as_tensor(tile, dtype=torch.int64).reshape(-1)
        n = tile.numel()
        self.records = torch.empty((n, 12), dtype=torch.int32, pin_memory=torch.cuda.is_available())
        self.ints = self.records[:, :8]
        self.floats = self.records[:, 8:].view(torch.float32)

        def col(x, dtype):
            x = torch.as_tensor(x).to(dtype).reshape(-1)
            return x.expand(n) if x.numel() == 1 else x.reshape(n)

        flags = (col(flip, torch.bool).int() * ops.SIMCLR_FLIP + col(jitter, torch.bool).int() * ops.SIMCLR_JITTER +
                 col(grey, torch.bool).int() * ops.SIMCLR_GREY + col(blur, torch.bool).int() * ops.SIMCLR_BLUR)
        order = torch.as_tensor(order, dtype=torch.int64).reshape(-1, 4)
        packed = (order << torch.tensor([0, 2, 4, 6])).sum(1).expand(n)
        for k, x in enumerate((tile, i, j, h, w, flags, packed, hue)):
            self.ints[:, k] = col(x, torch.int32)
        for k, x in enumerate((brightness, contrast, saturation, sigma)):
            self.floats[:, k] = col(x, torch.float32)

    def __len__(self):
        return self.records.shape[0]

    def order(self):
        """[n, 4]: the jitter operation at each position."""
        return torch.stack([(self.ints[:, 6] >> (2 * k)) & 3 for k in range(4)], 1)


def draw_view_params(n_tiles, H, W, size, s=1.0, generator=None):
    """The random parameters of SimCLR's transform pipeline for 2 n_tiles views (records 2k and 2k + 1 are the two views of
    tile k), drawn with torchvision's distributions: RandomResizedCrop.get_params (scale (0.08, 1), ratio (3/4, 4/3), ten
    tries, then the centre crop clamped to the ratio range), flip p = 0.5, ColorJitter(0.8s, 0.8s, 0.8s, 0.2s) applied with
    p = 0.8 in a uniformly random order, greyscale p = 0.2, blur p = 0.5 with sigma = U(0.1, 2.0).  ``generator``: a CPU
    torch.Generator (default: the global one).  ``size`` does not enter the draw (nor does it in torchvision's get_params); it
    is part of the signature because it belongs to the transform being drawn for.  The reference mixes torch's and numpy's global streams, so its stream is not
    reproduced; the distributions are."""
    import math
    n = 2 * int(n_tiles)
    H, W, s = int(H), int(W), float(s)

    def U(*shape):
        return torch.rand(*shape, generator=generator, dtype=torch.float64)

    area = H * W * (0.08 + (1.0 - 0.08) * U(n, 10))
    lo, hi = math.log(3.0 / 4.0), math.log(4.0 / 3.0)
    ratio = torch.exp(lo + (hi - lo) * U(n, 10))
    w_try = torch.round(torch.sqrt(area * ratio)).long()
    h_try = torch.round(torch.sqrt(area / ratio)).long()
    ok = (w_try > 0) & (w_try <= W) & (h_try > 0) & (h_try <= H)
    first = torch.argmax(ok.int(), dim=1)                       # the first accepted try
    any_ok = ok.any(dim=1)
    rows = torch.arange(n)
    w, h = w_try[rows, first], h_try[rows, first]
    i = torch.floor(U(n) * (H - h + 1).clamp_min(1)).long().clamp(max=H - 1)
    j = torch.floor(U(n) * (W - w + 1).clamp_min(1)).long().clamp(max=W - 1)
    in_ratio = W / H                                            # the fallback: the whole tile, clamped to the ratio range
    if in_ratio < 3.0 / 4.0:
        fw, fh = W, int(round(W / (3.0 / 4.0)))
    elif in_ratio > 4.0 / 3.0:
        fh, fw = H, int(round(H * (4.0 / 3.0)))
    else:
        fw, fh = W, H
    fw, fh = min(fw, W), min(fh, H)
    w = torch.where(any_ok, w, torch.tensor(fw))
    h = torch.where(any_ok, h, torch.tensor(fh))
    i = torch.where(any_ok, torch.minimum(i, H - h), torch.tensor((H - fh) // 2))
    j = torch.where(any_ok, torch.minimum(j, W - w), torch.tensor((W - fw) // 2))
    flip = U(n) < 0.5
    jitter = U(n) < 0.8
    f_lo, f_hi = max(0.0, 1.0 - 0.8 * s), 1.0 + 0.8 * s
    factors = f_lo + (f_hi - f_lo) * U(n, 3)
    hue = (-0.2 * s + 0.4 * s * U(n))
    hue_byte = torch.trunc(hue * 255).long() % 256
    order = torch.argsort(U(n, 4), dim=1)
    grey = U(n) < 0.2
    blur = U(n) < 0.5
    sigma = 0.1 + 1.9 * U(n)
    return ViewParams(torch.arange(n) // 2, i, j, h, w, flip, jitter, grey, blur, order, factors[:, 0], factors[:, 1],
                      factors[:, 2], hue_byte, sigma)


class TwoViewAugment:
    """SimCLRDataTransform over a batch of decoded tiles: ``aug(tiles_u8_nhwc) -> (xis, xjs)``, each [n, 3, S, S] fp32
    (``out="float"``, what ToTensor gives) or [n, S, S, 3] uint8 (``out="uint8"``, what the repository's trunk ingests).  Draws
    the parameters on the host (draw_view_params), launches ops.simclr_views once; xis / xjs are the even / odd views of that
    one output, nothing is copied.  ``last_params`` holds the parameters of the last call."""

    def __init__(self, size=224, s=1.0, generator=None, out="float"):
        if int(0.06 * int(size)) % 2 != 1 or not 17 <= int(size) <= 256:
            raise ValueError(f"size {size}: the blur kernel int(0.06 size) = {int(0.06 * int(size))} must be odd, 17 <= size <= 256")
        if out not in ("float", "uint8"):
            raise ValueError('out must be "float" or "uint8"')
        self.size, self.s, self.generator, self.out = int(size), float(s), generator, out
        self.last_params = None

    def __call__(self, tiles_u8_nhwc):
        n, H, W, _ = tiles_u8_nhwc.shape
        self.last_params = draw_view_params(n, H, W, self.size, self.s, self.generator)
        views = ops.simclr_views(tiles_u8_nhwc, self.last_params, self.size, out=self.out)
        return views[0::2], views[1::2]


# ---------------------------------------------------------------------------------------------------------------------------
# training the embedder: the convs' backward on the native kernels (csrc/conv_bwd.hip).  OPT-IN: nothing here is called by
# default, and the native inference route of IClassifier does not pass through these modules' forward.
# ---------------------------------------------------------------------------------------------------------------------------
def _same2(v):
    """The int both entries of a conv's (a, a) geometry pair share, else None (strings such as padding="same" included)."""
    if isinstance(v, int):
        return v
    if isinstance(v, (tuple, list)) and len(v) == 2 and all(isinstance(t, int) for t in v) and v[0] == v[1]:
        return v[0]
    return None


def _conv_geometry(m):
    """(ks, stride, pad) of a bias-free, ungrouped, undilated, zero-padded square conv, else None."""
    ks, stride, pad, dil = _same2(m.kernel_size), _same2(m.stride), _same2(m.padding), _same2(m.dilation)
    if m.bias is not None or m.groups != 1 or dil != 1 or m.padding_mode != "zeros" or None in (ks, stride, pad):
        return None
    return ks, stride, pad


def _nhwc(x):
    """The NHWC view of an NCHW tensor: no copy where x is ``channels_last``, else one."""
    xp = x.permute(0, 2, 3, 1)
    return xp if xp.is_contiguous() else xp.contiguous()


def _swap_children(model, eligible, make):
    """Replaces every module m under ``model`` with ``eligible(m)`` by ``make(m)``, in m's training mode; returns how many."""
    swapped = 0
    for parent in list(model.modules()):
        for name, m in list(parent.named_children()):
            if eligible(m):
                setattr(parent, name, make(m).train(m.training))
                swapped += 1
    return swapped


class _ConvNative(torch.autograd.Function):
    """y = conv(x, w) on NHWC fp32 maps.  Forward: ops.trunk32_conv (the fp32-class trunk's kernels) where it takes the shape;
    the stem (Cin = 3), which that entry leaves to the fused stem kernel, runs aten's conv.  Backward: ops.conv_backward_data /
    conv_backward_weight, each only if its gradient is asked for."""

    @staticmethod
    def forward(ctx, x_nhwc, w, ks, stride, pad, fwd_native):
        if fwd_native:
            y = ops.trunk32_conv(x_nhwc, w, stride, pad)[0]
        else:
            y = torch.nn.functional.conv2d(x_nhwc.permute(0, 3, 1, 2), w, None, stride, pad).permute(0, 2, 3, 1).contiguous()
        ctx.save_for_backward(x_nhwc, w)
        ctx.geom = (ks, stride, pad)
        return y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        x, w = ctx.saved_tensors
        ks, stride, pad = ctx.geom
        g = g.contiguous()
        dx = ops.conv_backward_data(g, w, x.shape[1], x.shape[2], stride, pad) if ctx.needs_input_grad[0] else None
        dw = ops.conv_backward_weight(x, g, ks, stride, pad) if ctx.needs_input_grad[1] else None
        return dx, dw, None, None, None, None


class NativeConv2d(torch.nn.Conv2d):
    """nn.Conv2d (same parameters, same state-dict keys) whose backward runs the native weight- and data-gradient kernels.

    On a 4-d fp32 CUDA input, with ``bias=None``, ``groups=1``, ``dilation=1``, zero padding and a geometry the entries take
    for every gradient that will be asked for, the forward is ``_ConvNative``; the input is read as NHWC without a copy when it is
    ``channels_last`` (``x.permute(0, 2, 3, 1)`` contiguous), else copied once, and the output is the NCHW view of the NHWC
    result.  Everything else — the CPU, other dtypes, biased or grouped convs, a refused shape such as the stem when its input
    requires grad — is ``nn.Conv2d.forward``."""

    def _native_plan(self, x):
        w = self.weight
        if not (x.is_cuda and x.dim() == 4 and x.dtype == torch.float32 and w.is_cuda and w.dtype == torch.float32 and
                w.device == x.device and w.is_contiguous()):
            return None
        geom = _conv_geometry(self)
        if geom is None:
            return None
        ks, stride, pad = geom
        B, Cin, H, W = x.shape
        Cout = w.shape[0]
        if Cin != w.shape[1] or min(B, H, W) < 1:
            return None
        grad = torch.is_grad_enabled()
        args = (Cin, Cout, ks, stride, pad, B, H, W)
        if grad and x.requires_grad and not ops.conv_backward_supported(*args, "data"):
            return None
        if not ops.conv_backward_supported(*args, "weight"):         # also the geometry check of a call without gradients
            return None
        fwd_native = ops.trunk32_conv_supported(*args)
        if not fwd_native and Cin != 3:
            return None
        return ks, stride, pad, fwd_native

    def forward(self, x):
        plan = self._native_plan(x)
        if plan is None:
            return super().forward(x)
        return _ConvNative.apply(_nhwc(x), self.weight, *plan).permute(0, 3, 1, 2)


def native_conv_eligible(m):
    """True for a plain nn.Conv2d whose geometry the conv backward entries take at some input size."""
    if type(m) is not torch.nn.Conv2d:
        return False
    geom = _conv_geometry(m)
    if geom is None:
        return False
    ks, stride, pad = geom
    return (ks in (1, 3, 7) and stride in (1, 2) and pad <= ks // 2 and (m.in_channels % 16 == 0 or m.in_channels == 3) and
            m.out_channels % 64 == 0)


def use_native_convs(model):
    """Swaps every eligible ``nn.Conv2d`` of ``model`` (in place) for a ``NativeConv2d`` holding the SAME Parameter object, and
    returns how many it swapped.  state_dict() keys and values, optimizers holding the parameters and ``isinstance(m,
    nn.Conv2d)`` checks (modules.resnet_convs_of, IClassifier's native inference route) are unaffected."""
    def make(m):
        new = NativeConv2d(m.in_channels, m.out_channels, m.kernel_size, m.stride, m.padding, m.dilation, m.groups, False,
                           m.padding_mode, device="meta")
        new.weight = m.weight
        return new
    return _swap_children(model, native_conv_eligible, make)


# ---------------------------------------------------------------------------------------------------------------------------
# training the embedder: a whole BasicBlock on the native path.  The forward is composed from the fp32-class trunk's stage entries
# (ops.trunk32_conv: raw map + fused statistics, the next conv stages relu(IN(.)) itself; ops.trunk32_tail), the backward from
# ops.norm_backward (csrc/norm_bwd.hip) and the conv backward entries.  No normalised copy of a map is ever stored.  OPT-IN.
# ---------------------------------------------------------------------------------------------------------------------------
class _BasicBlockNative(torch.autograd.Function):
    """out = relu(IN(conv2(relu(IN(conv1(x))))) + (x | IN(convd(x)))) on NHWC fp32 maps; ``wd`` is None for an identity block."""

    @staticmethod
    def forward(ctx, x, w1, w2, wd, stride):
        y1, m1, r1 = ops.trunk32_conv(x, w1, stride, 1)
        y2, m2, r2 = ops.trunk32_conv(y1, w2, 1, 1, in_stats=(m1, r1))
        if wd is None:
            yd = md = rd = None
            out = ops.trunk32_tail("identity", y2, (m2, r2), x)
        else:
            yd, md, rd = ops.trunk32_conv(x, wd, stride, 0)
            out = ops.trunk32_tail("down", y2, (m2, r2), yd, (md, rd))
        ctx.save_for_backward(x, w1, w2, wd, y1, m1, r1, y2, m2, r2, out, yd, md, rd)
        ctx.stride = stride
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        x, w1, w2, wd, y1, m1, r1, y2, m2, r2, out, yd, md, rd = ctx.saved_tensors
        need_x, need_w1, need_w2, need_wd = ctx.needs_input_grad[:4]
        stride = ctx.stride
        H, W = x.shape[1], x.shape[2]
        g = g.contiguous()
        if wd is None:
            gy2, gres = ops.norm_backward("add", g, y2, (m2, r2), out=out)
        else:
            gy2, gyd = ops.norm_backward("add_down", g, y2, (m2, r2), out=out, down=(yd, (md, rd)))
        dx = dw1 = dw2 = dwd = None
        if need_w2:
            dw2 = ops.conv_backward_weight(y1, gy2, 3, 1, 1, in_stats=(m1, r1))
        if need_x or need_w1:
            ga = ops.conv_backward_data(gy2, w2, y1.shape[1], y1.shape[2], 1, 1)
            gy1 = ops.norm_backward("relu", ga, y1, (m1, r1))
            if need_w1:
                dw1 = ops.conv_backward_weight(x, gy1, 3, stride, 1)
            if need_x:
                dx = ops.conv_backward_data(gy1, w1, H, W, stride, 1)
                dx.add_(gres if wd is None else ops.conv_backward_data(gyd, wd, H, W, stride, 0))
        if wd is not None and need_wd:
            dwd = ops.conv_backward_weight(x, gyd, 1, stride, 0)
        return dx, dw1, dw2, dwd, None


def _block_parts(blk):
    """(stride, downsample conv or None) of a BasicBlock whose modules are the stock ones with plain InstanceNorm, else None."""
    try:
        stride = _same2(blk.conv1.stride)
        if stride not in (1, 2) or not resnet._conv_is(blk.conv1, 3, stride, 1) or not resnet._conv_is(blk.conv2, 3, 1, 1):
            return None
        if not (resnet._is_plain_instance_norm(blk.bn1) and resnet._is_plain_instance_norm(blk.bn2)):
            return None
        if not isinstance(blk.relu, torch.nn.ReLU) or blk.conv2.in_channels != blk.conv1.out_channels:
            return None
        down = blk.downsample
        if down is None:
            return (stride, None) if stride == 1 and blk.conv1.in_channels == blk.conv2.out_channels else None
        if len(down) != 2 or not resnet._conv_is(down[0], 1, stride, 0) or not resnet._is_plain_instance_norm(down[1]):
            return None
        if down[0].in_channels != blk.conv1.in_channels or down[0].out_channels != blk.conv2.out_channels:
            return None
        return stride, down[0]
    except (AttributeError, TypeError):
        return None


class NativeBasicBlock(resnet.BasicBlock):
    """resnet.BasicBlock (same submodules, same state-dict keys) that trains on the native path.

    On a 4-d fp32 CUDA input, with plain InstanceNorm behind both convs (and behind the downsample conv), the stock bias-free
    3x3 / 1x1 convs and a shape every entry involved takes (dsmil_trunk32_conv, the conv backward for every gradient that will
    be asked for, dsmil_norm_bwd), the forward is ``_BasicBlockNative``: a ``channels_last`` input is read as NHWC without a
    copy, the output is the NCHW view of the NHWC result, so a chain of blocks copies nothing between them.  Everything else —
    the CPU, other dtypes, BatchNorm, a refused shape — is ``BasicBlock.forward`` unchanged."""

    def _native_plan(self, x):
        if not (x.is_cuda and x.dim() == 4 and x.dtype == torch.float32):
            return None
        parts = _block_parts(self)
        if parts is None:
            return None
        stride, dconv = parts
        ws = [self.conv1.weight, self.conv2.weight] + ([dconv.weight] if dconv is not None else [])
        if not all(w.is_cuda and w.dtype == torch.float32 and w.device == x.device and w.is_contiguous() for w in ws):
            return None
        B, Cin, H, W = x.shape
        P = self.conv1.out_channels
        if Cin != self.conv1.in_channels or min(B, H, W) < 1:
            return None
        Ho, Wo = ops._conv_out(H, W, 3, stride, 1)
        convs = [(Cin, P, 3, stride, 1, B, H, W), (P, P, 3, 1, 1, B, Ho, Wo)]
        if dconv is not None:
            convs.append((Cin, P, 1, stride, 0, B, H, W))
        if not all(ops.trunk32_conv_supported(*c) for c in convs):
            return None
        # (emb::chan_ok, the tail's rule on P too, and C <= 2048 of the norm backward's own: this answer covers the tail)
        if not ops.norm_backward_supported("relu", B, Ho * Wo, P):
            return None
        if torch.is_grad_enabled():
            want_x = x.requires_grad
            want_w = [w.requires_grad for w in ws]
            data = [want_x, want_x or want_w[0], want_x]                      # conv2's data gradient feeds conv1's weight
            for c, w_w, w_d in zip(convs, want_w, data):
                if w_w and not ops.conv_backward_supported(*c, "weight"):
                    return None
                if w_d and not ops.conv_backward_supported(*c, "data"):
                    return None
        return stride, dconv

    def forward(self, x):
        plan = self._native_plan(x)
        if plan is None:
            return super().forward(x)
        stride, dconv = plan
        out = _BasicBlockNative.apply(_nhwc(x), self.conv1.weight, self.conv2.weight, dconv.weight if dconv is not None else None, stride)
        return out.permute(0, 3, 1, 2)


def native_block_eligible(m):
    """True for a plain resnet.BasicBlock whose modules and widths the native block path takes at some input size."""
    if not isinstance(m, resnet.BasicBlock) or isinstance(m, NativeBasicBlock) or _block_parts(m) is None:
        return False
    return m.conv1.in_channels % 16 == 0 and m.conv1.out_channels % 64 == 0 and m.conv1.out_channels <= 2048


def use_native_blocks(model):
    """Swaps every eligible ``BasicBlock`` of ``model`` (in place) for a ``NativeBasicBlock`` holding the SAME submodules (hence
    the same Parameter objects, submodule names and state_dict() keys and values), and returns how many it swapped.
    resnet18_in_convs / modules.resnet_convs_of and IClassifier's native inference route are unaffected; it composes with
    ``use_native_convs`` in either order (which then still covers the stem)."""
    def make(m):
        new = NativeBasicBlock.__new__(NativeBasicBlock)
        torch.nn.Module.__init__(new)
        for child, sub in m._modules.items():                      # registration order: conv1, bn1, relu, conv2, bn2, downsample
            new.register_module(child, sub)
        if m.downsample is None:                                   # a None set in __init__ is a plain attribute, not a child
            new.downsample = None
        new.stride = m.stride
        return new
    return _swap_children(model, native_block_eligible, make)


# ---------------------------------------------------------------------------------------------------------------------------
# training the embedder: the stem on the native path.  The forward is ops.trunk32_stem_train (the inference stem's kernels on their
# two-kernel route: the raw map, its statistics, the pooled map and each pool window's winner), the backward
# ops.stem_pool_backward (csrc/stem_bwd.hip) and the conv's weight gradient.  No normalised map and no index map of torch's is
# stored.  OPT-IN.
# ---------------------------------------------------------------------------------------------------------------------------
class _StemNative(torch.autograd.Function):
    """pooled = maxpool3x3/2/1(relu(IN(conv7x7/2/3(x, w)))): x fp32 NCHW [B,3,H,W], the result fp32 NHWC [B,Hp,Wp,64]."""

    @staticmethod
    def forward(ctx, x, w):
        pooled, y, (mean, rstd), win = ops.trunk32_stem_train(x, w)
        ctx.save_for_backward(x, y, mean, rstd, win)
        return pooled

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        if ctx.needs_input_grad[0]:
            raise NotImplementedError("the native stem gives no input gradient")
        if not ctx.needs_input_grad[1]:
            return None, None
        x, y, mean, rstd, win = ctx.saved_tensors
        gy = ops.stem_pool_backward(g.contiguous(), y, (mean, rstd), win)
        return None, ops.conv_backward_weight(_nhwc(x), gy, 7, 2, 3)


def _stem_eligible(x, w):
    if not (torch.is_tensor(x) and x.is_cuda and x.dim() == 4 and x.dtype == torch.float32 and not x.requires_grad and
            x.shape[1] == 3 and w.is_cuda and w.dtype == torch.float32 and w.device == x.device and w.is_contiguous() and
            tuple(w.shape) == (64, 3, 7, 7)):
        return False
    B, _, H, W = x.shape
    if min(B, H, W) < 1 or not ops.trunk32_stem_train_supported(B, H, W):
        return False
    if torch.is_grad_enabled() and w.requires_grad:
        H1, W1 = ops._conv_out(H, W, 7, 2, 3)
        return ops.stem_pool_backward_supported(B, H1, W1, 64) and ops.conv_backward_supported(3, 64, 7, 2, 3, B, H, W, "weight")
    return True


def native_stem(x, conv1_w):
    """``maxpool3x3/2/1(relu(instance_norm(conv2d(x, conv1_w, stride 2, padding 3))))`` on the native path, for models that keep
    the stem as entries of an ``nn.Sequential``: x fp32 NCHW [B,3,H,W] on the device, not requiring grad -> NCHW [B,64,Hp,Wp], a
    view of the NHWC result (a following NativeBasicBlock copies nothing).  Raises where ``use_native_stem`` would take torch."""
    if not _stem_eligible(x, conv1_w):
        raise NotImplementedError("native_stem takes a 4-d fp32 CUDA(HIP) input that does not require grad, a contiguous fp32 "
                                  "[64,3,7,7] weight on its device and a shape the stem entries take")
    return _StemNative.apply(x.contiguous(), conv1_w).permute(0, 3, 1, 2)


def _stem_modules_ok(model):
    mp = model.maxpool
    return (resnet._conv_is(model.conv1, 7, 2, 3) and model.conv1.in_channels == 3 and model.conv1.out_channels == 64 and
            resnet._is_plain_instance_norm(model.bn1) and isinstance(model.relu, torch.nn.ReLU) and
            isinstance(mp, torch.nn.MaxPool2d) and resnet._pair(mp.kernel_size) == (3, 3) and resnet._pair(mp.stride) == (2, 2) and
            resnet._pair(mp.padding) == (1, 1) and resnet._pair(mp.dilation) == (1, 1) and not mp.ceil_mode and
            not mp.return_indices)


def stem_forward(model, x):
    """What ``ResNet._features_torch`` runs for its stem once ``use_native_stem`` has marked the model: ``_StemNative`` where the
    modules and the input are eligible, else the torch chain unchanged."""
    if _stem_modules_ok(model) and _stem_eligible(x, model.conv1.weight):
        return _StemNative.apply(x.contiguous(), model.conv1.weight).permute(0, 3, 1, 2)
    return model.maxpool(model.relu(model.bn1(model.conv1(x))))


def use_native_stem(model):
    """Marks a ``resnet.ResNet`` (in place) so that its TRAINING forward sends ``maxpool(relu(bn1(conv1(x))))`` through
    ``_StemNative`` when it is eligible: a 4-d fp32 CUDA input that does not require grad, a plain InstanceNorm ``bn1``, the
    bias-free 7/2/3 ``conv1``, ``nn.ReLU``, ``MaxPool2d(3, 2, 1)`` (dilation 1, no ceil mode) and a shape the entries take;
    everything else takes the torch chain unchanged.  Returns 1 where the model's stem modules are the eligible ones, else 0
    (the mark is set either way; eligibility is decided per call).  No child module is added, removed or renamed, the Parameters
    are the same objects, state_dict() is the same; resnet18_in_convs and IClassifier's native inference route are unaffected.
    Composes with ``use_native_blocks`` and ``use_native_convs`` in any order."""
    if not isinstance(model, resnet.ResNet):
        raise TypeError("use_native_stem takes a resnet.ResNet")
    model._native_stem = True
    return int(_stem_modules_ok(model))
