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

from . import ops

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
