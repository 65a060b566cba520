"""MILNet.forward_batch / batch_loss and training.train(bags_per_step > 1) on CPU tensors: the batch is the per-bag
results laid end to end, its loss the mean and its parameter gradients the sum (over n) of the per-bag ``bag_loss``
results, and a grouped epoch is the hand-written loop over the same groups.  fp64, CPU only."""
import io
import math
import types
from contextlib import redirect_stdout

import numpy as np
import pytest
import torch
import torch.nn as nn

import dsmil as mil
from dsmil_wsi_amd import training

LENGTHS = [1, 37, 128, 129, 700]
RTOL = 1e-10


def _net(K=24, C=2, nonlinear=True, passing_v=False, seed=0, dtype=torch.float64):
    torch.manual_seed(seed)
    return mil.MILNet(mil.FCLayer(K, C), mil.BClassifier(K, C, nonlinear=nonlinear, passing_v=passing_v)).to(dtype)


def _batch(K=24, C=2, seed=1, lengths=LENGTHS):
    g = torch.Generator().manual_seed(seed)
    feats = torch.randn(sum(lengths), K, generator=g, dtype=torch.float64)
    labels = (torch.rand(len(lengths), C, generator=g) > 0.5).to(torch.float64)
    return feats, labels


def _close(a, b):
    a, b = a.detach(), b.detach()
    scale = float(b.abs().max()) if b.numel() else 0.0
    assert float((a - b).abs().max()) <= RTOL * max(scale, 1e-300), (float((a - b).abs().max()), scale)


@pytest.mark.parametrize("nonlinear,passing_v,C", [(True, False, 2), (False, False, 1), (True, True, 3)])
def test_forward_batch_is_the_bags_laid_end_to_end(nonlinear, passing_v, C):
    net = _net(C=C, nonlinear=nonlinear, passing_v=passing_v).eval()
    feats, _ = _batch(C=C)
    classes, pred, A, B = net.forward_batch(feats, LENGTHS)
    T = sum(LENGTHS)
    assert classes.shape == (T, C) and pred.shape == (len(LENGTHS), C) and A.shape == (T, C) and B.shape == (len(LENGTHS), C, 24)
    o = 0
    for b, n in enumerate(LENGTHS):
        c1, p1, A1, B1 = net(feats[o:o + n])
        _close(classes[o:o + n], c1); _close(pred[b], p1.view(-1)); _close(A[o:o + n], A1); _close(B[b], B1.view(C, -1))
        o += n
    with pytest.raises(ValueError):
        net.forward_batch(feats, [5, 6])


@pytest.mark.parametrize("use_map", [False, True])
def test_batch_loss_is_the_mean_loss_and_the_summed_gradient(use_map):
    net = _net()
    feats, labels = _batch()
    feats.requires_grad_(True)
    lengths, row_map = LENGTHS, None
    if use_map:   # every bag keeps a random subset of its rows (dropout_patches as one concatenated index list)
        g = torch.Generator().manual_seed(5)
        maps, o = [], 0
        for n in LENGTHS:
            keep = max(1, int(n * 0.7))
            maps.append(torch.randperm(n, generator=g)[:keep] + o)
            o += n
        lengths, row_map = [int(m.numel()) for m in maps], torch.cat(maps)
    loss, pred, mx = net.batch_loss(feats, lengths, labels, row_map)
    assert loss.dim() == 0 and pred.shape == (5, 2) and mx.shape == (5, 2)
    loss.backward()
    got = {k: p.grad.clone() for k, p in net.named_parameters()}
    got_x = feats.grad.clone()
    net.zero_grad(); feats.grad = None
    ref_loss, o = 0.0, 0
    for b, n in enumerate(LENGTHS):
        rm = None if row_map is None else row_map[sum(lengths[:b]):sum(lengths[:b + 1])] - o
        l1, p1, m1 = net.bag_loss(feats[o:o + n], labels[b], rm)
        _close(pred[b], p1.view(-1)); _close(mx[b], m1.view(-1))
        (l1 / len(LENGTHS)).backward()
        ref_loss = ref_loss + l1.detach()
        o += n
    _close(loss.detach(), ref_loss / len(LENGTHS))
    for k, p in net.named_parameters():
        _close(got[k], p.grad)
    _close(got_x, feats.grad)
    each = net.batch_loss(feats.detach(), lengths, labels, row_map, per_bag=True)[3]
    assert each.shape == (5,) and not each.requires_grad
    _close(each.mean(), loss.detach())


class _Cache:
    def __init__(self, bags):
        self.bags = bags

    def get(self, item, feats_size=None):
        return self.bags[item]


@pytest.mark.parametrize("stock", [True, False])
def test_train_with_bags_per_step_matches_a_hand_written_loop(stock):
    K, C, n = 16, 2, 10
    g = torch.Generator().manual_seed(3)
    bags = {i: (torch.randn(5 + 7 * i, K, generator=g), (torch.rand(C, generator=g) > 0.5).float()) for i in range(n)}
    criterion = nn.BCEWithLogitsLoss() if stock else nn.BCEWithLogitsLoss(pos_weight=torch.tensor([1.5, 0.5]))
    args = types.SimpleNamespace(feats_size=K, dropout_patch=0, bags_per_step=4)

    net = _net(K, C, seed=7, dtype=torch.float32)
    opt = torch.optim.Adam(net.parameters(), lr=1e-3, betas=(0.5, 0.9), weight_decay=1e-3)
    steps = []
    opt.register_step_post_hook(lambda *a: steps.append(1))
    np.random.seed(11)
    out = io.StringIO()
    with redirect_stdout(out):
        mean_loss = training.train(args, list(range(n)), net, criterion, opt, cache=_Cache(bags))
    assert len(steps) == math.ceil(n / 4)
    lines = [s for s in out.getvalue().split("\r") if s.strip()]
    assert len(lines) == n and [int(s.split("[")[1].split("/")[0]) for s in lines] == list(range(n))   # one loss per bag

    from sklearn.utils import shuffle
    ref = _net(K, C, seed=7, dtype=torch.float32)
    ropt = torch.optim.Adam(ref.parameters(), lr=1e-3, betas=(0.5, 0.9), weight_decay=1e-3)
    np.random.seed(11)
    order = shuffle(list(range(n)))
    ref.train()
    reported = []
    for g0 in range(0, n, 4):
        ropt.zero_grad()
        group = order[g0:g0 + 4]
        total = 0
        for i in group:
            x, y = bags[i]
            ins, bag, _, _ = ref(x)
            mx = ins.max(0)[0]
            l = 0.5 * criterion(bag.view(1, -1), y.view(1, -1)) + 0.5 * criterion(mx.view(1, -1), y.view(1, -1))
            reported.append(float(l))
            total = total + l
        (total / len(group)).backward()
        ropt.step()
    for (k, p), (_, q) in zip(net.named_parameters(), ref.named_parameters()):
        assert torch.allclose(p, q, rtol=1e-5, atol=1e-7), k
    assert abs(mean_loss - sum(reported) / n) < 1e-5
    got = [float(s.split("loss:")[1]) for s in lines]
    assert np.allclose(got, reported, atol=2e-4)       # (printed with four decimals)

    # bags_per_step = 1 (and an args without the attribute) is the per-bag loop: one step per bag
    steps.clear()
    np.random.seed(11)
    with redirect_stdout(io.StringIO()):
        training.train(types.SimpleNamespace(feats_size=K, dropout_patch=0), list(range(n)), net, criterion, opt, cache=_Cache(bags))
    assert len(steps) == n
