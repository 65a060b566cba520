"""A class-weighted criterion on the CPU: training.bag_loss / batch_loss still give the reference expression
(0.5 * criterion(bag logits) + 0.5 * criterion(max instance logits)), and training.mil_epoch_train / mil_epoch_test from fixed
seeds give the parameters (bit for bit) and the losses of a literal restatement of train_mil.py:42-80 — the CPU path did not
move when the GPU path went native."""
import numpy as np
import pytest
import torch
import torch.nn as nn

import dsmil as mil
from dsmil_wsi_amd import training as T

K = 12


def _net(C, seed):
    torch.manual_seed(seed)
    return mil.MILNet(mil.FCLayer(K, C), mil.BClassifier(input_size=K, output_class=C))


def _criteria(C):
    t = torch.tensor
    per_class = t([0.25, 4.0, 1.5][:C])
    return [nn.BCEWithLogitsLoss(t(2.5)), nn.BCEWithLogitsLoss(pos_weight=per_class), nn.BCEWithLogitsLoss(weight=per_class),
            nn.BCEWithLogitsLoss(weight=per_class.view(1, C), pos_weight=t([3.0]))]


@pytest.mark.parametrize("C", [1, 3])
def test_bag_loss_and_batch_loss_equal_the_reference_expression(C):
    g = torch.Generator().manual_seed(5)
    lengths = [1, 7, 4]
    x = torch.randn(sum(lengths), K, generator=g)
    labels = (torch.rand(len(lengths), C, generator=g) > 0.5).float()
    row_map = torch.cat([torch.randperm(n, generator=g) + o for n, o in zip(lengths, (0, 1, 8))])
    for crit in _criteria(C):
        assert T._native_bce(crit, C) is not None
        net, ref = _net(C, 3), _net(C, 3)
        want, off = [], 0
        for n, y in zip(lengths, labels):
            ins, bag, _, _ = ref(x.index_select(0, row_map[off:off + n]))
            mx, _ = torch.max(ins, 0)
            want.append(0.5 * crit(bag.view(1, -1), y.view(1, -1)) + 0.5 * crit(mx.view(1, -1), y.view(1, -1)))
            off += n
        loss, bag, mx = T.bag_loss(net, crit, x, labels[1], row_map[1:8])
        assert torch.allclose(loss, want[1], rtol=1e-6, atol=1e-7)
        loss.backward()
        want[1].backward(retain_graph=True)
        for (name, p), (_, q) in zip(net.named_parameters(), ref.named_parameters()):
            assert torch.allclose(p.grad, q.grad, rtol=1e-5, atol=1e-7), name
        net.zero_grad(); ref.zero_grad()
        loss, pred, mxs, each = T.batch_loss(net, crit, x, lengths, labels, row_map)
        assert torch.allclose(each, torch.stack(want).detach(), rtol=1e-6, atol=1e-7)
        assert torch.allclose(loss, torch.stack(want).mean(), rtol=1e-6, atol=1e-7)
        loss.backward()
        torch.stack(want).mean().backward()
        for (name, p), (_, q) in zip(net.named_parameters(), ref.named_parameters()):
            assert torch.allclose(p.grad, q.grad, rtol=1e-5, atol=1e-7), name


def _reference_epoch_train(bags, ys, idx, milnet, criterion, optimizer):
    """train_mil.py:42-59, restated."""
    milnet.train()
    total = 0.0
    for i in idx:
        optimizer.zero_grad()
        data = bags[i][np.random.permutation(len(bags[i]))]
        bag_label = torch.tensor([[ys[i]]])
        classes, bag_prediction, _, _ = milnet(torch.from_numpy(data))
        max_prediction, _ = torch.max(classes, 0)
        loss_bag = criterion(bag_prediction.view(1, -1), bag_label.view(1, -1))
        loss_max = criterion(max_prediction.view(1, -1), bag_label.view(1, -1))
        loss_total = 0.5 * loss_bag + 0.5 * loss_max
        loss_total.backward()
        optimizer.step()
        total = total + loss_total.item()
    return total / len(idx)


def _reference_epoch_test(bags, ys, idx, milnet, criterion):
    """train_mil.py:61-80, restated."""
    milnet.eval()
    total, preds = 0.0, []
    with torch.no_grad():
        for i in idx:
            bag_label = torch.tensor([[ys[i]]])
            classes, bag_prediction, _, _ = milnet(torch.from_numpy(bags[i]))
            max_prediction, _ = torch.max(classes, 0)
            loss_total = 0.5 * criterion(bag_prediction.view(1, -1), bag_label.view(1, -1)) + \
                0.5 * criterion(max_prediction.view(1, -1), bag_label.view(1, -1))
            total = total + loss_total.item()
            preds.append(torch.sigmoid(bag_prediction).squeeze().item())
    return total / len(idx), np.asarray(preds)


def test_mil_epochs_on_the_cpu_are_the_reference_loop():
    rng = np.random.default_rng(4)
    bags = [rng.standard_normal((int(n), K)).astype(np.float32) for n in rng.integers(1, 9, size=14)]
    ys = (rng.random(14) > 0.6).astype(np.float32)
    train_idx, test_idx = np.arange(10), np.arange(10, 14)
    pos = float(ys[train_idx].sum())
    runs = []
    for mine in (True, False):
        net = _net(1, 9)
        crit = nn.BCEWithLogitsLoss(torch.tensor((len(train_idx) - pos) / max(pos, 1.0)))       # train_mil.py:172-173
        opt = torch.optim.Adam(net.parameters(), lr=2e-3, betas=(0.5, 0.9), weight_decay=5e-3)
        np.random.seed(21)
        log = []
        for _ in range(3):
            if mine:
                tr = T.mil_epoch_train(bags, ys, train_idx, net, crit, opt, torch.device("cpu"))
                te, preds = T.mil_epoch_test(bags, ys, test_idx, net, crit, torch.device("cpu"))
            else:
                tr = _reference_epoch_train(bags, ys, train_idx, net, crit, opt)
                te, preds = _reference_epoch_test(bags, ys, test_idx, net, crit)
            log.append((tr, te, preds))
        runs.append((net, opt, log))
    (net_a, opt_a, log_a), (net_b, opt_b, log_b) = runs
    for (tr_a, te_a, p_a), (tr_b, te_b, p_b) in zip(log_a, log_b):
        assert tr_a == tr_b and te_a == te_b
        assert np.array_equal(p_a, p_b)
    for (name, p), (_, q) in zip(net_a.named_parameters(), net_b.named_parameters()):
        assert torch.equal(p, q), name
        assert torch.equal(opt_a.state[p]["exp_avg"], opt_b.state[q]["exp_avg"]), name
        assert float(opt_a.state[p]["step"]) == float(opt_b.state[q]["step"]) == 30.0
