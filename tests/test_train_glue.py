"""The Python training glue on the CPU (dsmil-wsi_amd/training.py): the read-back ring with per-bag loss vectors, and
training.train's one loop at every group size — its progress lines, its return value, and for groups of one the plain
per-bag loop of train_tcga.py:60-75 written out here."""
import argparse
import re

import numpy as np
import pytest
import torch

import dsmil as mil
from dsmil_wsi_amd import training as T


def test_readback_ring_hands_1d_tensors_over_as_lists():
    rb = T.LossReadback("cpu")
    assert rb.flush() is None                                   # never pushed
    assert rb.push(torch.tensor([1.5, 2.5, 3.5])) is None
    assert rb.push(torch.tensor([4.5])) == [1.5, 2.5, 3.5]      # the first call's values, a list
    assert rb.flush() == [4.5]                                  # one value of a 1-D tensor stays a list
    assert rb.flush() is None
    assert rb.push(torch.tensor(0.25)) is None and rb.push(torch.tensor([0.5, 0.75])) == 0.25 and rb.flush() == [0.5, 0.75]


def _setup():
    """Five seeded 16-feature bags, model and optimiser of test_train_progress_line_reports_every_bag_in_order."""
    rng = np.random.default_rng(3)
    bags = [torch.from_numpy(np.concatenate([rng.standard_normal((20 + b, 16)).astype(np.float32),
                                             np.full((20 + b, 1), b % 2, np.float32)], 1)) for b in range(5)]
    args = argparse.Namespace(feats_size=16, num_classes=1, dropout_patch=0.0, dropout_node=0.0, non_linearity=1,
                              lr=1e-3, weight_decay=1e-4, num_epochs=1, average=False)
    torch.manual_seed(0)
    np.random.seed(0)
    net, crit, opt, _ = T.init_model(args, mil, torch.device("cpu"))
    return args, bags, net, crit, opt


@pytest.mark.parametrize("per_step", [1, 2, 5])
def test_train_one_loop_for_every_group_size(per_step, capsys):
    args, bags, net, crit, opt = _setup()
    args.bags_per_step = per_step
    mean_loss = T.train(args, bags, net, crit, opt, log=True)
    out = capsys.readouterr().out
    assert re.findall(r"Training bag \[\d+/\d+\]", out) == ["Training bag [%d/5]" % i for i in range(5)], out
    lines = re.findall(r"^ Training bag \[(\d+)/5\] bag loss: ([0-9.]+)$", out.replace("\r", "\n"), re.M)
    assert [int(i) for i, _ in lines] == [0, 1, 2, 3, 4], out
    assert abs(sum(float(v) for _, v in lines) / 5 - mean_loss) < 1e-3
    if per_step == 1:
        from sklearn.utils import shuffle
        args, bags, net, crit, opt = _setup()     # the same model, optimiser and seeds
        net.train()
        total = 0.0
        for item in shuffle(list(bags)):
            feats, label = item[:, :16].contiguous(), item[0, 16:].unsqueeze(0)
            opt.zero_grad()
            loss, _, _ = T.bag_loss(net, crit, feats, label)
            loss.backward()
            opt.step()
            total += loss.item()
        assert abs(total / 5 - mean_loss) < 1e-6, (total / 5, mean_loss)
