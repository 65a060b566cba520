"""Which entries of libdsmil_hip.so the Python glue (dsmil-wsi_amd/ops.py, modules.py, training.py) calls, and in which order: the one-bag
and the batched paths keep their own native entries (they launch different kernels), and a packed weight image is cut once
per weight set — not once per call, not once per stream.  A recording proxy around ``_native.lib()`` notes the name of every
called symbol and forwards the call.  Shapes: the `tcga` / `passv` weight sets, bags of 5, 64 and 33 rows.  Needs a real MI355X."""
import pytest
import torch

from inputs import make_bag
from util import VARIANT, build_net

pytestmark = pytest.mark.gpu

LENGTHS = (5, 64, 33)
ONE_BAG = (5, 64, 33)
PACKS = {"dsmil_agg_pack_split", "dsmil_agg_pack_f2", "dsmil_value_pack", "dsmil_agg_pack_bf16"}
# the entries that enqueue work (size queries and the route function are not listed: they touch no device)
WORK = PACKS | {"dsmil_agg_forward_ex", "dsmil_agg_forward_bf16", "dsmil_agg_forward", "dsmil_agg_loss_head",
                "dsmil_agg_loss_head_bags", "dsmil_agg_backward", "dsmil_agg_backward_ex", "dsmil_agg_backward_rows",
                "dsmil_agg_backward_bags", "dsmil_agg_train_step", "dsmil_value_forward", "dsmil_value_backward",
                "dsmil_value_backward_rows", "dsmil_fc_forward", "dsmil_agg_train_step_bags", "dsmil_agg_train_step_bags_bf16",
                "dsmil_agg_train_step_bags_w", "dsmil_agg_train_step_bags_bf16_w", "dsmil_agg_loss_head_w",
                "dsmil_agg_loss_head_bags_w", "dsmil_agg_backward_bags_bf16", "dsmil_adam_step"}


class _Recorder:
    """Stands in for the loaded library: attribute access hands out the real function wrapped to note its name."""

    def __init__(self, real):
        self._real, self.calls = real, []

    def __getattr__(self, name):
        fn = getattr(self._real, name)

        def call(*args):
            self.calls.append(name)
            return fn(*args)
        return call

    def take(self):
        """The work entries called since the last take, in order, split into (pack calls, everything else)."""
        calls, self.calls = [c for c in self.calls if c in WORK], []
        return [c for c in calls if c in PACKS], [c for c in calls if c not in PACKS]


@pytest.fixture
def rec(monkeypatch):
    from dsmil_wsi_amd import _native
    r = _Recorder(_native.lib())
    monkeypatch.setattr(_native, "lib", lambda: r)
    return r


def _net(tag):
    """A fresh module per test: fresh parameters are a weight set no earlier test has packed."""
    return build_net(tag, "cuda").train()


def _rows(n, tag="tcga", seed=3):
    return torch.from_numpy(make_bag(seed, n, VARIANT[tag][0])).cuda()


def _label(tag="tcga"):
    y = torch.zeros(VARIANT[tag][1], device="cuda")
    y[0] = 1
    return y


@pytest.mark.parametrize("with_row_map", [False, True])
def test_bag_loss_calls_the_one_bag_entries_in_order(rec, with_row_map):
    net = _net("tcga")
    first = True
    for n in ONE_BAG:
        x = _rows(n)
        row_map = torch.arange(n - 1, -1, -1, device="cuda")[: max(1, n - 2)] if with_row_map else None
        loss, _, _ = net.bag_loss(x, _label(), row_map)
        loss.backward()
        packs, calls = rec.take()
        assert calls == ["dsmil_agg_forward_ex", "dsmil_agg_loss_head", "dsmil_agg_backward_ex"], (n, calls)
        # one-off image cuts of a new weight set: on its first use only, and never another kind
        assert set(packs) <= {"dsmil_agg_pack_split", "dsmil_agg_pack_f2"} and (first or not packs), (n, packs)
        first = False
    assert torch.isfinite(net.b_classifier.q[0].weight.grad).all()


@pytest.mark.parametrize("tag", ["tcga", "passv"])
def test_forward_with_row_gradients_calls_backward_rows(rec, tag):
    net = _net(tag)
    for n in ONE_BAG:
        x = _rows(n, tag).requires_grad_()
        _, pred, _, _ = net(x)
        pred.sum().backward()
        _, calls = rec.take()
        backward = [c for c in calls if "backward" in c]
        assert [c for c in backward if c.startswith("dsmil_agg_")] == ["dsmil_agg_backward_rows"], (n, calls)
        assert not any(c.endswith("_bags") for c in calls), (n, calls)
        if VARIANT[tag][3]:
            assert "dsmil_value_backward_rows" in backward and "dsmil_value_backward" in backward, (n, calls)
        else:
            assert not any(c.startswith("dsmil_value_") for c in calls), (n, calls)
        assert x.grad is not None and torch.isfinite(x.grad).all()


def test_batched_calls_use_the_bags_entries(rec):
    net = _net("tcga")
    x = _rows(sum(LENGTHS))
    classes, pred, A, B = net.forward_batch(x, LENGTHS)
    (pred.sum() + classes.sum()).backward()
    _, calls = rec.take()
    assert calls == ["dsmil_agg_forward_ex", "dsmil_agg_backward_bags"], calls
    labels = torch.stack([_label(), 1 - _label(), _label()])
    loss, _, _ = net.batch_loss(x, LENGTHS, labels)
    loss.backward()
    _, calls = rec.take()
    assert calls == ["dsmil_agg_forward_ex", "dsmil_agg_loss_head_bags", "dsmil_agg_backward_bags"], calls


def test_no_one_bag_call_reaches_a_bags_entry(rec):
    from dsmil_wsi_amd import ops
    net = _net("tcga")
    for n in ONE_BAG:
        x = _rows(n)
        net.bag_loss(x, _label())[0].backward()
        net(x)[1].sum().backward()
        xg = _rows(n).requires_grad_()
        net(xg)[1].sum().backward()
        with torch.no_grad():
            net(x)
        w = {k: (v.detach() if v is not None else None) for k, v in net.b_classifier._weights().items()}
        w["fc_w"], w["fc_b"] = net.i_classifier.fc[0].weight.detach(), net.i_classifier.fc[0].bias.detach()
        _, _, A, B, idx = ops.agg_forward(x, [n], w)
        g = torch.ones(VARIANT["tcga"][1], device="cuda")
        ops.agg_backward(x, w, A, B, idx, g)
        ops.agg_backward(x, w, A, B, idx, g, g_max=g, want_g_feats=True)
    _, calls = rec.take()
    assert calls and not any(c.endswith("_bags") for c in calls), calls


@pytest.mark.parametrize("tag", ["tcga", "passv"])
def test_packed_images_are_cut_once_per_weight_set(rec, tag):
    from dsmil_wsi_amd import ops
    net = _net(tag).eval()
    x = _rows(64, tag)
    q0_w = net.b_classifier.q[0].weight
    with torch.no_grad():
        net(x)
        first, _ = rec.take()
        net(x)
        again, _ = rec.take()
        # this route's image cuts, once each on the first forward and not again while the weights stay as they are
        assert "dsmil_agg_pack_split" in first and len(first) == len(set(first)), first
        assert ("dsmil_value_pack" in first) == VARIANT[tag][3], first
        assert again == [], again
        q0_w.add_(0)   # in place under no_grad: the values stay, q0_w._version moves on
        net(x)
        edited, _ = rec.take()
        # the query images are cut once more; the value image hangs on v's weight alone and stays
        assert sorted(edited) == sorted(set(first) - {"dsmil_value_pack"}), (first, edited)
        pool = ops.StreamPool(2)
        outs = [pool.run(net, x) for _ in range(2)]
        pool.join()
        other, calls = rec.take()
        assert other == [] and calls.count("dsmil_agg_forward_ex") == 2, (other, calls)
        ref = net(x)
    torch.cuda.synchronize()
    for out in outs:
        for a, b in zip(out, ref):
            assert torch.equal(a, b)


TRAIN_ROWS = (5, 64, 33, 40)   # one wave of rows, two full tiles, not a multiple of 32; three per step leave a group of one


def _train_calls(rec, **kw):
    """The work entries (packs aside) of one training.train epoch over four small fp32 `tcga` bags: stock criterion, Adam."""
    import argparse
    from dsmil_wsi_amd import training as T
    K, C = VARIANT["tcga"][:2]
    net = _net("tcga")
    opt = torch.optim.Adam(net.parameters(), lr=1e-3, betas=(0.5, 0.9), weight_decay=1e-3)
    bags = []
    for b, n in enumerate(TRAIN_ROWS):
        label = torch.zeros(n, C, device="cuda")
        label[:, b % C] = 1.0
        bags.append(torch.cat([_rows(n, seed=20 + b), label], 1))
    args = argparse.Namespace(feats_size=K, num_classes=C, **{"dropout_patch": 0.0, "bags_per_step": 1, "fused_step": True, **kw})
    rec.take()
    torch.manual_seed(5)
    loss = T.train(args, bags, net, torch.nn.BCEWithLogitsLoss(), opt, cache=T.BagCache("cuda", K), log=False)
    assert loss == loss and 0 < loss < 10, loss
    assert all(int(opt.state[p]["step"]) == -(-len(bags) // args.bags_per_step) for p in net.parameters())
    return rec.take()[1]


@pytest.mark.parametrize("dropout", [0.0, 0.4])
def test_train_of_one_bag_per_step_calls_the_one_bag_step(rec, dropout):
    assert _train_calls(rec, dropout_patch=dropout) == ["dsmil_agg_train_step"] * 4


def test_train_of_groups_calls_the_bags_step_also_for_a_short_last_group(rec):
    assert _train_calls(rec, bags_per_step=3) == ["dsmil_agg_train_step_bags"] * 2


def test_train_without_the_fused_step_calls_the_one_bag_entries(rec):
    assert _train_calls(rec, fused_step=False) == ["dsmil_agg_forward_ex", "dsmil_agg_loss_head", "dsmil_agg_backward_ex"] * 4
