"""The class-weighted BCE objective on the GPU (BCEWithLogitsLoss(weight, pos_weight), train_mil.py:172-173 and :52-55):
the weighted loss heads (dsmil_agg_loss_head_w, dsmil_agg_loss_head_bags_w) against torch in fp64, the one-launch objective of
the batch step (k_loss_head_bags_mean inside dsmil_agg_train_step_bags_w / _bf16_w) against the loss head + generic backward,
the glue (MILNet.bag_loss / batch_loss, FusedTrainStep) against the torch expression under autograd + torch.optim.Adam, and
train_mil.py end to end on the native path against the same run with the native path switched off.  Needs a real MI355X."""
import ctypes
import functools
import io
from contextlib import redirect_stdout

import numpy as np
import pytest
import torch
import torch.nn as nn

from bwd_b16_cases import BATCH
from inputs import make_bag
from util import VARIANT, build_net, poison_workspace

pytestmark = pytest.mark.gpu

F32, B16 = torch.float32, torch.bfloat16
HP = dict(lr=1e-3, betas=(0.5, 0.9), weight_decay=1e-3)   # (tests/test_step_bags_gpu.py: six steps move the weights)
CLASSES = (1, 2, 5, 64)
N_BAGS = (1, 16, 17, 33)          # k_loss_head_bags_mean walks the bags 16 waves at a time
KINDS = ("pos", "weight", "both")
PLANT = (40.0, -40.0, 88.0, -88.0)   # the stable forms: exp(-|z|) underflows, exp(|z|) is near / beyond the fp32 range


def _class_weights(kind, C, seed):
    """(pos_weight, weight) as fp32 CPU tensors [C] or None, entries in [0.25, 4] with both ends present."""
    g = torch.Generator().manual_seed(seed)
    def draw():
        v = 0.25 * 16.0 ** torch.rand(C, generator=g)
        v[0] = 4.0
        v[-1] = 0.25 if C > 1 else 4.0
        return v.float()
    pw = draw() if kind in ("pos", "both") else None
    w = draw() if kind in ("weight", "both") else None
    return pw, w


@functools.lru_cache(maxsize=None)
def _head_case(C, n_bags):
    """The operands of a loss head for a batch: classes [T,C], pred / idx / labels [n,C] as fp32 / int64 CPU tensors, and the
    bag lengths.  Bag 0 is a single row, the last bag has its critical rows last; every class column of the labels holds both
    0 and 1 (n_bags > 1); logits at scale 3 with the PLANT values in the bag logits and at critical instance rows."""
    g = torch.Generator().manual_seed(1000 * C + n_bags)
    lengths = [1] + [int(v) for v in torch.randint(2, 8, (n_bags - 1,), generator=g)]
    T = sum(lengths)
    starts = [0] + [int(v) for v in np.cumsum(lengths)]
    classes = torch.randn(T, C, generator=g) * 3
    pred = torch.randn(n_bags, C, generator=g) * 3
    idx = torch.stack([torch.randint(0, n, (C,), generator=g) for n in lengths])
    idx[-1] = lengths[-1] - 1
    labels = torch.tensor([[float((b + c) % 2) for c in range(C)] for b in range(n_bags)])
    if n_bags == 1:
        labels = (torch.rand(1, C, generator=g) > 0.5).float()
    flat = n_bags * C
    for j in range(min(flat, 8)):          # both labels meet every planted value where the batch has room for it
        b, c = divmod(j, C)
        pred[b, c] = PLANT[j % 4] * (1.0 if j < 4 else -1.0)
        b, c = divmod(flat - 1 - j, C)
        classes[starts[b] + int(idx[b, c]), c] = PLANT[(j + 1) % 4] * (1.0 if j < 4 else -1.0)
    return classes, pred, idx, labels, tuple(lengths)


def _head_reference(C, n_bags, pw, w):
    """0.5 * crit(pred) + 0.5 * crit(max) per bag with crit = BCEWithLogitsLoss(weight, pos_weight) in fp64 on the CPU, and
    autograd for both logit gradients: (each [n], g_pred [n,C], g_max [n,C], max_pred [n,C]) as fp64 arrays."""
    classes, pred, idx, labels, lengths = _head_case(C, n_bags)
    starts = [0] + [int(v) for v in np.cumsum(lengths)]
    crit = nn.BCEWithLogitsLoss(weight=w.double() if w is not None else None, pos_weight=pw.double() if pw is not None else None)
    p64 = pred.double().requires_grad_(True)
    mx = torch.stack([classes[starts[b] + idx[b], torch.arange(C)] for b in range(n_bags)]).double().requires_grad_(True)
    each = torch.stack([0.5 * crit(p64[b].view(1, -1), labels[b].double().view(1, -1)) +
                        0.5 * crit(mx[b].view(1, -1), labels[b].double().view(1, -1)) for b in range(n_bags)])
    each.sum().backward()
    return each.detach().numpy(), p64.grad.numpy(), mx.grad.numpy(), mx.detach().numpy()


def _check_head(tag, got, ref, wprod, worst):
    """The bars of test_agg_bwd_gpu.py::test_loss_head_matches_torch_bce scaled by the weights: loss within
    1e-6 max(1, |ref|), gradients rtol 1e-5 + atol 1e-7 * (largest pos_weight * largest weight)."""
    each, g_pred, g_max = [t.double().cpu().numpy() for t in got]
    r_each, r_pred, r_max = ref
    le = np.abs(each - r_each) / np.maximum(1.0, np.abs(r_each))
    worst["loss"] = max(worst["loss"], float(le.max()))
    for name, a, r in (("g_pred", g_pred, r_pred), ("g_max", g_max, r_max)):
        excess = np.abs(a - r) / (1e-7 * wprod + 1e-5 * np.abs(r))
        worst[name] = max(worst[name], float(excess.max()))
    assert np.isfinite(each).all() and np.isfinite(g_pred).all() and np.isfinite(g_max).all(), tag
    assert float(le.max()) <= 1e-6, f"{tag}: loss off by {le.max():.3e} of max(1, |ref|)"
    np.testing.assert_allclose(g_pred, r_pred, rtol=1e-5, atol=1e-7 * wprod, err_msg=f"{tag}: g_pred")
    np.testing.assert_allclose(g_max, r_max, rtol=1e-5, atol=1e-7 * wprod, err_msg=f"{tag}: g_max")


@pytest.mark.parametrize("C", CLASSES)
def test_weighted_heads_match_torch_fp64(C):
    """dsmil_agg_loss_head_bags_w on batches of 1, 16, 17 and 33 bags and dsmil_agg_loss_head_w on each of their bags,
    pos_weight only / weight only / both, against BCEWithLogitsLoss(weight, pos_weight) in fp64 with autograd: loss within
    1e-6 max(1, |ref|), gradients rtol 1e-5 + atol 1e-7 * (max pos_weight * max weight); max_pred is the critical logit,
    bit for bit.  The worst measured errors, and whether the two entries agree to the bit, are printed."""
    from dsmil_wsi_amd import ops
    worst, same = {"loss": 0.0, "g_pred": 0.0, "g_max": 0.0}, True
    for n_bags in N_BAGS:
        classes, pred, idx, labels, lengths = _head_case(C, n_bags)
        starts = [0] + [int(v) for v in np.cumsum(lengths)]
        dev = [t.cuda() for t in (classes, pred, idx, labels)]
        for kind in KINDS:
            pw, w = _class_weights(kind, C, 7 * C + n_bags)
            wprod = float(pw.max() if pw is not None else 1.0) * float(w.max() if w is not None else 1.0)
            ref = _head_reference(C, n_bags, pw, w)
            cpw, cw = (pw.cuda() if pw is not None else None), (w.cuda() if w is not None else None)
            each, mx, g_pred, g_max = ops.agg_loss_head_bags(dev[0], lengths, dev[1], dev[2], dev[3], pos_weight=cpw, weight=cw)
            tag = f"C={C} n={n_bags} {kind}"
            _check_head(tag + " bags", (each, g_pred, g_max), ref[:3], wprod, worst)
            assert np.array_equal(mx.cpu().numpy().astype(np.float64), ref[3]), tag
            ones = [ops.agg_loss_head(dev[0][starts[b]:starts[b + 1]], dev[1][b], dev[2][b], dev[3][b], cpw, cw)
                    for b in range(n_bags)]       # the one-bag entry on every bag, at the same bars
            one = [torch.stack([o[i] for o in ones]) for i in range(4)]
            _check_head(tag + " one bag", (one[0], one[2], one[3]), ref[:3], wprod, worst)
            assert torch.equal(one[1], mx), tag
            same = same and all(torch.equal(a, b) for a, b in zip(one, (each, mx, g_pred, g_max)))
    print(f"C={C}: worst loss error {worst['loss']:.3e} of max(1,|ref|) (bar 1e-6); worst gradient error "
          f"{worst['g_pred']:.3f} / {worst['g_max']:.3f} of its bar; the two entries bit-equal on every bag: {same}")


def _raw_head(entry, dev, lengths, bw):
    """A loss-head entry called straight through ctypes on a batch (``_w``: bw = None for a NULL struct, or a BceWeights)."""
    from dsmil_wsi_amd import _native, ops
    classes, pred, idx, labels = dev
    n, C = pred.shape
    out = [torch.full((n,), 7.0, device="cuda")] + [torch.full((n, C), 7.0, device="cuda") for _ in range(3)]
    ptr = [t.data_ptr() for t in out]
    L = _native.lib()
    weighted = entry.endswith("_w")
    tail = ((ctypes.byref(bw) if bw is not None else None),) if weighted else ()
    stream = ops._stream(classes.device)
    if "bags" in entry:
        off = ops.offsets_tensor(lengths, classes.device)
        rc = getattr(L, entry)(classes.data_ptr(), off.data_ptr(), pred.data_ptr(), idx.data_ptr(), labels.data_ptr(), n, C, *ptr,
                               *tail, stream)
    else:
        assert n == 1
        rc = getattr(L, entry)(classes.data_ptr(), pred.data_ptr(), idx.data_ptr(), labels.data_ptr(), C, *ptr, *tail, stream)
    assert rc == 0, (entry, rc)
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("C", CLASSES)
def test_heads_with_null_weights_are_their_siblings_and_ones_agree(C):
    """dsmil_agg_loss_head_w / dsmil_agg_loss_head_bags_w with a NULL struct, and with a struct of two NULL members, give the
    bits of dsmil_agg_loss_head / dsmil_agg_loss_head_bags (loss, max_pred, g_pred, g_max); all-ones vectors agree with
    them within the bars of the fp64 comparison (they take the weighted arithmetic: not bit-equal in general)."""
    from dsmil_wsi_amd import _native
    ones = torch.ones(C, device="cuda")
    for n_bags in N_BAGS:
        classes, pred, idx, labels, lengths = _head_case(C, n_bags)
        dev = [t.cuda() for t in (classes, pred, idx, labels)]
        entries = ["dsmil_agg_loss_head_bags"] + (["dsmil_agg_loss_head"] if n_bags == 1 else [])
        for entry in entries:
            want = _raw_head(entry, dev, lengths, None)
            for bw in (None, _native.BceWeights(None, None)):
                got = _raw_head(entry + "_w", dev, lengths, bw)
                for a, b in zip(want, got):
                    assert torch.equal(a, b), (entry, n_bags)
            for bw in (_native.BceWeights(ones.data_ptr(), None), _native.BceWeights(None, ones.data_ptr()),
                       _native.BceWeights(ones.data_ptr(), ones.data_ptr())):
                got = _raw_head(entry + "_w", dev, lengths, bw)
                assert torch.equal(want[1], got[1])
                a, b = want[0].double().cpu().numpy(), got[0].double().cpu().numpy()
                assert (np.abs(a - b) <= 1e-6 * np.maximum(1.0, np.abs(a))).all(), (entry, n_bags)
                for u, v in zip(want[2:], got[2:]):
                    np.testing.assert_allclose(v.cpu().numpy(), u.cpu().numpy(), rtol=1e-5, atol=1e-7)


# ---- the models ------------------------------------------------------------------------------------------------------
def _small_net(C, K=32, seed=5):
    """MILNet(FCLayer, BClassifier) with C classes on the GPU, seeded (the shipped weight sets stop at three classes)."""
    import dsmil as mil
    torch.manual_seed(seed)
    net = mil.MILNet(mil.FCLayer(K, C), mil.BClassifier(input_size=K, output_class=C))
    return net.cuda().train()


def _criterion(kind, C, seed, shape="vector"):
    """BCEWithLogitsLoss with GPU class weights; ``shape``: "vector" [C], "row" [1,C], "scalar" 0-dim (train_mil.py:172)."""
    pw, w = _class_weights(kind, C, seed)
    def put(t):
        if t is None:
            return None
        if shape == "scalar":
            return t[0].clone().cuda()
        return (t.view(1, C) if shape == "row" else t).cuda()
    return nn.BCEWithLogitsLoss(weight=put(w), pos_weight=put(pw))


def _torch_objective(net, crit, x, lengths, labels, row_map=None):
    """The torch expression under autograd: per bag milnet(bag), torch.max, 0.5 * criterion + 0.5 * criterion; the mean
    over the bags.  Returns (loss, each [n] detached)."""
    if row_map is not None:
        x = x.index_select(0, row_map)
    each = []
    for bag, y in zip(torch.split(x, list(lengths), dim=0), labels.reshape(len(lengths), -1)):
        ins, pred, _, _ = net(bag)
        mx, _ = torch.max(ins, 0)
        each.append(0.5 * crit(pred.view(1, -1), y.view(1, -1)) + 0.5 * crit(mx.view(1, -1), y.view(1, -1)))
    each = torch.stack(each)
    return each.mean(), each.detach()


def _torch_objective_b16(net, crit, x, lengths, labels):
    """The same expression on bf16-STORED rows: the criterion in torch, on the fp32 logits of the batched bf16 forward
    (what MILNet.batch_loss forms its loss from: ``net(bag)`` itself would hand back logits rounded to bf16)."""
    ins, pred, _, _ = net._forward_batch(x, list(lengths), _f32_out=True)
    y = labels.reshape(len(lengths), -1)
    each = []
    for b, t in enumerate(torch.split(ins, list(lengths), dim=0)):
        mx, _ = torch.max(t, 0)
        each.append(0.5 * crit(pred[b].view(1, -1), y[b].view(1, -1)) + 0.5 * crit(mx.view(1, -1), y[b].view(1, -1)))
    each = torch.stack(each)
    return each.mean(), each.detach()


@pytest.mark.parametrize("C", CLASSES)
@pytest.mark.parametrize("n_bags", N_BAGS)
def test_step_objective_launch_matches_the_loss_head(C, n_bags):
    """k_loss_head_bags_mean with class weights (inside dsmil_agg_train_step_bags_w; lr = 0, zero moments, so
    exp_avg / (1 - beta1) is the step's gradient and the parameters stay put) against MILNet.batch_loss with the same
    criterion (dsmil_agg_loss_head_bags_w + the generic backward): each bag's loss and the mean within
    1e-6 max(1, |loss|) (whether the per-bag losses are bit-equal is printed), every parameter gradient at the bar of tests/test_bwd_bags_gpu.py, 2e-4 of its max-abs + 2e-5."""
    from dsmil_wsi_amd import training as T
    K, b1 = 32, 0.5
    g = torch.Generator().manual_seed(50 * C + n_bags)
    lengths = [1] + [int(v) for v in torch.randint(2, 9, (n_bags - 1,), generator=g)]
    x = torch.randn(sum(lengths), K, generator=g).cuda()
    labels = torch.tensor([[float((b + c) % 2) for c in range(C)] for b in range(n_bags)]).cuda()
    for kind in KINDS:
        crit = _criterion(kind, C, 3 * C + n_bags)
        nets = [_small_net(C, K), _small_net(C, K)]
        opt = torch.optim.Adam(nets[1].parameters(), lr=0.0, betas=(b1, 0.9), weight_decay=0.0)
        fused = T.FusedTrainStep.create(nets[1], crit, opt)
        assert fused is not None and fused.weighted
        before = {n: p.detach().clone() for n, p in nets[1].named_parameters()}
        loss0, _, _, each0 = T.batch_loss(nets[0], crit, x, lengths, labels)
        loss0.backward()
        loss1, each1 = fused.step_bags(x, lengths, labels)
        print(f"C={C} n={n_bags} {kind}: per-bag losses bit-equal {torch.equal(each0, each1)}")
        for u, v in zip([float(loss0)] + each0.tolist(), [float(loss1)] + each1.tolist()):
            assert abs(u - v) <= 1e-6 * max(1.0, abs(u)), (kind, u, v)
        for (n0, p0), (n1, p1) in zip(nets[0].named_parameters(), nets[1].named_parameters()):
            assert torch.equal(p1.detach(), before[n1]), n1
            ref = p0.grad.double().cpu().numpy()
            got = (opt.state[p1]["exp_avg"].double() / (1.0 - b1)).cpu().numpy()
            err, scale = float(np.abs(got - ref).max()), float(np.abs(ref).max())
            assert err <= 2e-4 * scale + 2e-5, f"{kind} {n0}: max err {err:.3e} vs scale {scale:.3e}"


# ---- glue ------------------------------------------------------------------------------------------------------------
PACKS = {"dsmil_agg_pack_split", "dsmil_agg_pack_f2", "dsmil_value_pack", "dsmil_agg_pack_bf16"}
WORK = PACKS | {"dsmil_agg_forward_ex", "dsmil_agg_forward_bf16", "dsmil_agg_forward", "dsmil_agg_loss_head",
                "dsmil_agg_loss_head_bags", "dsmil_agg_loss_head_w", "dsmil_agg_loss_head_bags_w", "dsmil_agg_backward",
                "dsmil_agg_backward_ex", "dsmil_agg_backward_rows", "dsmil_agg_backward_bags", "dsmil_agg_backward_bags_bf16",
                "dsmil_agg_train_step", "dsmil_agg_train_step_bags", "dsmil_agg_train_step_bags_bf16",
                "dsmil_agg_train_step_bags_w", "dsmil_agg_train_step_bags_bf16_w", "dsmil_adam_step", "dsmil_fc_forward",
                "dsmil_value_forward", "dsmil_value_backward", "dsmil_value_backward_rows"}


class _Recorder:
    """Stands in for the loaded library (tests/test_glue_calls_gpu.py): notes the name of every called symbol."""

    def __init__(self, real):
        self._real, self.calls = real, []

    def __getattr__(self, name):
        fn = getattr(self._real, name)

        def call(*args):
            self.calls.append(name)
            return fn(*args)
        return call

    def take(self):
        """The work entries called since the last take, in order, without the one-off image cuts of a new weight set."""
        calls, self.calls = [c for c in self.calls if c in WORK and c not in PACKS], []
        return calls


@pytest.fixture
def rec(monkeypatch):
    from dsmil_wsi_amd import _native
    r = _Recorder(_native.lib())
    monkeypatch.setattr(_native, "lib", lambda: r)
    return r


def _rows(n, tag, seed=3):
    return torch.from_numpy(make_bag(seed, n, VARIANT[tag][0])).cuda()


def _compare_grads(net, ref, what):
    for (n0, p0), (_, p1) in zip(ref.named_parameters(), net.named_parameters()):
        r, got = p0.grad.double().cpu().numpy(), p1.grad.double().cpu().numpy()
        err, scale = float(np.abs(got - r).max()), float(np.abs(r).max())
        assert err <= 2e-4 * scale + 2e-5, f"{what} {n0}: max err {err:.3e} vs scale {scale:.3e}"


@pytest.mark.parametrize("tag,kind,shape", [("tcga", "pos", "vector"), ("tcga", "both", "row"), ("musk", "pos", "scalar"),
                                            ("linq", "weight", "vector")])
def test_weighted_glue_calls_and_gradients(rec, tag, kind, shape):
    """training.bag_loss / batch_loss with a class-weighted criterion on a MILNet: exactly the native call sequences of the
    stock criterion with the ``_w`` head in place of the head, and parameter gradients equal to autograd through the torch
    expression (milnet(bag) + the criterion) at the bar of tests/test_bwd_bags_gpu.py: 2e-4 of the tensor's max-abs + 2e-5."""
    from dsmil_wsi_amd import training as T
    C = VARIANT[tag][1]
    crit = _criterion(kind, C, 11, shape)
    stock = nn.BCEWithLogitsLoss()
    for n in (5, 64, 33):
        x = _rows(n, tag, seed=n)
        y = torch.zeros(C, device="cuda")
        y[n % C] = float(n % 2) if C == 1 else 1.0
        row_map = torch.arange(n - 1, -1, -1, device="cuda")[: max(1, n - 2)] if n != 64 else None
        seqs = []
        for c in (stock, crit):
            net = build_net(tag, "cuda").train()
            loss, _, _ = T.bag_loss(net, c, x, y, row_map)
            loss.backward()
            seqs.append(rec.take())
        assert seqs[0] == ["dsmil_agg_forward_ex", "dsmil_agg_loss_head", "dsmil_agg_backward_ex"], seqs[0]
        assert seqs[1] == ["dsmil_agg_forward_ex", "dsmil_agg_loss_head_w", "dsmil_agg_backward_ex"], seqs[1]
        ref = build_net(tag, "cuda").train()
        want, _ = _torch_objective(ref, crit, x, [n if row_map is None else int(row_map.numel())], y, row_map)
        want.backward()
        rec.take()
        assert abs(float(loss) - float(want)) <= 1e-5 * max(1.0, abs(float(want)))
        _compare_grads(net, ref, f"bag_loss n={n}")
    lengths = (5, 64, 33)
    x = _rows(sum(lengths), tag, seed=9)
    labels = torch.tensor([[float((b + c) % 2) for c in range(C)] for b in range(3)]).cuda()
    seqs = []
    for c in (stock, crit):
        net = build_net(tag, "cuda").train()
        loss, _, _, each = T.batch_loss(net, c, x, lengths, labels)
        loss.backward()
        seqs.append(rec.take())
    assert seqs[0] == ["dsmil_agg_forward_ex", "dsmil_agg_loss_head_bags", "dsmil_agg_backward_bags"], seqs[0]
    assert seqs[1] == ["dsmil_agg_forward_ex", "dsmil_agg_loss_head_bags_w", "dsmil_agg_backward_bags"], seqs[1]
    ref = build_net(tag, "cuda").train()
    want, want_each = _torch_objective(ref, crit, x, lengths, labels)
    want.backward()
    assert abs(float(loss) - float(want)) <= 1e-5 * max(1.0, abs(float(want)))
    np.testing.assert_allclose(each.cpu().numpy(), want_each.cpu().numpy(), rtol=1e-5, atol=1e-6)
    _compare_grads(net, ref, "batch_loss")


# ---- the step --------------------------------------------------------------------------------------------------------
G_MUSK, G2 = [1, 2, 5, 3], [33, 64, 65]
# (tag, lengths, row dtype, row map: None / "perm" (every row kept, shuffled: train_mil.py:46) / a dropout rate, via __call__)
STEP_CASES = [("musk", G_MUSK, F32, "perm", False), ("tcga", G2, F32, 0.4, False), ("tcga", list(BATCH), B16, None, False),
              ("tcga", [700], B16, None, True), ("tcga", [129], F32, 0.4, True)]
STEP_IDS = ["musk-1x2x5x3-fp32-perm", "tcga-33x64x65-fp32-map", "tcga-G1-bf16", "tcga-700-bf16-call", "tcga-129-fp32-map-call"]


def _batch(tag, lengths, dtype, rmap, seed):
    """One batch (tests/test_step_bags_gpu.py): rows [sum(lengths), K] in ``dtype``, labels [n, C], the concatenated per-bag
    index lists (``lengths`` then count the kept rows)."""
    K, C = VARIANT[tag][0], VARIANT[tag][1]
    x = torch.from_numpy(np.concatenate([make_bag(seed + 13 * i, n, K) for i, n in enumerate(lengths)])).cuda().to(dtype)
    labels = torch.zeros(len(lengths), C)
    for b in range(len(lengths)):
        labels[b, (b + seed) % C] = float((b + seed) % 2) if C == 1 else 1.0
    row_map, kept = None, list(lengths)
    if rmap is not None:
        gen = torch.Generator().manual_seed(seed)
        maps, off, kept = [], 0, []
        for n in lengths:
            keep = n if rmap == "perm" else max(1, int(n * (1 - rmap)))
            maps.append(torch.randperm(n, generator=gen)[:keep] + off)
            off += n
            kept.append(keep)
        row_map = torch.cat(maps).cuda()
    return x, kept, labels.cuda(), row_map


@pytest.mark.parametrize("tag,lengths,dtype,rmap,lone", STEP_CASES, ids=STEP_IDS)
def test_weighted_step_follows_torch_autograd_and_adam(tag, lengths, dtype, rmap, lone):
    """Six steps of FusedTrainStep.step_bags (``lone``: FusedTrainStep.__call__) with a class-weighted criterion against the
    torch expression under autograd + torch.optim.Adam from the same start, at the bars of
    test_step_bags_follows_the_generic_path: losses to 1e-5 max(1, |loss|), parameters to 1e-4 of their scale, exp_avg to
    2e-4 of its scale, equal step counts.  Bit identity is not claimed: the reference's logit gradients are torch's."""
    from dsmil_wsi_amd import training as T
    C = VARIANT[tag][1]
    nets = [build_net(tag, "cuda").train() for _ in range(2)]
    opts = [torch.optim.Adam(n.parameters(), **HP) for n in nets]
    crit = _criterion("both" if C > 1 else "pos", C, 23, "scalar" if C == 1 else "vector")
    fused = T.FusedTrainStep.create(nets[1], crit, opts[1])
    assert fused is not None and fused.weighted
    for step in range(6):
        x, kept, labels, row_map = _batch(tag, lengths, dtype, rmap, 900 + 31 * step)
        assert fused.accepts(x)
        opts[0].zero_grad()
        if dtype is B16:
            l0, e0 = _torch_objective_b16(nets[0], crit, x, kept, labels)
        else:
            l0, e0 = _torch_objective(nets[0], crit, x, kept, labels, row_map)
        l0.backward()
        opts[0].step()
        if lone:
            l1 = fused(x, labels, row_map)
            e1 = l1.reshape(1)
        else:
            l1, e1 = fused.step_bags(x, kept, labels, row_map)
        a, b = [float(l0.detach())] + e0.tolist(), [float(l1)] + e1.tolist()
        print(f"step {step}: mean {a[0]:.7f} / {b[0]:.7f}, worst per-bag difference {max(abs(u - v) for u, v in zip(a, b)):.3e}")
        for u, v in zip(a, b):
            assert abs(u - v) <= 1e-5 * max(1.0, abs(u)), (step, a, b)
    fused.sync()
    for (n0, p0), (n1, p1) in zip(nets[0].named_parameters(), nets[1].named_parameters()):
        a, b = p0.detach().cpu().numpy(), p1.detach().cpu().numpy()
        s0, s1 = opts[0].state[p0], opts[1].state[p1]
        print(f"{n0}: bit-identical {np.array_equal(a, b)}, max diff {float(np.abs(a - b).max()):.3e}")
        np.testing.assert_allclose(b, a, atol=1e-4 * max(1e-3, float(np.abs(a).max())), rtol=0, err_msg=n0)
        assert float(s0["step"]) == float(s1["step"]) == 6.0
        np.testing.assert_allclose(s1["exp_avg"].cpu().numpy(), s0["exp_avg"].cpu().numpy(),
                                   atol=2e-4 * max(1e-6, float(s0["exp_avg"].abs().max())), rtol=0, err_msg=n0)


def _fresh(tag):
    """A step's operands from a fixed start (tests/test_step_bags_gpu.py): parameters, exp_avg, exp_avg_sq as new tensors."""
    net = build_net(tag, "cuda")
    w = dict(net.b_classifier._weights())
    lin = net.i_classifier.fc[0]
    params = [lin.weight, lin.bias, w["q0_w"], w["q0_b"], w["q2_w"], w["q2_b"], w["fcc_w"], w["fcc_b"]]
    params = [p.detach().clone() if p is not None else None for p in params]
    gen = torch.Generator().manual_seed(3)
    m = [(torch.randn(p.shape, generator=gen) * 1e-3).cuda() if p is not None else None for p in params]
    v = [(torch.rand(p.shape, generator=gen) * 1e-5).cuda() if p is not None else None for p in params]
    return params, m, v


@pytest.mark.parametrize("tag,lengths,dtype,rmap", [("tcga", list(BATCH), F32, 0.4), ("tcga", list(BATCH), B16, None),
                                                    ("musk", G_MUSK, F32, "perm")])
def test_weighted_step_is_deterministic_on_a_poisoned_workspace(tag, lengths, dtype, rmap):
    """Two runs of one weighted step from the same state give equal bits, and so does a run on a workspace whose every word
    was set to 0xFFFFFFFF before it."""
    from dsmil_wsi_amd import ops
    x, kept, labels, row_map = _batch(tag, lengths, dtype, rmap, 41)
    C = VARIANT[tag][1]
    pw, w = [t.cuda() for t in _class_weights("both", C, 2)]

    def run(poison):
        params, m, v = _fresh(tag)
        if poison:
            poison_workspace(ops)
        loss, each = ops.agg_train_step_bags(x, kept, labels, params, m, v, 3, 1e-3, (0.5, 0.9), 1e-8, 1e-3,
                                             nonlinear=bool(VARIANT[tag][2]), row_map=row_map, pos_weight=pw, weight=w)
        torch.cuda.synchronize()
        return [loss.clone(), each.clone()] + [t for t in params + m + v if t is not None]
    first, again, poisoned = run(False), run(False), run(True)
    assert all(torch.isfinite(t).all() for t in first)
    for i, (a, b, c) in enumerate(zip(first, again, poisoned)):
        assert torch.equal(a, b), f"output {i}: two runs differ"
        assert torch.equal(a, c), f"output {i}: the poisoned workspace changed it"


def _raw_step(entry, x, kept, labels, row_map, params, m, v, bw):
    """A step entry called straight through ctypes (``_w``: bw = None for a NULL struct, or a BceWeights).  Returns the
    status and (loss [1], loss_each [n])."""
    from dsmil_wsi_amd import _native, ops
    K, C = x.shape[1], labels.shape[1]
    ptr = lambda t: (t.data_ptr() if t is not None else 0)
    p = _native.AggParams(*[ptr(t) for t in params], K, K, C, 1)
    arr = ctypes.c_void_p * 8
    m_arr, v_arr = arr(*[ptr(t) for t in m]), arr(*[ptr(t) for t in v])
    st = _native.AdamState(ctypes.cast(m_arr, ctypes.POINTER(ctypes.c_void_p)), ctypes.cast(v_arr, ctypes.POINTER(ctypes.c_void_p)),
                           3, 1e-3, 0.5, 0.9, 1e-8, 1e-3)
    off = ops.offsets_tensor(kept, x.device)
    out = torch.zeros(1 + len(kept), device="cuda")
    L = _native.lib()
    sibling = entry[:-2] if entry.endswith("_w") else entry
    ws = ops._workspace(x.device, getattr(L, sibling + "_workspace_bytes")(len(kept), sum(kept), K, C, 1))
    rmap = () if "bf16" in entry else (ptr(row_map),)
    tail = ((ctypes.byref(bw) if bw is not None else None),) if entry.endswith("_w") else ()
    rc = getattr(L, entry)(x.data_ptr(), off.data_ptr(), len(kept), sum(kept), max(kept), *rmap, labels.data_ptr(),
                           ctypes.byref(p), ctypes.byref(st), out[1:].data_ptr(), out[0:1].data_ptr(), ws.data_ptr(), ws.numel(),
                           *tail, ops._stream(x.device))
    torch.cuda.synchronize()
    return rc, out


@pytest.mark.parametrize("dtype", [F32, B16], ids=["fp32", "bf16"])
def test_steps_with_null_weights_are_their_siblings_and_ones_agree(dtype):
    """dsmil_agg_train_step_bags_w / _bf16_w with a NULL struct or two NULL members: the bits of the sibling from the same
    state — loss_each, the mean, and through them and g_pred / g_max every parameter and both moments.  All-ones vectors:
    the losses within 1e-6 max(1, |loss|), parameters and exp_avg at the trajectory bars."""
    from dsmil_wsi_amd import _native
    entry = "dsmil_agg_train_step_bags_bf16" if dtype is B16 else "dsmil_agg_train_step_bags"
    x, kept, labels, row_map = _batch("tcga", list(BATCH), dtype, None if dtype is B16 else 0.4, 17)
    ones = torch.ones(labels.shape[1], device="cuda")

    def run(name, bw):
        params, m, v = _fresh("tcga")
        rc, out = _raw_step(name, x, kept, labels, row_map, params, m, v, bw)
        assert rc == 0, (name, rc)
        return [out] + [t for t in params + m + v if t is not None]
    want = run(entry, None)
    assert torch.isfinite(want[0]).all() and float(want[0].abs().sum()) > 0
    for bw in (None, _native.BceWeights(None, None)):
        for i, (a, b) in enumerate(zip(want, run(entry + "_w", bw))):
            assert torch.equal(a, b), f"tensor {i}"
    for bw in (_native.BceWeights(ones.data_ptr(), None), _native.BceWeights(ones.data_ptr(), ones.data_ptr())):
        got = run(entry + "_w", bw)
        a, b = want[0].double().cpu().numpy(), got[0].double().cpu().numpy()
        assert (np.abs(a - b) <= 1e-6 * np.maximum(1.0, np.abs(a))).all()
        n = (len(want) - 1) // 3
        for i in range(1, 1 + 2 * n):       # parameters (1e-4 of scale), then exp_avg (2e-4 of scale)
            r = want[i].cpu().numpy()
            tol = (1e-4 * max(1e-3, float(np.abs(r).max()))) if i <= n else (2e-4 * max(1e-6, float(np.abs(r).max())))
            np.testing.assert_allclose(got[i].cpu().numpy(), r, atol=tol, rtol=0)


@pytest.mark.parametrize("dtype", [F32, B16], ids=["fp32", "bf16"])
def test_refused_weighted_step_changes_nothing(dtype):
    """A refused weighted step (C = 65: labels and weights 65 wide, DSMIL_E_UNSUPPORTED before any launch; a weight pointer
    off its alignment at the C entry, DSMIL_E_ALIGN) leaves parameters, moments, outputs and FusedTrainStep.step untouched."""
    from dsmil_wsi_amd import _native, ops
    from dsmil_wsi_amd import training as T
    net = build_net("tcga", "cuda").train()
    opt = torch.optim.Adam(net.parameters(), **HP)
    crit = _criterion("both", 2, 4)
    fused = T.FusedTrainStep.create(net, crit, opt)
    x, kept, labels, _ = _batch("tcga", G2, dtype, None, 5)
    fused.step_bags(x, kept, labels)
    fused.sync()
    snap = lambda: [t.detach().clone() for p in net.parameters() for t in (p, opt.state[p]["exp_avg"], opt.state[p]["exp_avg_sq"])]
    before, step = snap(), fused.step
    wide, wide_w = torch.zeros(len(kept), 65, device="cuda"), torch.ones(65, device="cuda")
    params = [p.data if p is not None else None for p in fused.params]
    with pytest.raises(RuntimeError, match="dsmil_agg_train_step_bags(_bf16)?_w"):
        ops.agg_train_step_bags(x, kept, wide, params, fused.m, fused.v, 2, 1e-3, (0.5, 0.9), 1e-8, 0.0, pos_weight=wide_w,
                                weight=wide_w)
    with pytest.raises((RuntimeError, ValueError)):
        fused.step_bags(x, kept, wide)
    entry = "dsmil_agg_train_step_bags_bf16_w" if dtype is B16 else "dsmil_agg_train_step_bags_w"
    ones = torch.ones(4, device="cuda")
    rc, out = _raw_step(entry, x, kept, labels, None, params, fused.m, fused.v, _native.BceWeights(ones.data_ptr() + 2, None))
    assert rc == -5 and float(out.abs().sum()) == 0.0
    rc, out = _raw_step(entry, x, kept, wide, None, params, fused.m, fused.v, _native.BceWeights(wide_w.data_ptr(), None))
    assert rc == -2 and float(out.abs().sum()) == 0.0
    assert fused.step == step == 1
    for a, b in zip(before, snap()):
        assert torch.equal(a, b)


# ---- train_mil.py end to end -----------------------------------------------------------------------------------------
def test_train_mil_runs_on_the_native_path(monkeypatch, tmp_path):
    """train_mil.py --num_epoch 2 --cv_fold 3 on write_synthetic_mil_file(n_bags=24, n_inst=120, n_pos=9) (the default of 47
    positive bags would make all 24 positive and pos_weight = 0: a loss that is zero everywhere): one
    dsmil_agg_train_step_bags_w per training bag per epoch, one batched forward + one dsmil_agg_loss_head_bags_w per
    mil_epoch_test, no torch Adam step; the same run from the same seeds with the native path switched off reaches the same
    per-epoch losses within 1e-5 max(1, |loss|) and final parameters / exp_avg within the step test's bars."""
    import train_mil
    from dsmil_wsi_amd import _native
    from dsmil_wsi_amd import training as T
    path = T.write_synthetic_mil_file(str(tmp_path / "synthetic.svm"), n_bags=24, n_inst=120, n_pos=9)
    rec = _Recorder(_native.lib())
    monkeypatch.setattr(_native, "lib", lambda: rec)
    adam_steps = []
    adam_step = torch.optim.Adam.step
    monkeypatch.setattr(torch.optim.Adam, "step", lambda self, *a, **k: (adam_steps.append(1), adam_step(self, *a, **k))[1])
    log = {"train": [], "test": [], "models": []}
    train, test = T.mil_epoch_train, T.mil_epoch_test

    def train_rec(bags, ys, idx, milnet, criterion, optimizer, device):
        if not log["models"] or log["models"][-1][0] is not milnet:
            log["models"].append((milnet, optimizer))
        # train_mil.py:172-173 hands its 0-dim tensor to BCEWithLogitsLoss positionally: it is the criterion's ``weight``
        assert criterion.pos_weight is None and criterion.weight is not None and criterion.weight.dim() == 0
        log["train"].append((train(bags, ys, idx, milnet, criterion, optimizer, device), len(idx)))
        return log["train"][-1][0]

    def test_rec(bags, ys, idx, milnet, criterion, device):
        out = test(bags, ys, idx, milnet, criterion, device)
        log["test"].append((out[0], np.asarray(out[1]), len(idx)))
        return out
    monkeypatch.setattr(T, "mil_epoch_train", train_rec)
    monkeypatch.setattr(T, "mil_epoch_test", test_rec)
    runs = {}
    for native in (True, False):
        monkeypatch.setattr(T, "mil_fused_step", native)
        for v in log.values():
            v.clear()
        rec.calls.clear()
        adam_steps.clear()
        np.random.seed(7)
        torch.manual_seed(7)
        with redirect_stdout(io.StringIO()):
            acs = train_mil.main(["--data_file", path, "--num_epoch", "2", "--cv_fold", "3"])
        assert len(acs) == 3 and len(log["train"]) == len(log["test"]) == 6 and len(log["models"]) == 3
        calls = rec.take()
        if native:
            want = []
            for (_, n_train), (_, _, n_test) in zip(log["train"], log["test"]):
                assert n_train == 16 and n_test == 8
                want += ["dsmil_agg_train_step_bags_w"] * n_train + ["dsmil_agg_forward_ex", "dsmil_agg_loss_head_bags_w"]
            assert calls == want, calls
            assert not adam_steps
        else:
            assert not any(c.startswith("dsmil_agg_train_step") for c in calls) and len(adam_steps) == 6 * 16
        runs[native] = ([t[0] for t in log["train"]], [t[0] for t in log["test"]], [t[1] for t in log["test"]],
                        [({n: p.detach().clone() for n, p in net.named_parameters()},
                          {n: opt.state[p]["exp_avg"].clone() for n, p in net.named_parameters()},
                          {float(opt.state[p]["step"]) for p in net.parameters()}) for net, opt in log["models"]])
    a, b = runs[True], runs[False]
    for u, v in zip(a[0] + a[1], b[0] + b[1]):
        print(f"epoch loss native {u:.7f} / reference loop {v:.7f}")
        assert abs(u - v) <= 1e-5 * max(1.0, abs(v)), (a[:2], b[:2])
    for pa, pb in zip(a[2], b[2]):
        np.testing.assert_allclose(pa, pb, atol=1e-5, rtol=0)
    for (wa, ma, sa), (wb, mb, sb) in zip(a[3], b[3]):
        assert sa == sb == {32.0}
        for n in wb:
            r = wb[n].cpu().numpy()
            np.testing.assert_allclose(wa[n].cpu().numpy(), r, atol=1e-4 * max(1e-3, float(np.abs(r).max())), rtol=0, err_msg=n)
            r = mb[n].cpu().numpy()
            np.testing.assert_allclose(ma[n].cpu().numpy(), r, atol=2e-4 * max(1e-6, float(np.abs(r).max())), rtol=0, err_msg=n)
