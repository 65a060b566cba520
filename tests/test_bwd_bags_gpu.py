"""dsmil_agg_backward_bags / dsmil_agg_loss_head_bags (csrc/agg_bwd_bags.h) and the layers above them — the aggregator
backward over a BATCH of bags — against fp64 restatements: oracle.agg_oracle.train_loss_and_grads per bag, summed, for
the training objective; an fp64 torch autograd restatement (per bag, the critical indices held constant) for dense
upstream gradients, the input rows and the value rows.  Needs a real MI355X.

Bar (the project's bar for gradients, tests/test_agg_bwd_gpu.py): each gradient within 2e-4 of its own max-abs + 2e-5
absolute; losses within 1e-5."""
import io
import types
from contextlib import redirect_stdout

import numpy as np
import pytest
import torch

from conftest import load_weights
from inputs import make_bag
from util import VARIANT, build_net, poison_workspace

pytestmark = pytest.mark.gpu

KEYS = ("fc_w", "fc_b", "q0_w", "q0_b", "q2_w", "q2_b", "fcc_w", "fcc_b")
FEW = [1, 37, 128, 129, 4000, 10000]


def _weights(tag):
    """(weights as fp32 CPU tensors, K, C, nonlinear, passing_v); "c5" is a seeded C = 5 set."""
    if tag == "c5":
        K, C = 64, 5
        rng = np.random.default_rng(505)
        p = {"fc_w": rng.standard_normal((C, K), dtype=np.float32) * 0.05, "fc_b": rng.standard_normal(C, dtype=np.float32) * 0.1,
             "q0_w": rng.standard_normal((128, K), dtype=np.float32) * np.float32(1.0 / np.sqrt(K)),
             "q0_b": rng.standard_normal(128, dtype=np.float32) * 0.1,
             "q2_w": rng.standard_normal((128, 128), dtype=np.float32) * np.float32(1.0 / np.sqrt(128)),
             "q2_b": rng.standard_normal(128, dtype=np.float32) * 0.1,
             "fcc_w": rng.standard_normal((C, C, K), dtype=np.float32) * 0.05, "fcc_b": rng.standard_normal(C, dtype=np.float32) * 0.1}
        return {k: torch.from_numpy(v) for k, v in p.items()}, K, C, True, False
    K, C, nonlinear, passing_v = VARIANT[tag]
    p = load_weights(tag)
    return {k: torch.from_numpy(np.ascontiguousarray(p[k])).float() for k in KEYS if k in p}, K, C, nonlinear, passing_v


def _batch(lengths, K, seed):
    return torch.from_numpy(np.concatenate([make_bag(seed + 17 * b, n, K) for b, n in enumerate(lengths)], axis=0))


def _autograd_f64(x, vals, p, lengths, idx, nonlinear, g):
    """Plain fp64 restatement (CPU) of FCLayer + BClassifier over the bags of a batch given their critical indices
    (bag-local); objective = sum over the bags of <output, upstream gradient> for every upstream form in g
    (pred [n,C], max [n,C] on the critical rows' logits, classes / A [T,C], B [n,C,Kv]).  Returns the parameter
    gradients (summed over the bags by construction), "feats" and, with vals, "vals"."""
    x = x.double().requires_grad_(True)
    P = {k: v.double().requires_grad_(True) for k, v in p.items()}
    V = vals.double().requires_grad_(True) if vals is not None else x
    obj, o = 0.0, 0
    for b, n in enumerate(lengths):
        xb, Vb, ib = x[o:o + n], V[o:o + n], idx[b]
        c = xb @ P["fc_w"].T + P["fc_b"]
        h = xb @ P["q0_w"].T + P["q0_b"]
        Q = torch.tanh(torch.relu(h) @ P["q2_w"].T + P["q2_b"]) if nonlinear else h
        A = torch.softmax(Q @ Q[ib].T / np.sqrt(128.0), 0)
        B = A.T @ Vb
        pred = torch.einsum("ock,ck->o", P["fcc_w"], B) + P["fcc_b"]
        obj = obj + (pred * g["pred"][b].double()).sum()
        if g.get("max") is not None:
            obj = obj + (c[ib, torch.arange(c.shape[1])] * g["max"][b].double()).sum()
        if g.get("classes") is not None:
            obj = obj + (c * g["classes"][o:o + n].double()).sum()
        if g.get("A") is not None:
            obj = obj + (A * g["A"][o:o + n].double()).sum()
        if g.get("B") is not None:
            obj = obj + (B * g["B"][b].double()).sum()
        o += n
    obj.backward()
    out = {k: v.grad for k, v in P.items() if v.grad is not None}
    out["feats"] = x.grad
    if vals is not None:
        out["vals"] = V.grad
    return out


def _check(got, ref, tag, keys=None):
    for k, r in ref.items():
        if keys is not None and k not in keys:
            continue
        if k not in got:
            continue
        r = r.numpy() if isinstance(r, torch.Tensor) else np.asarray(r)
        scale = max(float(np.abs(r).max()), 1e-12)
        err = float(np.abs(got[k].cpu().numpy().astype(np.float64) - r).max())
        print(f"{tag} {k}: max err {err:.3e} scale {scale:.3e}")
        assert err <= 2e-4 * scale + 2e-5, f"{tag} {k}: max err {err:.3e} vs scale {scale:.3e}"


def _upstream(which, lengths, C, Kv, rng):
    n, T = len(lengths), sum(lengths)
    r = lambda *s: torch.from_numpy(rng.standard_normal(s).astype(np.float32))
    g = {"pred": r(n, C)}
    if "m" in which:
        g["max"] = r(n, C)
    if "c" in which:
        g["classes"] = r(T, C)
    if "A" in which:
        g["A"] = r(T, C)
    if "B" in which:
        g["B"] = r(n, C, Kv)
    return g


def _native(xg, lengths, pg, fwd, gg, vg, nonlinear, want_x, want_v, row_map=None):
    """ops.agg_backward_bags once to size the workspace, then on a NaN-poisoned workspace: a read of anything this call
    has not written (an idle tile slot of gqp, another bag's partials) shows up."""
    from dsmil_wsi_amd import ops
    _, _, A, B, idx = fwd
    call = lambda: ops.agg_backward_bags(xg, lengths, pg, A, B, idx, gg["pred"], g_classes=gg.get("classes"),
                                         g_A=gg.get("A"), g_B=gg.get("B"), vals=vg, nonlinear=nonlinear,
                                         want_g_vals=want_v, g_max=gg.get("max"), row_map=row_map, want_g_feats=want_x)
    call()
    poison_workspace(ops)
    out = {k: v.clone() for k, v in call().items()}
    torch.cuda.synchronize()
    return out


def _case(tag, lengths, which, want_x, seed=0):
    from dsmil_wsi_amd import ops
    p, K, C, nonlinear, passing_v = _weights(tag)
    rng = np.random.default_rng(1000 + seed + sum(lengths))
    x = _batch(lengths, K, 300 + seed)
    vals = torch.from_numpy(rng.standard_normal((sum(lengths), K)).astype(np.float32)) if passing_v else None
    pg = {k: v.cuda() for k, v in p.items()}
    xg, vg = x.cuda(), (vals.cuda() if vals is not None else None)
    fwd = ops.agg_forward(xg, lengths, pg, vals=vg, nonlinear=nonlinear)
    g = _upstream(which, lengths, C, K, rng)
    gg = {k: v.cuda() for k, v in g.items()}
    got = _native(xg, lengths, pg, fwd, gg, vg, nonlinear, want_x, passing_v)
    ref = _autograd_f64(x, vals, p, lengths, fwd[4].cpu(), nonlinear, g)
    if not want_x:
        assert "feats" not in got
    if "m" not in which and "c" not in which:
        assert "fc_w" not in got
    _check(got, ref, f"{tag} {lengths if len(lengths) < 8 else len(lengths)} {which}")
    return got


TAGS = ["tcga", "c16", "musk", "tree", "linq", "passv", "c5"]


@pytest.mark.parametrize("tag", TAGS)
def test_training_objective_few_rows(tag):
    """g_pred + sparse g_max from the batched loss head, lengths [1, 37, 128, 129, 4000, 10000]: losses and gradients
    against the fp64 restatement; for the reference's model form (nonlinear, v = Identity) also against
    oracle.agg_oracle.train_loss_and_grads per bag, summed."""
    from dsmil_wsi_amd import ops
    import agg_oracle
    p, K, C, nonlinear, passing_v = _weights(tag)
    lengths = FEW
    x = _batch(lengths, K, 40)
    rng = np.random.default_rng(4)
    vals = torch.from_numpy(rng.standard_normal((sum(lengths), K)).astype(np.float32)) if passing_v else None
    labels = torch.from_numpy((rng.random((len(lengths), C)) > 0.5).astype(np.float32))
    pg = {k: v.cuda() for k, v in p.items()}
    xg, vg = x.cuda(), (vals.cuda() if vals is not None else None)
    fwd = ops.agg_forward(xg, lengths, pg, vals=vg, nonlinear=nonlinear)
    loss, max_pred, g_pred, g_max = ops.agg_loss_head_bags(fwd[0], lengths, fwd[1], fwd[4], labels.cuda())
    # the batched head is the one-bag head, bag by bag
    o = 0
    for b, n in enumerate(lengths):
        l1, m1, gp1, gm1 = ops.agg_loss_head(fwd[0][o:o + n], fwd[1][b], fwd[4][b], labels[b].cuda())
        assert torch.equal(l1, loss[b]) and torch.equal(m1, max_pred[b]) and torch.equal(gp1, g_pred[b]) and torch.equal(gm1, g_max[b])
        o += n
    gg = {"pred": g_pred, "max": g_max}
    got = _native(xg, lengths, pg, fwd, gg, vg, nonlinear, False, passing_v)
    ref = _autograd_f64(x, vals, p, lengths, fwd[4].cpu(), nonlinear, {"pred": g_pred.cpu(), "max": g_max.cpu()})
    _check(got, ref, f"{tag} objective")
    if nonlinear and not passing_v:
        pn = {k: v.numpy() for k, v in p.items()}
        tot, o = None, 0
        for b, n in enumerate(lengths):
            lb, gb = agg_oracle.train_loss_and_grads(x[o:o + n].numpy(), labels[b].numpy(), pn)
            print(f"{tag} bag {b}: loss {float(loss[b]):.7f} oracle {lb:.7f}")
            assert abs(float(loss[b]) - lb) <= 1e-5
            tot = gb if tot is None else {k: tot[k] + gb[k] for k in gb}
            o += n
        _check(got, tot, f"{tag} oracle")


@pytest.mark.parametrize("tag", TAGS)
def test_dense_upstream_with_row_gradients_few_rows(tag):
    _case(tag, FEW, "pmcAB", True)


@pytest.mark.parametrize("lengths,which,want_x", [
    ([10000] * 8, "pm", True), ([10000] * 8, "pcAB", False),
    ([64] * 17 + [30000] + [64] * 23, "pmcAB", True),
    ([64] * 17 + [70000] + [64] * 23, "pm", True),        # the same ragged shape in the four-wave tile regime
])
def test_batch_tile_regime(lengths, which, want_x):
    _case("tcga", lengths, which, want_x, seed=3)


def test_batch_tile_regime_unaligned_rows():
    _case("musk", [20000, 3, 50000, 64], "pmcAB", True, seed=5)   # K = 166 at >= 65 536 rows: the one-wave tile over slots


@pytest.mark.parametrize("want_x", [False, True])
def test_row_map_is_the_gathered_copy(want_x):
    from dsmil_wsi_amd import ops
    p, K, C, nonlinear, _ = _weights("tcga")
    phys = [50, 700, 129, 4000]
    x = _batch(phys, K, 9).cuda()
    gen = torch.Generator().manual_seed(2)
    maps, o = [], 0
    for n in phys:
        maps.append(torch.randperm(n, generator=gen)[:max(1, int(n * 0.8))] + o)
        o += n
    lengths, row_map = [int(m.numel()) for m in maps], torch.cat(maps).cuda()
    pg = {k: v.cuda() for k, v in p.items()}
    g = {k: v.cuda() for k, v in _upstream("pmcAB", lengths, C, K, np.random.default_rng(8)).items()}
    xc = x.index_select(0, row_map).contiguous()
    fm = ops.agg_forward(x, lengths, pg, nonlinear=nonlinear, row_map=row_map)
    fc = ops.agg_forward(xc, lengths, pg, nonlinear=nonlinear)
    for a, b in zip(fm, fc):
        assert torch.equal(a, b)
    a = _native(x, lengths, pg, fm, g, None, nonlinear, want_x, False, row_map=row_map)
    b = _native(xc, lengths, pg, fc, g, None, nonlinear, want_x, False)
    assert set(a) == set(b)
    for k in a:
        assert torch.equal(a[k], b[k]), k
    ref = _autograd_f64(xc.cpu(), None, p, lengths, fc[4].cpu(), nonlinear, {k: v.cpu() for k, v in g.items()})
    _check(a, ref, "row_map")


def test_two_classes_share_a_critical_row():
    from dsmil_wsi_amd import ops
    p, K, C, nonlinear, _ = _weights("tcga")
    p["fc_w"][1] = 2.0 * p["fc_w"][0]       # the same direction: both classes pick the same instance
    p["fc_b"][1] = p["fc_b"][0]
    lengths = [300, 1, 2000, 65]
    x = _batch(lengths, K, 21)
    pg = {k: v.cuda() for k, v in p.items()}
    fwd = ops.agg_forward(x.cuda(), lengths, pg, nonlinear=nonlinear)
    idx = fwd[4].cpu()
    assert torch.equal(idx[:, 0], idx[:, 1]), idx
    g = _upstream("pmcAB", lengths, C, K, np.random.default_rng(3))
    got = _native(x.cuda(), lengths, pg, fwd, {k: v.cuda() for k, v in g.items()}, None, nonlinear, True, False)
    _check(got, _autograd_f64(x, None, p, lengths, idx, nonlinear, g), "shared critical row")


@pytest.mark.parametrize("tag,N,which", [("tcga", 3000, "pmcAB"), ("tcga", 70000, "pm"), ("musk", 333, "pmcAB"),
                                         ("linq", 1000, "pmA"), ("passv", 500, "pmcAB"), ("c5", 129, "pmcAB")])
def test_one_bag_is_bit_identical_to_backward_rows(tag, N, which):
    from dsmil_wsi_amd import ops
    p, K, C, nonlinear, passing_v = _weights(tag)
    rng = np.random.default_rng(N)
    x = torch.from_numpy(make_bag(7, N, K)).cuda()
    vg = torch.from_numpy(rng.standard_normal((N, K)).astype(np.float32)).cuda() if passing_v else None
    pg = {k: v.cuda() for k, v in p.items()}
    fwd = ops.agg_forward(x, [N], pg, vals=vg, nonlinear=nonlinear)
    g = {k: v.cuda() for k, v in _upstream(which, [N], C, K, rng).items()}
    one = ops.agg_backward(x, pg, fwd[2], fwd[3], fwd[4], g["pred"], g_classes=g.get("classes"), g_A=g.get("A"),
                           g_B=g["B"][0] if "B" in g else None, vals=vg, nonlinear=nonlinear, want_g_vals=passing_v,
                           g_max=g.get("max"), want_g_feats=True)
    one = {k: v.clone() for k, v in one.items()}
    bags = _native(x, [N], pg, fwd, g, vg, nonlinear, True, passing_v)
    assert set(one) == set(bags)
    for k in one:
        assert torch.equal(one[k], bags[k]), f"{tag} N={N} {k}: {float((one[k] - bags[k]).abs().max()):.3e}"


def test_deterministic_and_close_to_the_sum_of_one_bag_calls():
    """Two runs give the same bits; and the batched result against the parent route — one dsmil_agg_backward_rows per
    bag, summed in fp64 — at the bar of this file (the gap is printed)."""
    from dsmil_wsi_amd import ops
    p, K, C, nonlinear, _ = _weights("tcga")
    lengths = [10000, 37, 4000, 129, 10000, 1, 6000, 2500]
    x = _batch(lengths, K, 77).cuda()
    pg = {k: v.cuda() for k, v in p.items()}
    fwd = ops.agg_forward(x, lengths, pg, nonlinear=nonlinear)
    g = {k: v.cuda() for k, v in _upstream("pmcAB", lengths, C, K, np.random.default_rng(6)).items()}
    a = _native(x, lengths, pg, fwd, g, None, nonlinear, True, False)
    b = _native(x, lengths, pg, fwd, g, None, nonlinear, True, False)
    for k in a:
        assert torch.equal(a[k], b[k]), k
    tot, rows, o = {}, [], 0
    for i, n in enumerate(lengths):
        sl = slice(o, o + n)
        one = ops.agg_backward(x[sl], pg, fwd[2][sl], fwd[3][i:i + 1], fwd[4][i:i + 1], g["pred"][i], g_classes=g["classes"][sl],
                               g_A=g["A"][sl], g_B=g["B"][i], nonlinear=nonlinear, g_max=g["max"][i], want_g_feats=True)
        rows.append(one.pop("feats").double().cpu())
        for k, v in one.items():
            tot[k] = tot.get(k, 0) + v.double().cpu()
        o += n
    tot["feats"] = torch.cat(rows)
    _check(a, tot, "batched vs the sum of one-bag calls")


def test_a_nan_bag_stays_in_its_rows():
    from dsmil_wsi_amd import ops
    p, K, C, nonlinear, _ = _weights("tcga")
    for lengths in ([300, 100, 1000], [30000, 200, 40000]):       # both tile regimes; the NaN bag is the middle one
        x = _batch(lengths, K, 13).cuda()
        pg = {k: v.cuda() for k, v in p.items()}
        fwd = [t.clone() for t in ops.agg_forward(x, lengths, pg, nonlinear=nonlinear)]
        o, n = lengths[0], lengths[1]
        x[o:o + n] = float("nan")
        fwd[2][o:o + n] = float("nan")       # the forward of a NaN bag: NaN attention and bag embedding, any index
        fwd[3][1] = float("nan")
        g = {k: v.cuda() for k, v in _upstream("pm", lengths, C, K, np.random.default_rng(1)).items()}
        g["pred"][1] = 0
        g["max"][1] = 0
        got = _native(x, lengths, pg, fwd, g, None, nonlinear, True, False)["feats"]
        assert torch.isfinite(got[:o]).all() and torch.isfinite(got[o + n:]).all(), lengths
        assert not torch.isfinite(got[o:o + n]).all()


@pytest.mark.parametrize("tag,passing_v", [("tcga", False), ("passv", True)])
def test_forward_batch_and_batch_loss_follow_the_cpu_module(tag, passing_v):
    """MILNet.forward_batch under autograd (dense upstream, input rows included; with passing_v the value layer's
    gradients) and MILNet.batch_loss against the same module on the CPU in fp64."""
    K, C, nonlinear, _ = VARIANT[tag]
    lengths = [37, 700, 129, 2000]
    x = _batch(lengths, K, 31)
    rng = np.random.default_rng(12)
    w = [torch.from_numpy(rng.standard_normal(s).astype(np.float32)) for s in
         ((sum(lengths), C), (len(lengths), C), (sum(lengths), C), (len(lengths), C, K))]
    labels = torch.from_numpy((rng.random((len(lengths), C)) > 0.5).astype(np.float32))
    res = []
    for dev in ("cpu", "cuda"):
        net = build_net(tag, dev).eval()
        if dev == "cpu":
            net = net.double()
        dt = torch.float64 if dev == "cpu" else torch.float32
        xd = x.to(dev, dt).requires_grad_(True)
        outs = net.forward_batch(xd, lengths)
        sum((o * g.to(dev, dt)).sum() for o, g in zip(outs, w)).backward()
        grads = {k: v.grad.clone() for k, v in net.named_parameters()}
        grads["x"] = xd.grad.clone()
        net.zero_grad()
        loss, pred, mx = net.batch_loss(x.to(dev, dt), lengths, labels.to(dev, dt))
        loss.backward()
        res.append((outs, grads, loss.detach(), {k: v.grad.clone() for k, v in net.named_parameters() if v.grad is not None}))
    (o0, g0, l0, b0), (o1, g1, l1, b1) = res
    assert abs(float(l0) - float(l1)) <= 1e-5
    _check({k: v for k, v in g1.items()}, {k: v.cpu() for k, v in g0.items()}, f"{tag} forward_batch")
    _check({k: v for k, v in b1.items()}, {k: v.cpu() for k, v in b0.items()}, f"{tag} batch_loss")


def test_short_training_run_follows_the_cpu_module_path(monkeypatch):
    """training.train(bags_per_step = 8), 6 groups, on the GPU against the same loop on the CPU module path: per-bag losses
    to 1e-5 max(1, |loss|), parameters to 1e-4 of their scale (the bars of test_fused_train_step_follows_the_generic_path).
    The optimiser is SGD with momentum: its update is linear in the gradient, so the parameter bar bounds the summed
    gradient difference of the two devices.  Adam (the fused test's choice, where both sides run the SAME kernels) divides
    by sqrt(v): a gradient element whose exact value is near zero gets a step of the full learning rate with the sign of its
    rounding error, which differs between a CPU and a GPU summation order — measured with Adam(lr 1e-3): losses within the
    bar, but 1 % of q.0.weight off by up to 2.9e-4 (bar 1.5e-5).  That measures the optimiser's conditioning, not the backward."""
    from dsmil_wsi_amd import training as T
    K, C, nonlinear, _ = VARIANT["tcga"]
    n = 48
    rng = np.random.default_rng(5)
    sizes = rng.integers(50, 3000, n)
    bags = {i: (torch.from_numpy(make_bag(500 + i, int(sizes[i]), K)), torch.tensor([float(i % 2), float((i // 2) % 2)]))
            for i in range(n)}

    class Cache:
        def __init__(self, dev):
            self.dev = dev

        def get(self, item, feats_size=None):
            return bags[item][0].to(self.dev), bags[item][1].to(self.dev)
    hp = dict(lr=0.05, momentum=0.9, weight_decay=1e-3)
    crit = torch.nn.BCEWithLogitsLoss()
    args = types.SimpleNamespace(feats_size=K, dropout_patch=0, bags_per_step=8)
    out = {}
    seen = []
    orig = T.batch_loss

    def recording(*a, **kw):
        r = orig(*a, **kw)
        seen.append(r[3].detach().cpu())
        return r
    monkeypatch.setattr(T, "batch_loss", recording)
    for dev in ("cpu", "cuda"):
        seen.clear()
        net = build_net("tcga", dev).train()
        opt = torch.optim.SGD(net.parameters(), **hp)
        steps = []
        opt.register_step_post_hook(lambda *a: steps.append(1))
        np.random.seed(3)
        buf = io.StringIO()
        with redirect_stdout(buf):
            T.train(args, list(range(n)), net, crit, opt, cache=Cache(dev))
        assert len(steps) == 6
        assert len([s for s in buf.getvalue().split("\r") if s.strip()]) == n      # one reported loss per bag
        losses = torch.cat(seen).tolist()
        assert len(losses) == n
        out[dev] = (losses, {k: v.detach().cpu().numpy() for k, v in net.named_parameters()})
    for a, b in zip(out["cpu"][0], out["cuda"][0]):
        assert abs(a - b) <= 1e-5 * max(1.0, abs(a)), (a, b)
    start = {k: v.detach().numpy() for k, v in build_net("tcga", "cpu").named_parameters()}
    for k, a in out["cpu"][1].items():
        print(f"{k}: moved {float(np.abs(a - start[k]).max()):.3e}, devices differ by {float(np.abs(out['cuda'][1][k] - a).max()):.3e}")
    assert max(float(np.abs(a - start[k]).max()) for k, a in out["cpu"][1].items()) > 1e-3      # the run moved the weights
    for k, a in out["cpu"][1].items():
        np.testing.assert_allclose(out["cuda"][1][k], a, atol=1e-4 * max(1e-3, float(np.abs(a).max())), rtol=0, err_msg=k)
