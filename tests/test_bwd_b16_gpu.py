"""Training on bf16-stored rows: dsmil_agg_backward_bags_bf16 (csrc/agg_bwd_bags.h) through ops and the modules against
formula_f64 of tests/bwd_b16_cases.py — the analytic gradient at the bf16 rows and the bf16-rounded weights, fed the
forward's own A, B, idx.  The bar is the fp32 backward's own (2e-4 of the tensor's max-abs + 2e-5): the operands are exact
bf16 MFMA operands, so nothing looser is justified.  Needs a real MI355X."""
import argparse

import numpy as np
import pytest
import torch

import bwd_b16_cases as bc
from inputs import make_bag
from util import build_net

pytestmark = pytest.mark.gpu

NAMES = {"i_classifier.fc.0.weight": "fc_w", "i_classifier.fc.0.bias": "fc_b", "b_classifier.q.0.weight": "q0_w",
         "b_classifier.q.0.bias": "q0_b", "b_classifier.q.2.weight": "q2_w", "b_classifier.q.2.bias": "q2_b",
         "b_classifier.fcc.weight": "fcc_w", "b_classifier.fcc.bias": "fcc_b"}


def _dev(d):
    return {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in d.items()}


def _b16(x):
    return torch.from_numpy(x).cuda().to(torch.bfloat16)


def _within_bar(got, ref, tag, keys=None):
    worst = 0.0
    for k in keys or ref:
        r = ref[k]
        err, b = bc.max_err(got[k].detach().float().cpu().numpy().reshape(r.shape), r), bc.bar(r)
        print(f"{tag} {k}: err {err:.3e} = {err / b:.3f} of the bar (scale {float(np.abs(r).max()):.3e})")
        assert err <= b, f"{tag} {k}: max err {err:.3e} > {b:.3e}"
        worst = max(worst, err / b)
    return worst


def _run_case(tag, N):
    """(got, ref) of one (tag, N) case: forward on the bf16 rows, backward with its A, B, idx, formula_f64 fed the same."""
    from dsmil_wsi_amd import ops
    x, p, g = bc.make_case(tag, N)
    _, _, nonlinear = bc.variant(tag)
    xb, w, gg = _b16(x), _dev(p), _dev(g)
    _, _, A, B, idx = ops.agg_forward(xb, [N], w, nonlinear=nonlinear)
    got = ops.agg_backward(xb, w, A, B, idx, gg["pred"], g_classes=gg["classes"], g_A=gg["A"], g_B=gg["B"],
                           nonlinear=nonlinear, want_g_vals=True)
    torch.cuda.synchronize()
    ref = bc.formula_f64(x, None, p, A.cpu().numpy(), B[0].cpu().numpy(), idx[0].cpu().numpy(), g, nonlinear)
    return got, ref


def _batch_case():
    """The batch case: rows, rounded weights, lengths and dense upstream gradients laid end to end."""
    cases = [bc.make_case("tcga", n, seed=1000 * (b + 1)) for b, n in enumerate(bc.BATCH)]
    x = np.concatenate([c[0] for c in cases])
    g = {"pred": np.stack([c[2]["pred"] for c in cases]), "classes": np.concatenate([c[2]["classes"] for c in cases]),
         "A": np.concatenate([c[2]["A"] for c in cases]), "B": np.stack([c[2]["B"] for c in cases])}
    return x, cases[0][1], g, [c[2] for c in cases]


def _sum_of_formulas(x, p, A, B, idx, gs, scale=1.0):
    """Sum over the bags of the per-bag formula (parameter gradients), g_vals laid end to end."""
    off = np.concatenate([[0], np.cumsum(bc.BATCH)])
    total = None
    for b, g in enumerate(gs):
        sl = slice(int(off[b]), int(off[b + 1]))
        r = bc.formula_f64(x[sl], None, p, A[sl], B[b], idx[b], g, True)
        vals = r.pop("vals")
        if total is None:
            total = {k: v * scale for k, v in r.items()}
            total["vals"] = [vals]
        else:
            for k, v in r.items():
                total[k] = total[k] + v * scale
            total["vals"].append(vals)
    total["vals"] = np.concatenate(total["vals"]) * scale
    return total


# ---- (a) the kernel bar ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag,N", bc.CASES)
def test_kernel_bar(tag, N):
    got, ref = _run_case(tag, N)
    _within_bar(got, ref, f"{tag} N={N}")


def test_kernel_bar_batch():
    from dsmil_wsi_amd import ops
    x, p, g, gs = _batch_case()
    xb, w, gg = _b16(x), _dev(p), _dev(g)
    _, _, A, B, idx = ops.agg_forward(xb, bc.BATCH, w)
    got = ops.agg_backward_bags(xb, bc.BATCH, w, A, B, idx, gg["pred"], g_classes=gg["classes"], g_A=gg["A"], g_B=gg["B"],
                                want_g_vals=True)
    torch.cuda.synchronize()
    ref = _sum_of_formulas(x, p, A.cpu().numpy(), B.cpu().numpy(), idx.cpu().numpy(), gs)
    _within_bar(got, ref, "batch")


# ---- (b) two runs, the same bits -----------------------------------------------------------------------------------------
def test_two_runs_give_the_same_bits():
    from dsmil_wsi_amd import ops
    x, p, g = bc.make_case("tcga", 700)
    xb, w, gg = _b16(x), _dev(p), _dev(g)
    _, _, A, B, idx = ops.agg_forward(xb, [700], w)
    run = lambda: {k: v.clone() for k, v in ops.agg_backward(
        xb, w, A, B, idx, gg["pred"], g_classes=gg["classes"], g_A=gg["A"], g_B=gg["B"], want_g_vals=True).items()}
    a, b = run(), run()
    for k in a:
        assert torch.equal(a[k], b[k]), k
    x, p, g, _ = _batch_case()
    xb, gg = _b16(x), _dev(g)
    _, _, A, B, idx = ops.agg_forward(xb, bc.BATCH, w)
    run = lambda: {k: v.clone() for k, v in ops.agg_backward_bags(
        xb, bc.BATCH, w, A, B, idx, gg["pred"], g_classes=gg["classes"], g_A=gg["A"], g_B=gg["B"], want_g_vals=True).items()}
    a, b = run(), run()
    for k in a:
        assert torch.equal(a[k], b[k]), "batch " + k


# ---- (c) the module path ---------------------------------------------------------------------------------------------------
def _loss_head_f64(classes, pred, idx, y):
    """The two logit gradients of 0.5 BCE(bag) + 0.5 BCE(max instance) (train_tcga.py:67-71) from fp32 logits, in fp64."""
    C = y.size
    zb, zm = pred.reshape(-1).astype(np.float64), classes[idx, np.arange(C)].astype(np.float64)
    sig = lambda z: 1.0 / (1.0 + np.exp(-z))
    return 0.5 * (sig(zb) - y) / C, 0.5 * (sig(zm) - y) / C


def _module_reference(net, xb, y):
    """formula_f64 of the training objective at the bf16 rows and the module's bf16-rounded weights."""
    from dsmil_wsi_amd import ops
    w = {NAMES[k]: v.detach().float() for k, v in net.named_parameters()}
    classes, pred, A, B, idx = (t.cpu().numpy() for t in ops.agg_forward(xb, [xb.shape[0]], w))
    g_pred, g_max = _loss_head_f64(classes, pred, idx[0], y)
    p = {k: bc.round_bf16(v.cpu().numpy()) for k, v in w.items()}
    ref = bc.formula_f64(xb.float().cpu().numpy(), None, p, A, B[0], idx[0], {"pred": g_pred, "max": g_max}, True)
    ref.pop("vals")
    return ref


def test_module_bag_loss_trains_fp32_masters_on_bf16_rows():
    N = 333
    xb = _b16(make_bag(8100, N, 512))
    y = torch.tensor([1.0, 0.0], device="cuda")
    net = build_net("tcga", "cuda").train()
    loss, bag, mx = net.bag_loss(xb, y)
    assert loss.dtype == torch.float32 and bag.dtype == torch.float32 and mx.dtype == torch.float32
    loss.backward()
    grads = {NAMES[k]: v.grad for k, v in net.named_parameters()}
    assert all(v is not None and v.dtype == torch.float32 for v in grads.values())
    _within_bar(grads, _module_reference(net, xb, y.cpu().numpy().astype(np.float64)), "bag_loss")


def test_module_forward_bce_backward_on_bf16_rows():
    """net(xb) -> BCE -> backward: the outputs are bf16 (the rows' dtype) and differentiable; the gradients that arrive at
    them are widened to fp32 and go through the same native backward."""
    N = 200
    x = bc.round_bf16(make_bag(8200, N, 512))
    xb = _b16(x)
    y = torch.tensor([[0.0, 1.0]], device="cuda")
    net = build_net("tcga", "cuda").train()
    ins, bag, A, B = net(xb)
    assert ins.dtype == torch.bfloat16 and ins.requires_grad and bag.requires_grad
    ins.retain_grad(); bag.retain_grad()
    crit = torch.nn.BCEWithLogitsLoss()
    mx, _ = torch.max(ins, 0)
    loss = 0.5 * crit(bag.float().view(1, -1), y) + 0.5 * crit(mx.float().view(1, -1), y)
    loss.backward()
    from dsmil_wsi_amd import ops
    w = {NAMES[k]: v.detach() for k, v in net.named_parameters()}
    _, _, A32, B32, idx = (t.cpu().numpy() for t in ops.agg_forward(xb, [N], w))
    p = {k: bc.round_bf16(v.cpu().numpy()) for k, v in w.items()}
    g = {"pred": bag.grad.float().cpu().numpy().reshape(-1), "classes": ins.grad.float().cpu().numpy()}
    ref = bc.formula_f64(x, None, p, A32, B32[0], idx[0], g, True)
    ref.pop("vals")
    grads = {NAMES[k]: v.grad for k, v in net.named_parameters()}
    assert all(v is not None and v.dtype == torch.float32 for v in grads.values())
    _within_bar(grads, ref, "net(xb)")


def test_bfloat16_module_gets_bf16_gradients():
    N = 333
    xb = _b16(make_bag(8100, N, 512))
    y = torch.tensor([1.0, 0.0], device="cuda")
    net = build_net("tcga", "cuda").to(torch.bfloat16).train()
    net.bag_loss(xb, y)[0].backward()
    ref = _module_reference(net, xb, y.cpu().numpy().astype(np.float64))
    for k, prm in net.named_parameters():
        assert prm.grad is not None and prm.grad.dtype == torch.bfloat16, k
        r = ref[NAMES[k]]
        # the fp32 gradient inside the bar, then ONE rounding to bf16: half an ulp of 8 significant bits, <= 2^-8 relative
        err = np.abs(prm.grad.float().cpu().numpy().astype(np.float64).reshape(r.shape) - r)
        assert np.all(err <= bc.bar(r) + 2.0 ** -8 * (np.abs(r) + bc.bar(r))), k


# ---- (d) a row map is one index_select in front of the call -----------------------------------------------------------------
def test_row_map_equals_gathered_bf16_rows():
    N = 900
    xb = _b16(make_bag(8300, N, 512))
    rows = torch.randperm(N, device="cuda", generator=torch.Generator(device="cuda").manual_seed(N))[:600]
    y = torch.tensor([1.0, 0.0], device="cuda")
    out = []
    for mapped in (True, False):
        net = build_net("tcga", "cuda").train()
        loss = net.bag_loss(xb, y, rows)[0] if mapped else net.bag_loss(xb.index_select(0, rows), y)[0]
        loss.backward()
        out.append((loss.item(), {k: q.grad.clone() for k, q in net.named_parameters()}))
    assert out[0][0] == out[1][0]
    for k in out[0][1]:
        assert torch.equal(out[0][1][k], out[1][1][k]), k


# ---- (e) batch_loss -----------------------------------------------------------------------------------------------------------
def test_batch_loss_on_bf16_rows():
    from dsmil_wsi_amd import ops
    x, _, _, _ = _batch_case()
    xb = _b16(x)
    n = len(bc.BATCH)
    labels = torch.tensor([[b % 2, 1 - b % 2] for b in range(n)], dtype=torch.float32, device="cuda")
    net = build_net("tcga", "cuda").train()
    loss, pred, mx, each = net.batch_loss(xb, bc.BATCH, labels, per_bag=True)
    assert each.shape == (n,) and pred.shape == (n, 2) and mx.shape == (n, 2) and pred.dtype == torch.float32
    loss.backward()
    off = np.concatenate([[0], np.cumsum(bc.BATCH)])
    ones = []
    with torch.no_grad():
        for b in range(n):
            ones.append(net.bag_loss(xb[int(off[b]):int(off[b + 1])], labels[b])[0].item())
    print("batch loss", loss.item(), "mean of the bags'", float(np.mean(ones)))
    assert abs(loss.item() - float(np.mean(ones))) <= 1e-6
    np.testing.assert_allclose(each.cpu().numpy(), np.asarray(ones, np.float32), atol=1e-6, rtol=0)
    w = {NAMES[k]: v.detach() for k, v in net.named_parameters()}
    classes, predf, A, B, idx = (t.cpu().numpy() for t in ops.agg_forward(xb, bc.BATCH, w))
    p = {k: bc.round_bf16(v.cpu().numpy()) for k, v in w.items()}
    gs = []
    for b in range(n):
        sl = slice(int(off[b]), int(off[b + 1]))
        g_pred, g_max = _loss_head_f64(classes[sl], predf[b], idx[b], labels[b].cpu().numpy().astype(np.float64))
        gs.append({"pred": g_pred, "max": g_max})
    ref = _sum_of_formulas(x, p, A, B, idx, gs, scale=1.0 / n)
    ref.pop("vals")
    _within_bar({NAMES[k]: v.grad for k, v in net.named_parameters()}, ref, "batch_loss")


# ---- (f) the toy training loop of test_agg_bwd_gpu.py::test_train_loop_uses_fused_objective_and_learns on a bf16 cache ------
@pytest.mark.parametrize("per_step", [1, 4])
def test_train_loop_learns_on_a_bf16_cache(per_step):
    from dsmil_wsi_amd import training as T
    import dsmil as mil
    rng = np.random.default_rng(0)
    direction = rng.standard_normal(64).astype(np.float32)
    bags = []
    for b in range(16):
        lab = b % 2
        X = rng.standard_normal((150 + 11 * b, 64)).astype(np.float32)
        if lab:
            X[:6] += 2.5 * direction
        bags.append(torch.from_numpy(np.concatenate([X, np.full((X.shape[0], 1), lab, np.float32)], 1)).cuda())
    args = argparse.Namespace(feats_size=64, num_classes=1, dropout_patch=0.3, dropout_node=0.0, non_linearity=1,
                              lr=2e-3, weight_decay=1e-4, num_epochs=8, average=False, bags_per_step=per_step)
    torch.manual_seed(0)
    np.random.seed(0)
    net, crit, opt, sched = T.init_model(args, mil, torch.device("cuda"))
    cache = T.BagCache(torch.device("cuda"), 64, dtype=torch.bfloat16)
    assert cache.get(bags[0])[0].dtype == torch.bfloat16 and cache.get(bags[0])[1].dtype == torch.float32
    losses = [T.train(args, bags, net, crit, opt, cache=cache, log=False) for _ in range(8)]
    tl, score, aucs, th = T.test(args, bags, net, crit, cache=cache, log=False)
    print(f"bags_per_step {per_step}: losses {losses[0]:.4f} -> {losses[-1]:.4f}, AUC {aucs[0]:.4f}")
    assert losses[-1] < 0.8 * losses[0], losses
    assert aucs[0] > 0.9, aucs


# ---- (g) end to end against the fp32 path on the widened rows ----------------------------------------------------------------
@pytest.mark.parametrize("tag,N", bc.HOST_DEV_CASES)
def test_against_the_fp32_path_on_widened_rows(tag, N):
    """The bf16 path (bf16 forward: hidden layer rounded once; bf16-row backward) against the fp32 forward + backward on
    xb.float() and the same rounded weights: the two differ by what the hidden rounding does to A, B (dev_host, emulated on
    the host) and by accumulation order: bar = (4 dev_host[k] + 2e-4) scale + 2e-5."""
    from dsmil_wsi_amd import ops
    x, p, g = bc.make_case(tag, N)
    _, _, nonlinear = bc.variant(tag)
    xb, w, gg = _b16(x), _dev(p), _dev(g)
    kw = dict(g_classes=gg["classes"], g_A=gg["A"], g_B=gg["B"], nonlinear=nonlinear)
    _, _, A, B, idx = ops.agg_forward(xb, [N], w, nonlinear=nonlinear)
    got = ops.agg_backward(xb, w, A, B, idx, gg["pred"], **kw)
    xf = xb.float()
    _, _, A32, B32, idx32 = ops.agg_forward(xf, [N], w, nonlinear=nonlinear)
    ref = ops.agg_backward(xf, w, A32, B32, idx32, gg["pred"], **kw)
    assert torch.equal(idx, idx32)
    dev = bc.dev_host(tag, N)
    for k, r in ref.items():
        r = r.cpu().numpy().astype(np.float64)
        scale = float(np.abs(r).max())
        b = (4 * dev[k] + 2e-4) * scale + 2e-5
        err = bc.max_err(got[k].cpu().numpy(), r)
        print(f"(g) {tag} N={N} {k}: err {err:.3e} = {err / b:.3f} of the bar (dev_host {dev[k]:.2e})")
        assert err <= b, (tag, N, k, err, b)


# ---- (h) refusals ---------------------------------------------------------------------------------------------------------------
def test_refusals():
    from dsmil_wsi_amd import ops
    from util import load_weights
    x, p, g = bc.make_case("tcga", 40)
    xb, w, gg = _b16(x), _dev(p), _dev(g)
    _, _, A, B, idx = ops.agg_forward(xb, [40], w)
    rows = torch.arange(40, device="cuda")
    with pytest.raises(ValueError, match="row_map"):
        ops.agg_backward(xb, w, A, B, idx, gg["pred"], row_map=rows)
    with pytest.raises(ValueError, match="row_map"):
        ops.agg_backward_bags(xb, [40], w, A, B, idx, gg["pred"], row_map=rows)
    # K = 166: the bf16 forward's condition
    wm = _dev(load_weights("musk"))
    xm = _b16(make_bag(1, 40, 166))
    zA, zB, zi = torch.zeros(40, 1, device="cuda"), torch.zeros(1, 1, 166, device="cuda"), torch.zeros(1, 1, dtype=torch.int64, device="cuda")
    with pytest.raises(RuntimeError, match="unsupported"):
        ops.agg_backward(xm, wm, zA, zB, zi, torch.zeros(1, device="cuda"))
    with pytest.raises(RuntimeError, match="unsupported"):
        build_net("musk", "cuda").train().bag_loss(xm, torch.tensor([1.0], device="cuda"))
    # bf16 rows that themselves require a gradient
    net = build_net("tcga", "cuda").train()
    y = torch.tensor([1.0, 0.0], device="cuda")
    xr = xb.clone().requires_grad_(True)
    for call in (lambda: net(xr), lambda: net.bag_loss(xr, y), lambda: net.batch_loss(xr, [40], y.view(1, 2)),
                 lambda: net.forward_batch(xr, [40])):
        with pytest.raises(NotImplementedError):
            call()
    with torch.no_grad():
        net(xr)                                    # (without grad mode there is nothing to refuse)
    # passing_v with a trainable value layer: the bf16 value projection has no backward
    netv = build_net("passv", "cuda").train()
    xv = _b16(make_bag(2, 40, bc.VARIANT["passv"][0]))
    yv = torch.zeros(bc.VARIANT["passv"][1], device="cuda")
    for call in (lambda: netv(xv), lambda: netv.bag_loss(xv, yv)):
        with pytest.raises(NotImplementedError, match="passing_v"):
            call()
    for q in netv.b_classifier.v.parameters():
        q.requires_grad_(False)
    netv.bag_loss(xv, yv)[0].backward()           # a frozen value layer is a constant: the rest trains
    assert netv.b_classifier.fcc.weight.grad is not None and netv.b_classifier.v[1].weight.grad is None


# ---- train_tcga.py --feats_dtype bf16, end to end ---------------------------------------------------------------------------------
def test_train_tcga_feats_dtype_bf16(tmp_path, monkeypatch):
    import glob
    import os
    import pandas as pd
    import train_tcga as tt
    from dsmil_wsi_amd import training as T
    monkeypatch.chdir(tmp_path)
    rng = np.random.default_rng(0)
    rows = []
    direction = rng.standard_normal(32).astype(np.float32)
    for b in range(10):
        lab = b % 2
        os.makedirs(f"datasets/toy3/c{lab}", exist_ok=True)
        X = rng.standard_normal((12 + b, 32)).astype(np.float32)
        if lab:
            X[:3] += 3.0 * direction
        path = f"datasets/toy3/c{lab}/bag{b}.csv"
        pd.DataFrame(X).to_csv(path, index=False, float_format="%.4f")
        rows.append((path, lab))
    pd.DataFrame(rows, columns=["0", "label"]).to_csv("datasets/toy3/toy3.csv", index=False)
    seen = []
    split = T.BagCache._split
    monkeypatch.setattr(T.BagCache, "_split", lambda self, *a: seen.append(split(self, *a)[0].dtype) or split(self, *a))
    tt.main(["--dataset", "toy3", "--num_classes", "1", "--feats_size", "32", "--num_epochs", "3", "--lr", "0.002",
             "--eval_scheme", "5-fold-cv", "--feats_dtype", "bf16"])
    assert seen and all(d == torch.bfloat16 for d in seen)
    assert glob.glob("weights/*/fold_*_*.pth")   # (a fold whose test bags score 0 saves nothing)
