"""Training the value layer of BClassifier(passing_v=True) on bf16-stored rows: ops.value_proj_backward on bf16 operands
(dsmil_value_backward_bf16: k_value_tn_b16, csrc/agg_value.h) and the opted-in module routes through it, against the fp64
formulas of tests/value_bwd_b16_cases.py and tests/bwd_b16_cases.py.  The bar is the backward's own in this project
(2e-4 of the tensor's max-abs + 2e-5; tests/test_value_bwd_b16_host.py shows the kernel's arithmetic reaches it).
Needs a real MI355X."""
import numpy as np
import pytest
import torch

import bwd_b16_cases as bc
import value_bwd_b16_cases as cs
from inputs import make_bag
from util import build_net

pytestmark = pytest.mark.gpu


def _dev(a, dtype=None):
    t = torch.from_numpy(np.array(a)).cuda()                # (a copy: the shared cases are read-only)
    return t if dtype is None else t.to(dtype)


def _host(t):
    return t.detach().float().cpu().numpy().astype(np.float64)


def _check(tag, got, ref):
    err, lim = cs.max_err(_host(got).reshape(ref.shape), ref), cs.bar(ref)
    print(f"{tag}: err {err:.3e} = {err / lim:.4f} of the bar {lim:.3e}")
    assert err <= lim, f"{tag}: max err {err:.3e} > {lim:.3e}"


def _operands(rows, K, Kv):
    x, V, g = cs.make_case(rows, K, Kv)
    return _dev(x, torch.bfloat16), _dev(V, torch.bfloat16), _dev(g)


# ---- 1. the kernel bar ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows,K,Kv", cs.SHAPES)
def test_kernel_bar(rows, K, Kv):
    from dsmil_wsi_amd import ops
    xb, Vb, g = _operands(rows, K, Kv)
    g_w, g_b = ops.value_proj_backward(xb, Vb, g)
    assert g_w.dtype == torch.float32 and g_b.dtype == torch.float32 and g_w.shape == (Kv, K) and g_b.shape == (Kv,)
    ref_w, ref_b = cs.reference(rows, K, Kv)
    _check(f"{rows}x{K}x{Kv} g_v_w", g_w, ref_w)
    _check(f"{rows}x{K}x{Kv} g_v_b", g_b, ref_b)


# ---- 2. two runs, the same bits -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows,K,Kv", cs.BITS)
def test_two_runs_give_the_same_bits(rows, K, Kv):
    from dsmil_wsi_amd import ops
    from util import poison_workspace
    xb, Vb, g = _operands(rows, K, Kv)
    a = [t.clone() for t in ops.value_proj_backward(xb, Vb, g)]
    poison_workspace(ops)                                   # (nothing of the first run may survive into the second)
    b = ops.value_proj_backward(xb, Vb, g)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


# ---- 3. the mask is a select ----------------------------------------------------------------------------------------------------
def test_mask_is_a_select_on_the_bf16_value():
    from dsmil_wsi_amd import ops
    rows, K, Kv = 129, 72, 68
    x, V, g = (a.copy() for a in cs.make_case(rows, K, Kv))
    V[:, 5] = 0.0                                           # an all-zero column
    V[3, :] = 0.0                                           # +0
    V[70, :] = -0.0                                         # -0 (bits 0x8000)
    Vb = _dev(V, torch.bfloat16)
    assert int((Vb.view(torch.int16) == -32768).sum()) == Kv and bool(Vb[70].eq(0).all())
    dead = ~(V > 0)
    assert 0.3 < dead.mean() < 0.8
    g0 = g.copy()
    g0[dead] = 0.0
    gbad = g.copy()
    gbad[dead] = np.resize(np.array([np.nan, np.inf, -np.inf], np.float32), int(dead.sum()))
    xb = _dev(x, torch.bfloat16)
    clean = [t.clone() for t in ops.value_proj_backward(xb, Vb, _dev(g0))]
    got = ops.value_proj_backward(xb, Vb, _dev(gbad))
    for name, u, v in zip(("g_v_w", "g_v_b"), got, clean):
        assert bool(torch.isfinite(u).all()), name
        assert torch.equal(u, v), name
    assert not bool(got[0][5].any()) and float(got[1][5]) == 0.0
    ref_w, ref_b = cs.grads_f64(x, V, gbad)
    _check("mask g_v_w", got[0], ref_w)
    _check("mask g_v_b", got[1], ref_b)


# ---- 4. against the fp32 route on the widened operands --------------------------------------------------------------------------
@pytest.mark.parametrize("rows,K,Kv", [(129, 72, 68), (700, 512, 512)])
def test_against_the_fp32_route_on_widened_operands(rows, K, Kv):
    """dsmil_value_backward on x.float(), V.float(): both routes within the bar of fp64 (not bit for bit: the fp32 kernel
    drops three of its nine plane products, this one keeps all of its three)."""
    from dsmil_wsi_amd import ops
    xb, Vb, g = _operands(rows, K, Kv)
    ref_w, ref_b = cs.reference(rows, K, Kv)
    new = ops.value_proj_backward(xb, Vb, g)
    old = ops.value_proj_backward(xb.float(), Vb.float(), g)
    for tag, (g_w, g_b) in (("bf16 route", new), ("fp32 route", old)):
        _check(f"{tag} {rows}x{K}x{Kv} g_v_w", g_w, ref_w)
        _check(f"{tag} {rows}x{K}x{Kv} g_v_b", g_b, ref_b)


# ---- 5. the module, opted in ----------------------------------------------------------------------------------------------------
V_KEYS = ("v_w", "v_b")


def _net(K, opt_in=True, dtype=None):
    net = cs.module_net(K).cuda()
    if dtype is not None:
        net = net.to(dtype)
    net.b_classifier.train_value_on_bf16 = opt_in
    return net.train()


def _grads(net):
    return {cs.ORACLE_NAMES[k]: v.grad for k, v in net.named_parameters()}


def _bce_backward(net, xb, y):
    """loss = 0.5 BCE(bag) + 0.5 BCE(max instance) on net(xb) (tests/test_bwd_b16_gpu.py::
    test_module_forward_bce_backward_on_bf16_rows); returns the upstream gradients that arrived at the bf16 outputs."""
    ins, bag, _, _ = net(xb)
    assert ins.dtype == torch.bfloat16 and ins.requires_grad and bag.requires_grad
    ins.retain_grad(); bag.retain_grad()
    crit = torch.nn.BCEWithLogitsLoss()
    mx, _ = torch.max(ins, 0)
    loss = 0.5 * crit(bag.float().view(1, -1), y) + 0.5 * crit(mx.float().view(1, -1), y)
    loss.backward()
    return {"pred": _host(bag.grad).reshape(-1), "classes": _host(ins.grad)}


def _module_reference(net, x, xb, g):
    """The fp64 gradient of all ten parameters at the bf16 rows and the bf16-rounded parameters, straight-through: the
    forward's own A, B, idx and the mask of the device's own V.  Also checks that mask against the reference's sign wherever the
    forward's accumulation bar decides it, and that the undecided share is under the cap."""
    from dsmil_wsi_amd import ops
    w = {cs.ORACLE_NAMES[k]: v.detach() for k, v in net.named_parameters()}
    V = ops.value_proj(xb, w["v_w"], w["v_b"])
    assert V.dtype == torch.bfloat16
    _, _, A, B, idx = (t.cpu().numpy() for t in ops.agg_forward(xb, [xb.shape[0]], w, vals=V))
    p = cs.module_params(net)
    Vh = V.float().cpu().numpy()
    ref = bc.formula_f64(x, Vh, p, A, B[0], idx[0], g, True)
    ref["v_w"], ref["v_b"] = cs.grads_f64(x, Vh, ref.pop("vals"))
    z, decided = cs.mask_band(x, p)
    share = 1.0 - float(decided.mean())
    print(f"mask band: {share:.2e} of V undecided; device mask live {float((Vh > 0).mean()):.3f}")
    assert share <= cs.BAND_CAP, f"inconclusive: {share:.2e} of the value layer's outputs lie inside the accumulation bar"
    assert np.array_equal((Vh > 0)[decided], (z > 0)[decided])
    return ref


@pytest.mark.parametrize("K,N", cs.MODULE_CASES)
def test_module_trains_the_value_layer_on_bf16_rows(K, N):
    x = cs.module_rows(K, N)
    xb = _dev(x, torch.bfloat16)
    net = _net(K)
    g = _bce_backward(net, xb, torch.tensor([[0.0, 1.0]], device="cuda"))
    grads = _grads(net)
    assert all(v is not None and v.dtype == torch.float32 for v in grads.values())
    ref = _module_reference(net, x, xb, g)
    for k in V_KEYS + tuple(bc.KEYS):
        _check(f"K={K} N={N} {k}", grads[k], ref[k])


# ---- 6. / 7. bag_loss, batch_loss, forward_batch: one value-backward call, fp32 g_vals, the caller's bf16 rows ---------------------
LENGTHS = [1, 33, 129]


class _Spy:
    def __init__(self, ops):
        self.real, self.seen = ops.value_proj_backward, []

    def __call__(self, feats, V, g_vals, row_map=None):
        self.seen.append((feats.dtype, V.dtype, g_vals.dtype, feats.data_ptr(), tuple(feats.shape), tuple(g_vals.shape), row_map))
        return self.real(feats, V, g_vals, row_map)


def test_batch_loss_is_the_mean_of_the_bag_losses_in_one_value_backward_call(monkeypatch):
    from dsmil_wsi_amd import ops
    K, T = 64, sum(LENGTHS)
    xb = _dev(cs.module_rows(K, T), torch.bfloat16)
    labels = torch.tensor([[1.0, 0.0], [0.0, 1.0], [1.0, 1.0]], device="cuda")
    off = np.concatenate([[0], np.cumsum(LENGTHS)])
    spy = _Spy(ops)
    monkeypatch.setattr(ops, "value_proj_backward", spy)
    # the three bags one by one
    net = _net(K)
    ones, mean = [], None
    for b, n in enumerate(LENGTHS):
        net.zero_grad(set_to_none=True)
        rows = xb[int(off[b]):int(off[b + 1])]
        loss = net.bag_loss(rows, labels[b])[0]
        assert loss.dtype == torch.float32
        loss.backward()
        ones.append(loss.item())
        assert len(spy.seen) == b + 1 and spy.seen[-1][3] == rows.data_ptr() and spy.seen[-1][4] == (n, K)
        gr = {k: _host(v) / len(LENGTHS) for k, v in _grads(net).items()}
        mean = gr if mean is None else {k: mean[k] + gr[k] for k in gr}
    # the batch
    spy.seen.clear()
    net.zero_grad(set_to_none=True)
    loss, pred, mx = net.batch_loss(xb, LENGTHS, labels)
    assert pred.dtype == torch.float32 and pred.shape == (3, 2) and mx.shape == (3, 2)
    loss.backward()
    print("batch loss", loss.item(), "mean of the bags'", float(np.mean(ones)))
    assert abs(loss.item() - float(np.mean(ones))) <= 1e-6
    assert len(spy.seen) == 1, spy.seen                                # ONE call over the concatenated rows
    fd, vd, gd, ptr, fshape, gshape, rmap = spy.seen[0]
    assert gd == torch.float32 and fd == torch.bfloat16 and vd == torch.bfloat16
    assert ptr == xb.data_ptr() and fshape == (T, K) and gshape == (T, K) and rmap is None
    grads = _grads(net)
    for k in V_KEYS + tuple(bc.KEYS):
        _check(f"batch_loss {k}", grads[k], mean[k])
    # forward_batch: differentiable, bf16 outputs, the same single call
    spy.seen.clear()
    net.zero_grad(set_to_none=True)
    classes, pred, A, B = net.forward_batch(xb, LENGTHS)
    assert classes.dtype == torch.bfloat16 and pred.shape == (3, 2) and B.shape == (3, 2, K)
    (pred.float().sum() + B.float().square().sum()).backward()
    assert len(spy.seen) == 1 and spy.seen[0][2] == torch.float32 and spy.seen[0][3] == xb.data_ptr()
    assert net.b_classifier.v[1].weight.grad is not None and bool(net.b_classifier.v[1].weight.grad.any())


def test_forward_hands_over_fp32_g_vals_and_the_callers_rows(monkeypatch):
    from dsmil_wsi_amd import ops
    spy = _Spy(ops)
    monkeypatch.setattr(ops, "value_proj_backward", spy)
    xb = _dev(cs.module_rows(512, 129), torch.bfloat16)
    y = torch.tensor([[0.0, 1.0]], device="cuda")
    for call in ("milnet", "bclassifier"):
        net = _net(512)
        spy.seen.clear()
        if call == "milnet":
            _bce_backward(net, xb, y)
        else:
            _, c = net.i_classifier(xb)
            pred, A, B = net.b_classifier(xb, c.detach())
            assert pred.dtype == torch.bfloat16
            pred.float().sum().backward()
        assert len(spy.seen) == 1, (call, spy.seen)
        fd, vd, gd, ptr, fshape, gshape, rmap = spy.seen[0]
        assert gd == torch.float32 and fd == torch.bfloat16 and vd == torch.bfloat16, call
        assert ptr == xb.data_ptr() and fshape == (129, 512) and gshape == (129, 512) and rmap is None, call
        assert net.b_classifier.v[1].weight.grad is not None and net.b_classifier.v[1].bias.grad is not None


# ---- 8. a module after .bfloat16() gets bf16 gradients --------------------------------------------------------------------------
def test_bfloat16_module_gets_bf16_value_gradients():
    K, N = 512, 129
    x = cs.module_rows(K, N)
    xb = _dev(x, torch.bfloat16)
    net = _net(K, dtype=torch.bfloat16)
    g = _bce_backward(net, xb, torch.tensor([[0.0, 1.0]], device="cuda"))
    ref = _module_reference(net, x, xb, g)
    grads = _grads(net)
    for k in V_KEYS + tuple(bc.KEYS):
        assert grads[k] is not None and grads[k].dtype == torch.bfloat16, k
        r = ref[k]
        err = np.abs(_host(grads[k]).reshape(r.shape) - r)
        lim = cs.bar(r) + 2.0 ** -8 * np.abs(r)             # the fp32 gradient inside the bar, then ONE rounding to bf16
        print(f"bfloat16 module {k}: worst err / limit {float((err / lim).max()):.4f}")
        assert np.all(err <= lim), k


# ---- 9. the default and what stays refused --------------------------------------------------------------------------------------
def test_default_and_refusals():
    from dsmil_wsi_amd import modules as M
    from dsmil_wsi_amd import ops
    assert M.BClassifier.train_value_on_bf16 is False
    K = bc.VARIANT["passv"][0]
    xb = _dev(make_bag(2, 40, K), torch.bfloat16)
    y = torch.zeros(2, device="cuda")
    # an un-opted module refuses as before
    net = build_net("passv", "cuda").train()
    assert net.b_classifier.train_value_on_bf16 is False
    for call in (lambda: net(xb), lambda: net.bag_loss(xb, y), lambda: net.batch_loss(xb, [40], y.view(1, 2)),
                 lambda: net.forward_batch(xb, [40]), lambda: net.b_classifier(xb, torch.zeros(40, 2, device="cuda"))):
        with pytest.raises(NotImplementedError, match="passing_v"):
            call()
    # opted in: bf16 rows that themselves require a gradient are still refused
    net.b_classifier.train_value_on_bf16 = True
    xr = xb.clone().requires_grad_(True)
    for call in (lambda: net(xr), lambda: net.bag_loss(xr, y), lambda: net.batch_loss(xr, [40], y.view(1, 2)),
                 lambda: net.forward_batch(xr, [40])):
        with pytest.raises(NotImplementedError):
            call()
    # ops: no row map on the bf16 route; K = 166 is not a width of the bf16 path
    Vb, g = torch.zeros(40, K, dtype=torch.bfloat16, device="cuda"), torch.zeros(40, K, device="cuda")
    with pytest.raises(ValueError, match="row_map is implemented for the fp32 path"):
        ops.value_proj_backward(xb, Vb, g, row_map=torch.arange(40, device="cuda"))
    with pytest.raises(ValueError):
        ops.value_proj_backward(xb, Vb.float(), g)
    with pytest.raises(ValueError):
        ops.value_proj_backward(xb, Vb, g.to(torch.bfloat16))
    z = lambda *s: torch.zeros(*s, dtype=torch.bfloat16, device="cuda")
    with pytest.raises(RuntimeError, match="unsupported"):
        ops.value_proj_backward(z(40, 166), z(40, 166), torch.zeros(40, 166, device="cuda"))
    # a frozen value layer stays a constant: the rest trains
    for q in net.b_classifier.v.parameters():
        q.requires_grad_(False)
    net.bag_loss(xb, y)[0].backward()
    assert net.b_classifier.fcc.weight.grad is not None and net.b_classifier.v[1].weight.grad is None


def test_active_dropout_keeps_the_torch_route(monkeypatch):
    """Opted in, an ACTIVE dropout of the value layer is still torch's own (nn.Linear + ReLU on the dropped rows), as
    tests/test_value_b16_gpu.py::test_active_dropout_on_bf16_rows_keeps_the_torch_route pins it without the opt-in: neither
    native value call runs, classes / A equal the eval-mode results, B does not.  Its V reaches the aggregator as
    caller-supplied vals, which get no gradient on bf16 rows — under autograd the backward refuses, as it did."""
    from dsmil_wsi_amd import modules as M
    from dsmil_wsi_amd import ops
    spy = _Spy(ops)
    monkeypatch.setattr(ops, "value_proj_backward", spy)
    net = M.MILNet(M.FCLayer(64, 2), M.BClassifier(64, 2, dropout_v=0.5, passing_v=True)).cuda().to(torch.bfloat16)
    net.b_classifier.train_value_on_bf16 = True
    xb = _dev(make_bag(5, 100, 64), torch.bfloat16)
    with torch.no_grad():
        ev = net.eval()(xb)
    projected = []
    real = ops.value_proj
    monkeypatch.setattr(ops, "value_proj", lambda *a, **k: projected.append(1) or real(*a, **k))
    tr = net.train()(xb)
    assert projected == []
    assert torch.equal(ev[0], tr[0]) and torch.equal(ev[2], tr[2]) and not torch.equal(ev[3], tr[3])
    assert all(bool(torch.isfinite(t.float()).all()) for t in tr)
    with pytest.raises(NotImplementedError):
        tr[1].float().sum().backward()
    assert spy.seen == []


# ---- 10. it trains --------------------------------------------------------------------------------------------------------------
def test_passing_v_model_trains_on_a_bf16_cache():
    from dsmil_wsi_amd import training as T
    rng = np.random.default_rng(0)
    direction = rng.standard_normal(64).astype(np.float32)
    bags = []
    for b in range(8):
        lab = b % 2
        X = rng.standard_normal((60 + 7 * b, 64)).astype(np.float32)
        if lab:
            X[:6] += 2.5 * direction
        lab2 = np.tile(np.array([[lab, 1 - lab]], np.float32), (X.shape[0], 1))
        bags.append(torch.from_numpy(np.concatenate([X, lab2], 1)).cuda())
    cache = T.BagCache(torch.device("cuda"), 64, dtype=torch.bfloat16)
    net = build_net("passv", "cuda").train()
    net.b_classifier.train_value_on_bf16 = True
    v_w0 = net.b_classifier.v[1].weight.detach().clone()
    opt = torch.optim.Adam(net.parameters(), lr=2e-3)
    epochs = []
    for _ in range(6):
        total = 0.0
        for bag in bags:
            feats, label = cache.get(bag)
            assert feats.dtype == torch.bfloat16
            opt.zero_grad()
            loss = net.bag_loss(feats, label)[0]
            loss.backward()
            opt.step()
            total += loss.item()
        epochs.append(total / len(bags))
    print("losses", [f"{v:.4f}" for v in epochs])
    assert epochs[-1] < 0.8 * epochs[0], epochs
    assert not torch.equal(net.b_classifier.v[1].weight.detach(), v_w0)
    assert float((net.b_classifier.v[1].weight.detach() - v_w0).abs().max()) > 1e-4
