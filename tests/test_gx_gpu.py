"""The gradient of the INPUT rows in HIP (csrc/agg_gx.h): dsmil_agg_backward_rows (k_bwd_gx) through
ops.agg_backward(want_g_feats=True), dsmil_value_backward_rows (k_value_gx) through ops.value_proj_backward_rows, and the
module routes that now use them (x.requires_grad_() through MILNet), against fp64 autograd on the CPU given the device's
critical indices.  Needs a real MI355X.

Bar for every gradient, the project's own (tests/test_agg_bwd_gpu.py, tests/test_value_gpu.py):
max|got - ref| <= 2e-4 * max|ref| + 2e-5."""
import ctypes

import numpy as np
import pytest
import torch

from conftest import load_weights
from inputs import make_bag
from util import VARIANT, build_net, poison_workspace

pytestmark = pytest.mark.gpu

KEYS = ("fc_w", "fc_b", "q0_w", "q0_b", "q2_w", "q2_b", "fcc_w", "fcc_b")

# launches of the profiled attend channel (dsmil_profile_collect(0)) during ONE plain loss.backward() (rows that need no
# gradient) of the `tcga` net on a 3000-row bag, recorded from the parent commit 2718779 on an MI355X
PARENT_ATTEND_LAUNCHES_BACKWARD = 0


def _params(tag):
    p = load_weights(tag)
    return {k: torch.from_numpy(np.ascontiguousarray(p[k])) for k in KEYS if k in p}


def _autograd_f64(x, vals, p, idx, nonlinear, g, g_max=None):
    """Plain fp64 restatement (CPU) of FCLayer + BClassifier given the critical indices, the rows a leaf that requires a
    gradient; g_max: upstream gradient of max_n classes[n, :] = classes[idx_c, c]."""
    x = x.double().requires_grad_(True)
    P = {k: v.double().requires_grad_(True) for k, v in p.items()}
    V = vals.double().requires_grad_(True) if vals is not None else x
    c = x @ P["fc_w"].T + P["fc_b"]
    h = x @ P["q0_w"].T + P["q0_b"]
    Q = torch.tanh(torch.relu(h) @ P["q2_w"].T + P["q2_b"]) if nonlinear else h
    s = Q @ Q[idx].T / np.sqrt(128.0)
    A = torch.softmax(s, 0)
    B = A.T @ V
    pred = torch.einsum("ock,ck->o", P["fcc_w"], B) + P["fcc_b"]
    obj = (pred * g["pred"].double()).sum()
    for name, t in (("classes", c), ("A", A), ("B", B)):
        if g.get(name) is not None:
            obj = obj + (t * g[name].double()).sum()
    if g_max is not None:
        obj = obj + (c[idx, torch.arange(c.shape[1])] * g_max.double()).sum()
    obj.backward()
    out = {k: v.grad for k, v in P.items() if v.grad is not None}
    out["feats"] = x.grad
    if vals is not None:
        out["vals"] = V.grad
    return out


def _check(got, ref, tag, skip=()):
    worst = 0.0
    for k, r in ref.items():
        if k in skip:
            continue
        r = np.asarray(r.numpy() if torch.is_tensor(r) else r, np.float64)
        g = got[k].detach().cpu().numpy().astype(np.float64)
        assert g.shape == r.shape, f"{tag} {k}: shape {g.shape} vs {r.shape}"
        scale = max(float(np.abs(r).max()), 1e-12)
        err = float(np.abs(g - r).max())
        print(f"{tag} g_{k}: max err {err:.3e} vs scale {scale:.3e}")
        assert np.isfinite(g).all(), f"{tag} {k}: non-finite values"
        assert err <= 2e-4 * scale + 2e-5, f"{tag} {k}: max err {err:.3e} vs scale {scale:.3e}"
        worst = max(worst, err / (2e-4 * scale + 2e-5))
    return worst


def _upstream(rng, N, C, K, which):
    g = {"pred": torch.from_numpy(rng.standard_normal(C).astype(np.float32))}
    if "c" in which:
        g["classes"] = torch.from_numpy(rng.standard_normal((N, C)).astype(np.float32))
    if "A" in which:
        g["A"] = torch.from_numpy(rng.standard_normal((N, C)).astype(np.float32))
    if "B" in which:
        g["B"] = torch.from_numpy(rng.standard_normal((C, K)).astype(np.float32))
    gm = torch.from_numpy(rng.standard_normal(C).astype(np.float32)) if "m" in which else None
    return g, gm


def _run_rows(x, p, vals, nonlinear, g, gm, passing_v, poison=False, row_map=None):
    """forward + ops.agg_backward with and without want_g_feats on the device -> (with, without, idx)."""
    from dsmil_wsi_amd import ops
    pg = {k: v.cuda() for k, v in p.items()}
    xg = x.cuda()
    vg = vals.cuda() if vals is not None else None
    mg = row_map.cuda() if row_map is not None else None
    N = x.shape[0] if row_map is None else row_map.numel()
    _, _, A, B, idx = ops.agg_forward(xg, [N], pg, vals=vg, nonlinear=nonlinear, row_map=mg)
    gg = {k: v.cuda() for k, v in g.items()}
    kw = dict(g_classes=gg.get("classes"), g_A=gg.get("A"), g_B=gg.get("B"), vals=vg, nonlinear=nonlinear,
              want_g_vals=passing_v, g_max=gm.cuda() if gm is not None else None, row_map=mg)
    plain = {k: v.clone() for k, v in ops.agg_backward(xg, pg, A, B, idx, gg["pred"], **kw).items()}
    if poison:
        poison_workspace(ops)
    got = {k: v.clone() for k, v in ops.agg_backward(xg, pg, A, B, idx, gg["pred"], want_g_feats=True, **kw).items()}
    if poison:
        poison_workspace(ops)
    again = ops.agg_backward(xg, pg, A, B, idx, gg["pred"], want_g_feats=True, **kw)
    torch.cuda.synchronize()
    assert set(got) == set(plain) | {"feats"}
    for k in plain:   # asking for the rows' gradient changes no other gradient by a bit
        assert torch.equal(got[k], plain[k]), f"{k}: differs from the call without want_g_feats"
    for k in got:     # deterministic
        assert torch.equal(got[k], again[k]), f"{k}: two runs differ"
    return got, plain, idx[0].cpu()


CASES = [  # tag, N, which upstream grads are given: p = pred, c = dense classes, A, B, m = sparse g_max
    ("tcga", 1, "pcAB"), ("tcga", 31, "pcAB"), ("tcga", 33, "pc"), ("tcga", 700, "pcAB"), ("c16", 5000, "pcAB"),
    ("musk", 40, "pcAB"), ("musk", 333, "p"), ("tree", 300, "pcAB"), ("linq", 50, "pcAB"), ("linq", 1000, "pA"),
    ("passv", 50, "pcAB"), ("tcga", 70000, "pcAB"),
    ("tcga", 700, "pm"), ("tcga", 700, "pcm"), ("musk", 333, "pm"), ("linq", 1000, "pcmAB"), ("passv", 50, "pm"),
]


@pytest.mark.parametrize("tag,N,which", CASES)
def test_agg_backward_rows_vs_fp64_autograd(tag, N, which):
    """ops.agg_backward(want_g_feats=True): g_feats and every other gradient against fp64 autograd with the rows a leaf;
    parameter gradients bit-identical to the call without want_g_feats; two runs bit-identical; the 70 000-row case on a
    NaN-poisoned workspace."""
    K, C, nonlinear, passing_v = VARIANT[tag]
    rng = np.random.default_rng(77 + N + K)
    x = torch.from_numpy(make_bag(900 + N, N, K))
    p = _params(tag)
    vals = torch.from_numpy(rng.standard_normal((N, K)).astype(np.float32)) if passing_v else None
    g, gm = _upstream(rng, N, C, K, which)
    got, _, idx = _run_rows(x, p, vals, nonlinear, g, gm, passing_v, poison=N >= 70000)
    ref = _autograd_f64(x, vals, p, idx, nonlinear, g, gm)
    assert tuple(got["feats"].shape) == (N, K)
    skip = () if ("c" in which or "m" in which) else ("fc_w", "fc_b")
    for k in skip:
        assert k not in got
    _check(got, ref, f"{tag} N={N} {which}", skip=skip)


@pytest.mark.parametrize("C,N", [(3, 700), (5, 333), (64, 129), (65, 3000)])
def test_agg_backward_rows_many_classes(C, N):
    """C > 2 (the tail of k_bwd_gx walks the classes), dense upstream on everything plus the sparse g_max; C = 65 on a
    NaN-poisoned workspace."""
    K = 512
    rng = np.random.default_rng(1200 + N + C)
    w = {"fc_w": rng.standard_normal((C, K), dtype=np.float32) * 0.05, "fc_b": rng.standard_normal(C, dtype=np.float32) * 0.1,
         "q0_w": rng.standard_normal((128, K), dtype=np.float32) * np.float32(1.0 / np.sqrt(K)),
         "q0_b": rng.standard_normal(128, dtype=np.float32) * 0.1,
         "q2_w": rng.standard_normal((128, 128), dtype=np.float32) * np.float32(1.0 / np.sqrt(128)),
         "q2_b": rng.standard_normal(128, dtype=np.float32) * 0.1,
         "fcc_w": rng.standard_normal((C, C, K), dtype=np.float32) * 0.05, "fcc_b": rng.standard_normal(C, dtype=np.float32) * 0.1}
    p = {k: torch.from_numpy(v) for k, v in w.items()}
    x = torch.from_numpy(make_bag(8200 + N + C, N, K))
    g, gm = _upstream(rng, N, C, K, "pcmAB")
    got, _, idx = _run_rows(x, p, None, True, g, gm, False, poison=C == 65)
    ref = _autograd_f64(x, None, p, idx, True, g, gm)
    _check(got, ref, f"C={C} N={N}")


@pytest.mark.parametrize("kind", ["subset", "permutation"])
def test_agg_backward_rows_row_map(kind):
    """row_map (dropout_patches as an index list): g_feats comes back in LOGICAL row order, i.e. it is the gradient of the
    gathered copy x[row_map]."""
    tag, Np = "tcga", 3000
    K, C, nonlinear, _ = VARIANT[tag]
    rng = np.random.default_rng(5 if kind == "subset" else 6)
    sel = rng.permutation(Np)[:1777 if kind == "subset" else Np].astype(np.int64)
    x = torch.from_numpy(make_bag(4711, Np, K))
    p = _params(tag)
    n = len(sel)
    g, gm = _upstream(rng, n, C, K, "pcmAB")
    rm = torch.from_numpy(sel)
    got, _, idx = _run_rows(x, p, None, nonlinear, g, gm, False, row_map=rm)
    assert tuple(got["feats"].shape) == (n, K)
    ref = _autograd_f64(x[rm], None, p, idx, nonlinear, g, gm)
    _check(got, ref, f"row_map {kind}")
    # and the same bits as the call on the gathered copy
    got2, _, idx2 = _run_rows(x[rm].contiguous(), p, None, nonlinear, g, gm, False)
    assert torch.equal(idx, idx2) and torch.equal(got["feats"], got2["feats"])


# ---- the value layer ---------------------------------------------------------------------------------------------------
def _make_net(K, C, seed, passing_v=True):
    """MILNet(FCLayer, BClassifier) with train_tcga.py:229-239 style weights (tests/test_value_gpu.py's recipe and seeds)
    and the same parameters as fp32 numpy arrays."""
    from dsmil_wsi_amd import modules as M
    net = M.MILNet(M.FCLayer(in_size=K, out_size=C),
                   M.BClassifier(input_size=K, output_class=C, dropout_v=0.0, nonlinear=True, passing_v=passing_v)).eval()
    gen = torch.Generator().manual_seed(seed)
    for m in net.modules():
        if isinstance(m, (torch.nn.Linear, torch.nn.Conv1d)):
            torch.nn.init.orthogonal_(m.weight, generator=gen)
            with torch.no_grad():
                m.bias.copy_(0.05 * torch.randn(m.bias.shape, generator=gen))
    sd = {k: v.detach().numpy().copy() for k, v in net.state_dict().items()}
    p = {NAMES[k]: v for k, v in sd.items()}
    return net.cuda(), p


NAMES = {"i_classifier.fc.0.weight": "fc_w", "i_classifier.fc.0.bias": "fc_b", "b_classifier.q.0.weight": "q0_w",
         "b_classifier.q.0.bias": "q0_b", "b_classifier.q.2.weight": "q2_w", "b_classifier.q.2.bias": "q2_b",
         "b_classifier.v.1.weight": "v_w", "b_classifier.v.1.bias": "v_b", "b_classifier.fcc.weight": "fcc_w",
         "b_classifier.fcc.bias": "fcc_b"}


def _mask_checked(x, p, V, tag):
    """The device's ReLU mask, checked against the fp64 pre-activations (the convention of
    test_backward_passing_v_vs_fp64_autograd): equal wherever |z_ref| > 1e-4, at most 1e-3 of the entries inside the band."""
    z_ref = x.astype(np.float64) @ p["v_w"].astype(np.float64).T + p["v_b"].astype(np.float64)
    mask = V > 0
    clear = np.abs(z_ref) > 1e-4
    share = 1.0 - clear.mean()
    print(f"{tag}: share of |z_ref| <= 1e-4: {share:.2e}; mask flips outside the band: {int((mask != (z_ref > 0))[clear].sum())}")
    assert share <= 1e-3, f"inconclusive: {share:.2e} of the pre-activations lie within the forward bar of zero"
    assert np.array_equal(mask[clear], (z_ref > 0)[clear])
    return mask


@pytest.mark.parametrize("accumulate", [False, True])
@pytest.mark.parametrize("K,N", [(64, 50), (166, 333), (512, 700), (1024, 300)])
def test_value_proj_backward_rows_vs_fp64(K, N, accumulate):
    """ops.value_proj_backward_rows: g_x = (g * (V > 0)) Wv against fp64 with the device's mask; with accumulate on top of a
    buffer that already holds values (the bar then scales with the sum); two runs bit-identical."""
    from dsmil_wsi_amd import ops
    _, p = _make_net(K, 2, 50 + K)
    x = make_bag(900 + N, N, K)
    v_w, v_b = torch.from_numpy(p["v_w"]).cuda(), torch.from_numpy(p["v_b"]).cuda()
    V = ops.value_proj(torch.from_numpy(x).cuda(), v_w, v_b)
    mask = _mask_checked(x, p, V.cpu().numpy(), f"K={K} N={N}")
    rng = np.random.default_rng(31 + K + N)
    g = rng.standard_normal((N, K)).astype(np.float32)
    base = rng.standard_normal((N, K)).astype(np.float32)
    gg = torch.from_numpy(g).cuda()

    def run():
        if accumulate:
            out = torch.from_numpy(base).cuda()
            r = ops.value_proj_backward_rows(V, gg, v_w, out=out, accumulate=True)
            assert r is out
            return r
        return ops.value_proj_backward_rows(V, gg, v_w)
    a, b = run(), run()
    torch.cuda.synchronize()
    assert torch.equal(a, b), "two runs differ"
    ref = (g.astype(np.float64) * mask) @ p["v_w"].astype(np.float64)
    if accumulate:
        ref = ref + base.astype(np.float64)
    _check({"x": a}, {"x": ref}, f"value rows K={K} N={N} accumulate={accumulate}")


# ---- module level --------------------------------------------------------------------------------------------------------
def _objective(net, xg, y):
    crit = torch.nn.BCEWithLogitsLoss()
    ins, bag, _, _ = net(xg)
    mx, _ = torch.max(ins, 0)
    return 0.5 * crit(bag.view(1, -1), y) + 0.5 * crit(mx.view(1, -1), y), ins


def _module_ref(x, p, idx, mask, y):
    """fp64 autograd (CPU) of the objective of train_tcga.py:67-71 with the rows a leaf; mask: the value layer's ReLU mask
    (None: v = Identity)."""
    xt = torch.from_numpy(x).double().requires_grad_(True)
    P = {k: torch.from_numpy(v).double().requires_grad_(True) for k, v in p.items()}
    c = xt @ P["fc_w"].T + P["fc_b"]
    h = xt @ P["q0_w"].T + P["q0_b"]
    Q = torch.tanh(torch.relu(h) @ P["q2_w"].T + P["q2_b"])
    V = xt if mask is None else (xt @ P["v_w"].T + P["v_b"]) * mask
    A = torch.softmax(Q @ Q[idx].T / np.sqrt(128.0), 0)
    B = A.T @ V
    pred = torch.einsum("ock,ck->o", P["fcc_w"], B) + P["fcc_b"]
    mx = c[idx, torch.arange(c.shape[1])]
    crit = torch.nn.BCEWithLogitsLoss()
    loss = 0.5 * crit(pred.view(1, -1), y.view(1, -1)) + 0.5 * crit(mx.view(1, -1), y.view(1, -1))
    loss.backward()
    out = {k: v.grad.numpy() for k, v in P.items()}
    out["x"] = xt.grad.numpy()
    return out


class _NoDense:
    """Inside: _AggFunction._backward_dense and torch.Tensor.mm raise (no dense fallback, no torch product in the
    backward); ops.value_proj calls are counted."""

    def __init__(self, monkeypatch):
        from dsmil_wsi_amd import modules as M
        from dsmil_wsi_amd import ops

        def boom(*a, **k):
            raise AssertionError("the dense torch fallback ran")
        self.calls = {"value_proj": 0, "value_rows": 0, "agg_rows": 0}
        monkeypatch.setattr(M._AggFunction, "_backward_dense", staticmethod(boom))
        monkeypatch.setattr(torch.Tensor, "mm", boom)
        vp, vr, ab = ops.value_proj, ops.value_proj_backward_rows, ops.agg_backward

        def value_proj(*a, **k):
            self.calls["value_proj"] += 1
            return vp(*a, **k)

        def value_rows(*a, **k):
            self.calls["value_rows"] += 1
            return vr(*a, **k)

        def agg_backward(*a, **k):
            self.calls["agg_rows"] += 1 if k.get("want_g_feats") else 0
            return ab(*a, **k)
        monkeypatch.setattr(ops, "value_proj", value_proj)
        monkeypatch.setattr(ops, "value_proj_backward_rows", value_rows)
        monkeypatch.setattr(ops, "agg_backward", agg_backward)


@pytest.mark.parametrize("passing_v,K,N", [(False, 512, 700), (True, 512, 700), (True, 166, 333), (False, 1024, 300)])
def test_module_input_gradient_vs_fp64_autograd(monkeypatch, passing_v, K, N):
    """x.requires_grad_() through MILNet(FCLayer, BClassifier), objective of train_tcga.py:67-71: x.grad and every
    parameter gradient against fp64 autograd; two runs bit-identical; the backward runs no dense fallback and no torch
    product, and a passing_v model with rows that require a gradient goes through ops.value_proj."""
    from dsmil_wsi_amd import ops
    net, p = _make_net(K, 2, 50 + K, passing_v=passing_v)
    net.train()
    x = make_bag(900 + N, N, K)
    y = torch.tensor([[1.0, 0.0]], device="cuda")
    spy = _NoDense(monkeypatch)
    runs = []
    for _ in range(2):
        net.zero_grad(set_to_none=True)
        xg = torch.from_numpy(x).cuda().requires_grad_(True)
        loss, ins = _objective(net, xg, y)
        loss.backward()
        torch.cuda.synchronize()
        gr = {NAMES[k]: prm.grad.clone() for k, prm in net.named_parameters()}
        gr["x"] = xg.grad.clone()
        runs.append(gr)
    assert spy.calls["agg_rows"] == 2, spy.calls
    assert spy.calls["value_proj"] == (2 if passing_v else 0) and spy.calls["value_rows"] == (2 if passing_v else 0), spy.calls
    for k in runs[0]:
        assert torch.equal(runs[0][k], runs[1][k]), f"{k}: two runs differ"
    idx = torch.argmax(ins.detach(), 0).cpu()
    mask = None
    if passing_v:
        with torch.no_grad():
            V = ops.value_proj(torch.from_numpy(x).cuda(), net.b_classifier.v[1].weight.detach(),
                               net.b_classifier.v[1].bias.detach()).cpu().numpy()
        mask = torch.from_numpy(_mask_checked(x, p, V, f"K={K} N={N}")).double()
    ref = _module_ref(x, p, idx, mask, y.cpu().double())
    _check(runs[0], ref, f"module passing_v={passing_v} K={K} N={N}")


def test_two_module_route_input_gradient(monkeypatch):
    """BClassifier.forward(feats, c) with the caller's instance logits (the two-module route, attention_map.py:85): the rows'
    gradient of the aggregator is native there too (the stand-alone FCLayer's own three products stay torch's)."""
    from dsmil_wsi_amd import modules as M
    net, p = _make_net(512, 2, 50 + 512, passing_v=False)
    x = make_bag(1600, 700, 512)
    xg = torch.from_numpy(x).cuda().requires_grad_(True)
    with torch.no_grad():
        c = net.i_classifier(xg)[1]

    def boom(*a, **k):
        raise AssertionError("the dense torch fallback ran")
    monkeypatch.setattr(M._AggFunction, "_backward_dense", staticmethod(boom))
    pred, A, B = net.b_classifier(xg, c)
    pred.sum().backward()
    xt = torch.from_numpy(x).double().requires_grad_(True)
    P = {k: torch.from_numpy(v).double() for k, v in p.items()}
    Q = torch.tanh(torch.relu(xt @ P["q0_w"].T + P["q0_b"]) @ P["q2_w"].T + P["q2_b"])
    idx = torch.argmax(c, 0).cpu()
    Bm = torch.softmax(Q @ Q[idx].T / np.sqrt(128.0), 0).T @ xt
    (torch.einsum("ock,ck->o", P["fcc_w"], Bm) + P["fcc_b"]).sum().backward()
    _check({"x": xg.grad}, {"x": xt.grad}, "two-module route")


# ---- unchanged paths -----------------------------------------------------------------------------------------------------
def test_call_without_row_gradients_is_backward_ex():
    """dsmil_agg_backward_rows with g_feats == NULL against dsmil_agg_backward_ex called directly (ops.agg_backward without
    want_g_feats IS that call): every parameter gradient bit-identical."""
    from dsmil_wsi_amd import _native, ops
    tag, N = "tcga", 3000
    K, C, nonlinear, _ = VARIANT[tag]
    L = _native.lib()
    pg = {k: v.cuda() for k, v in _params(tag).items()}
    xg = torch.from_numpy(make_bag(5, N, K)).cuda()
    _, _, A, B, idx = ops.agg_forward(xg, [N], pg, nonlinear=nonlinear)
    gp = torch.tensor([0.3, -0.7], device="cuda")
    gm = torch.tensor([0.2, 0.1], device="cuda")
    gc = torch.full((N, C), 0.01, device="cuda")
    ex = ops.agg_backward(xg, pg, A, B, idx, gp, g_classes=gc, g_max=gm, nonlinear=nonlinear)
    ex = {k: v.clone() for k, v in ex.items()}
    keep = [pg[k] for k in KEYS]
    P = _native.AggParams(*[t.data_ptr() for t in keep], K, K, C, 1)
    out = {k: torch.empty_like(v) for k, v in ex.items()}
    G = _native.AggGrads(*[out[k].data_ptr() for k in KEYS])
    nbytes = L.dsmil_agg_backward_rows_workspace_bytes(N, K, K, C)
    ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda").fill_(0xFF)
    ptr = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None
    rc = L.dsmil_agg_backward_rows(ptr(xg), ptr(xg), N, ctypes.byref(P), ptr(A), ptr(B), ptr(idx), ptr(gc), ptr(gm), ptr(gp),
                                   None, None, ctypes.byref(G), None, None, ptr(ws), nbytes,
                                   ctypes.c_void_p(torch.cuda.current_stream().cuda_stream), None)
    torch.cuda.synchronize()
    assert rc == 0
    for k in ex:
        assert torch.equal(out[k], ex[k]), k


def test_plain_backward_keeps_its_launches(monkeypatch):
    """A plain loss.backward() (rows that need no gradient) reports the parent's number of profiled launches, calls
    dsmil_agg_backward_ex (no row-gradient launch) and gives the gradients of ops.agg_backward without want_g_feats."""
    from dsmil_wsi_amd import _native, ops
    L = _native.lib()
    net = build_net("tcga", "cuda").train()
    x = torch.from_numpy(make_bag(7, 3000, 512)).cuda()
    y = torch.tensor([[1.0, 0.0]], device="cuda")
    _objective(net, x, y)[0].backward()   # warm-up
    torch.cuda.synchronize()
    wants = []
    ab = ops.agg_backward

    def agg_backward(*a, **k):
        wants.append(bool(k.get("want_g_feats")))
        return ab(*a, **k)
    monkeypatch.setattr(ops, "agg_backward", agg_backward)
    loss, _ = _objective(net, x, y)
    ms, n = ctypes.c_double(0), ctypes.c_int64(0)
    L.dsmil_profile_enable(1)
    try:
        L.dsmil_profile_collect(0, ctypes.byref(ms), ctypes.byref(n))   # reset
        loss.backward()
        torch.cuda.synchronize()
        L.dsmil_profile_collect(0, ctypes.byref(ms), ctypes.byref(n))
    finally:
        L.dsmil_profile_enable(0)
    print(f"attend-channel launches of a plain backward: {int(n.value)}")
    assert int(n.value) == PARENT_ATTEND_LAUNCHES_BACKWARD
    assert wants == [False]
