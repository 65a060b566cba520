"""The native value stream of BClassifier(passing_v=True) (dsmil.py:35-39,48: V = ReLU(Linear(K, K)(Dropout(feats))),
B = A^T V): ops.value_proj / ops.value_proj_backward (csrc/agg_value.h) and every module route through them, against the
fp64 oracle (oracle/agg_oracle.py) and fp64 autograd.  Needs a real MI355X.

Bars (the project's own, BASELINE.md section 4 / tests/test_agg_gpu.py::_cmp): classes / pred / B within 1e-4 abs + 1e-5 rel,
A within 1e-6 abs + 1e-3 rel; gradients err <= 2e-4 * max|ref| + 2e-5 (tests/test_agg_bwd_gpu.py).  Weights of widths
without a shipped set are drawn from a seeded torch.nn.init.orthogonal_ (as tests/golden/make_golden.py)."""
import numpy as np
import pytest
import torch

import agg_oracle as orc
from inputs import make_bag
from util import build_net

pytestmark = pytest.mark.gpu

# launches of the profiled attend channel (dsmil_profile_collect(0)) of the `tcga` net (v = Identity), recorded from the
# parent commit 189eecb on an MI355X: one net(x) of a 10 000-row bag / one forward_bags of the ragged batch below
PARENT_ATTEND_LAUNCHES_FORWARD = 1
PARENT_ATTEND_LAUNCHES_FORWARD_BAGS = 1
RAGGED = [1, 500, 37, 2000, 129, 128, 31, 33, 4097]


def _make_net(K, C, seed, dropout_v=0.0):
    """MILNet(FCLayer, BClassifier(passing_v=True)) with train_tcga.py:229-239 style weights (orthogonal, small random
    bias) and the same parameters as fp32 numpy arrays under the oracle's names."""
    from dsmil_wsi_amd import modules as M
    net = M.MILNet(M.FCLayer(in_size=K, out_size=C),
                   M.BClassifier(input_size=K, output_class=C, dropout_v=dropout_v, nonlinear=True, passing_v=True)).eval()
    g = torch.Generator().manual_seed(seed)
    for m in net.modules():
        if isinstance(m, (torch.nn.Linear, torch.nn.Conv1d)):
            torch.nn.init.orthogonal_(m.weight, generator=g)
            with torch.no_grad():
                m.bias.copy_(0.05 * torch.randn(m.bias.shape, generator=g))
    sd = {k: v.detach().numpy().copy() for k, v in net.state_dict().items()}
    p = {"fc_w": sd["i_classifier.fc.0.weight"], "fc_b": sd["i_classifier.fc.0.bias"],
         "q0_w": sd["b_classifier.q.0.weight"], "q0_b": sd["b_classifier.q.0.bias"],
         "q2_w": sd["b_classifier.q.2.weight"], "q2_b": sd["b_classifier.q.2.bias"],
         "v_w": sd["b_classifier.v.1.weight"], "v_b": sd["b_classifier.v.1.bias"],
         "fcc_w": sd["b_classifier.fcc.weight"], "fcc_b": sd["b_classifier.fcc.bias"]}
    return net.cuda(), p


def _cmp(out, ref_cls, ref_pred, ref_A, ref_B):
    classes, pred, A, B = [o.detach().cpu().numpy() for o in out]
    np.testing.assert_allclose(classes, ref_cls, atol=1e-4, rtol=1e-5)
    np.testing.assert_allclose(pred, ref_pred, atol=1e-4, rtol=1e-5)
    np.testing.assert_allclose(A, ref_A, atol=1e-6, rtol=1e-3)
    np.testing.assert_allclose(B, ref_B, atol=1e-4, rtol=1e-5)


def _v_ref(x, p):
    return orc.value_proj(np.asarray(x, np.float64), {"v_w": p["v_w"].astype(np.float64), "v_b": p["v_b"].astype(np.float64)}, True)


# ---- T1: the projection alone ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,N", [(64, 50), (166, 333), (256, 129), (512, 1), (512, 31), (512, 10000), (1024, 300), (512, 70000)])
def test_value_proj_vs_oracle(K, N):
    from dsmil_wsi_amd import ops
    _, p = _make_net(K, 2, 300 + K)
    x = make_bag(900 + N, N, K)
    V = ops.value_proj(torch.from_numpy(x).cuda(), torch.from_numpy(p["v_w"]).cuda(), torch.from_numpy(p["v_b"]).cuda())
    ref = _v_ref(x, p)
    got = V.cpu().numpy()
    print(f"value_proj K={K} N={N}: max err {np.abs(got - ref).max():.3e}  max |V| {np.abs(ref).max():.3e}")
    assert got.shape == (N, K) and got.dtype == np.float32
    np.testing.assert_allclose(got, ref, atol=1e-4, rtol=1e-5)


def test_value_proj_row_map_subset():
    from dsmil_wsi_amd import ops
    K, rows = 512, 3000
    _, p = _make_net(K, 2, 300 + K)
    x = make_bag(4711, rows, K)
    sel = np.sort(np.random.default_rng(5).permutation(rows)[:1777]).astype(np.int64)
    sel = np.random.default_rng(6).permutation(sel)   # a random subset in random order (train_tcga.py:78-83)
    V = ops.value_proj(torch.from_numpy(x).cuda(), torch.from_numpy(p["v_w"]).cuda(), torch.from_numpy(p["v_b"]).cuda(),
                       row_map=torch.from_numpy(sel).cuda())
    ref = _v_ref(x[sel], p)
    print(f"value_proj row_map: max err {np.abs(V.cpu().numpy() - ref).max():.3e}")
    assert tuple(V.shape) == (len(sel), K)
    np.testing.assert_allclose(V.cpu().numpy(), ref, atol=1e-4, rtol=1e-5)


@pytest.mark.parametrize("scale", [1e-3, 1.0, 300.0])
def test_value_proj_row_scales(scale):
    """Bags on very different scales (as test_batch_form_f2_vs_oracle_and_six_product_form): the per-row power-of-two scale keeps
    the fp16 planes in range; the bar scales with the rows: V is linear in its row up to the bias, a row of N(0, 1) values
    (max |x| near 4) has the plain bar, a row s times larger s times the bar (never less than the plain bar).  One bag mixes
    rows four decades apart."""
    from dsmil_wsi_amd import ops
    K, N = 512, 1000
    _, p = _make_net(K, 2, 300 + K)
    x = make_bag(77, N, K, scale=scale)
    x[::7] *= np.float32(1e-2)
    x[3::11] *= np.float32(1e2)
    V = ops.value_proj(torch.from_numpy(x).cuda(), torch.from_numpy(p["v_w"]).cuda(), torch.from_numpy(p["v_b"]).cuda())
    ref = _v_ref(x, p)
    row_sc = np.maximum(1.0, np.abs(x).max(axis=1, keepdims=True).astype(np.float64) / 4.0)   # rows of N(0,1) peak near 4
    err = np.abs(V.cpu().numpy() - ref)
    print(f"value_proj scale={scale:g}: max err / row scale {(err / row_sc).max():.3e}")
    assert np.all(err <= 1e-4 * row_sc + 1e-5 * np.abs(ref))


# ---- T2: the module forward --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,C,N", [(512, 1, 10000), (512, 2, 10000), (512, 5, 10000), (1024, 2, 300)])
def test_milnet_passing_v_vs_oracle(K, C, N):
    net, p = _make_net(K, C, 40 + K + C)
    x = make_bag(4242 + N + C, N, K)
    ref = orc.milnet_forward(x, p, passing_v=True, dtype="f64")
    with torch.no_grad():
        out = net(torch.from_numpy(x).cuda())
    idx = np.argmax(out[0].cpu().numpy(), axis=0)
    assert np.array_equal(idx, ref[4])
    for name, o, r in zip(("classes", "pred", "A", "B"), out, ref):
        print(f"passing_v K={K} C={C} N={N} {name}: max err {np.abs(o.cpu().numpy() - r).max():.3e}")
    _cmp(out, ref[0], ref[1], ref[2], ref[3])


# ---- T3: routes ----------------------------------------------------------------------------------------------------------
def _weights(net):
    bc, lin = net.b_classifier, net.i_classifier.fc[0]
    w = {k: (v.detach() if v is not None else None) for k, v in bc._weights().items()}
    w["fc_w"], w["fc_b"] = lin.weight.detach(), lin.bias.detach()
    return w, bc.v[1].weight.detach(), bc.v[1].bias.detach()


def test_module_route_is_the_native_projection():
    """B and pred of the module are BIT-identical to the explicit native sequence: a torch GEMM would not give these bits."""
    from dsmil_wsi_amd import ops
    N, K = 3000, 512
    net, _ = _make_net(K, 2, 11)
    x = torch.from_numpy(make_bag(31, N, K)).cuda()
    w, v_w, v_b = _weights(net)
    with torch.no_grad():
        out = net(x)
        bout = net.b_classifier(x, out[0])
    exp = ops.agg_forward(x, [N], w, vals=ops.value_proj(x, v_w, v_b))
    assert torch.equal(out[3], exp[3]) and torch.equal(out[1], exp[1]) and torch.equal(out[2], exp[2])
    exp_c = ops.agg_forward(x, [N], w, classes_in=out[0], vals=ops.value_proj(x, v_w, v_b))
    assert torch.equal(bout[2], exp_c[3]) and torch.equal(bout[0], exp_c[1])   # BClassifier.forward alone, caller's c
    # and under autograd (training mode, dropout_v = 0): the same bits
    out_t = net.train()(x)
    assert torch.equal(out_t[3].detach(), exp[3]) and torch.equal(out_t[1].detach(), exp[1])


def test_forward_bags_passing_v():
    net, p = _make_net(512, 2, 12)
    bags = [torch.from_numpy(make_bag(900 + i, n, 512)).cuda() for i, n in enumerate(RAGGED)]
    outs = net.forward_bags(bags)
    assert len(outs) == len(bags)
    for b, o in zip(bags, outs):
        ref = orc.milnet_forward(b.cpu().numpy(), p, passing_v=True, dtype="f64")
        _cmp(o, ref[0], ref[1], ref[2], ref[3])
        with torch.no_grad():
            single = net(b)
        for u, v in zip(o, single):
            np.testing.assert_allclose(u.cpu().numpy(), v.cpu().numpy(), atol=2e-5, rtol=1e-4)
    # the tuple form (feats, lengths) is the same call
    outs2 = net.forward_bags((torch.cat(bags), RAGGED))
    for o, o2 in zip(outs, outs2):
        assert all(torch.equal(u, v) for u, v in zip(o, o2))


def test_graphed_passing_v():
    N, K = 2000, 512
    net, _ = _make_net(K, 2, 13)
    x = torch.from_numpy(make_bag(32, N, K)).cuda()
    with torch.no_grad():
        exp = [t.clone() for t in net(x)]
    run = net.graphed(N)
    for _ in range(2):
        got = run(x)
        torch.cuda.synchronize()
        for u, v in zip(got, exp):
            assert torch.equal(u, v)
    got = run(x * 0.5)   # another bag through the same graph
    with torch.no_grad():
        exp2 = net(x * 0.5)
    for u, v in zip(got, exp2):
        assert torch.equal(u, v)


class _Stop(Exception):
    pass


def _play_ranks(fn, R):
    """Run ``fn(rank, gather)`` for R ranks inside ONE process: the function has two all-gather points; pass p records every
    rank's message of exchange p (and stops there), the last pass replays all."""
    msgs = []
    for phase in range(3):
        new, outs = [], []
        for r in range(R):
            k = {"i": 0}

            def gather(t, group=None, _k=k):
                i = _k["i"]
                _k["i"] += 1
                if i < len(msgs):
                    return msgs[i]
                new.append(t.clone())
                raise _Stop
            try:
                outs.append(fn(r, gather))
            except _Stop:
                pass
        if phase < 2:
            assert len(new) == R
            msgs.append(new)
    assert len(outs) == R
    return outs


def test_instance_sharded_bag_passing_v():
    from dsmil_wsi_amd import dist as dd
    N, K, R = 10000, 512, 3
    net, p = _make_net(K, 2, 14)
    x = torch.from_numpy(make_bag(555 + N, N, K)).cuda()
    shards = [dd.shard_range(N, r, R) for r in range(R)]
    outs = _play_ranks(lambda r, g: dd.sharded_bag_forward(net, x[shards[r][0]:shards[r][1]], shards[r][0], gather=g), R)
    with torch.no_grad():
        full = net(x)
    ref = orc.milnet_forward(x.cpu().numpy(), p, passing_v=True, dtype="f64")
    classes = torch.cat([o[0] for o in outs])
    A = torch.cat([o[2] for o in outs])
    for o in outs:
        assert np.array_equal(o[4].cpu().numpy(), np.asarray(ref[4]))
        np.testing.assert_allclose(o[1].cpu().numpy(), full[1].cpu().numpy(), atol=2e-6)
        np.testing.assert_allclose(o[3].cpu().numpy(), full[3].cpu().numpy(), atol=2e-6)
    _cmp((classes, outs[0][1], A, outs[0][3]), ref[0], ref[1], ref[2], ref[3])


# ---- T4: backward ----------------------------------------------------------------------------------------------------------
def _autograd_f64(x, p, idx, mask, y):
    """fp64 restatement (CPU) of the training objective of train_tcga.py:67-71 through FCLayer + BClassifier(passing_v) given
    the critical indices and the ReLU mask of the value layer."""
    x = torch.from_numpy(x).double()
    P = {k: torch.from_numpy(v).double().requires_grad_(True) for k, v in p.items()}
    c = x @ P["fc_w"].T + P["fc_b"]
    h = x @ P["q0_w"].T + P["q0_b"]
    Q = torch.tanh(torch.relu(h) @ P["q2_w"].T + P["q2_b"])
    V = (x @ P["v_w"].T + P["v_b"]) * mask
    A = torch.softmax(Q @ Q[idx].T / np.sqrt(128.0), 0)
    B = A.T @ V
    pred = torch.einsum("ock,ck->o", P["fcc_w"], B) + P["fcc_b"]
    mx = c[idx, torch.arange(c.shape[1])]
    crit = torch.nn.BCEWithLogitsLoss()
    loss = 0.5 * crit(pred.view(1, -1), y.view(1, -1)) + 0.5 * crit(mx.view(1, -1), y.view(1, -1))
    loss.backward()
    return {k: v.grad.numpy() for k, v in P.items()}


NAMES = {"i_classifier.fc.0.weight": "fc_w", "i_classifier.fc.0.bias": "fc_b", "b_classifier.q.0.weight": "q0_w",
         "b_classifier.q.0.bias": "q0_b", "b_classifier.q.2.weight": "q2_w", "b_classifier.q.2.bias": "q2_b",
         "b_classifier.v.1.weight": "v_w", "b_classifier.v.1.bias": "v_b", "b_classifier.fcc.weight": "fcc_w",
         "b_classifier.fcc.bias": "fcc_b"}


@pytest.mark.parametrize("K,N", [(64, 50), (512, 700), (166, 333), (1024, 300)])
def test_backward_passing_v_vs_fp64_autograd(K, N):
    """loss.backward() through the module (value layer's dropout inactive): every parameter gradient, v.1.weight and v.1.bias
    included, against fp64 autograd; two runs bit-identical.  The ReLU makes the comparison ill-conditioned where a
    pre-activation is near zero (one mask flip moves a row of g_Wv by percents), so the reference takes its mask from the
    device's V; the mask itself must equal the oracle's wherever |z_ref| > 1e-4 (the forward bar), and at most 1e-3 of the
    entries may lie inside that band (else the case is inconclusive and fails)."""
    from dsmil_wsi_amd import ops
    C = 2
    net, p = _make_net(K, C, 50 + K)
    net.train()
    x = make_bag(900 + N, N, K)
    xg = torch.from_numpy(x).cuda()
    y = torch.tensor([[1.0, 0.0]], device="cuda")
    crit = torch.nn.BCEWithLogitsLoss()
    grads = []
    for _ in range(2):
        net.zero_grad(set_to_none=True)
        ins, bag, _, _ = net(xg)
        mx, _ = torch.max(ins, 0)
        loss = 0.5 * crit(bag.view(1, -1), y) + 0.5 * crit(mx.view(1, -1), y)
        loss.backward()
        grads.append({NAMES[k]: prm.grad.clone() for k, prm in net.named_parameters()})
    for k in grads[0]:
        assert torch.equal(grads[0][k], grads[1][k]), f"{k}: two runs differ"
    with torch.no_grad():
        w, v_w, v_b = _weights(net)
        V = ops.value_proj(xg, v_w, v_b).cpu().numpy()
        idx = torch.argmax(ins.detach(), 0).cpu()
    z_ref = x.astype(np.float64) @ p["v_w"].astype(np.float64).T + p["v_b"].astype(np.float64)
    mask = V > 0
    clear = np.abs(z_ref) > 1e-4
    share = 1.0 - clear.mean()
    print(f"K={K} N={N}: share of |z_ref| <= 1e-4: {share:.2e}; mask flips outside the band: {int((mask != (z_ref > 0))[clear].sum())}")
    assert share <= 1e-3, f"inconclusive: {share:.2e} of the pre-activations lie within the forward bar of zero"
    assert np.array_equal(mask[clear], (z_ref > 0)[clear])
    ref = _autograd_f64(x, p, idx, torch.from_numpy(mask).double(), y.cpu().double())
    for k, r in ref.items():
        scale = max(float(np.abs(r).max()), 1e-12)
        err = float(np.abs(grads[0][k].cpu().numpy().astype(np.float64) - r).max())
        print(f"K={K} N={N} g_{k}: max err {err:.3e} vs scale {scale:.3e}")
        assert err <= 2e-4 * scale + 2e-5, f"K={K} N={N} {k}: max err {err:.3e} vs scale {scale:.3e}"


def test_value_proj_backward_row_map():
    from dsmil_wsi_amd import ops
    K, rows = 256, 900
    _, p = _make_net(K, 2, 300 + K)
    x = make_bag(99, rows, K)
    sel = np.random.default_rng(8).permutation(rows)[:500].astype(np.int64)
    xg, mg = torch.from_numpy(x).cuda(), torch.from_numpy(sel).cuda()
    V = ops.value_proj(xg, torch.from_numpy(p["v_w"]).cuda(), torch.from_numpy(p["v_b"]).cuda(), row_map=mg)
    g = torch.from_numpy(np.random.default_rng(9).standard_normal((500, K)).astype(np.float32)).cuda()
    gw, gb = ops.value_proj_backward(xg, V, g, row_map=mg)
    gz = g.double().cpu() * (V.cpu() > 0)
    rw, rb = (gz.T @ torch.from_numpy(x[sel]).double()).numpy(), gz.sum(0).numpy()
    for name, got, r in (("g_v_w", gw, rw), ("g_v_b", gb, rb)):
        err, scale = float(np.abs(got.cpu().numpy() - r).max()), float(np.abs(r).max())
        print(f"{name}: max err {err:.3e} vs scale {scale:.3e}")
        assert err <= 2e-4 * scale + 2e-5


# ---- T5: v = Identity is untouched -------------------------------------------------------------------------------------------
def test_identity_models_keep_their_launch_sequence():
    from dsmil_wsi_amd import _native
    import ctypes
    L = _native.lib()
    net = build_net("tcga", "cuda")
    x = torch.from_numpy(make_bag(1, 10000, 512)).cuda()
    bags = [torch.from_numpy(make_bag(900 + i, n, 512)).cuda() for i, n in enumerate(RAGGED)]
    with torch.no_grad():
        net(x), net.forward_bags(bags)   # warm-up: packed weights, workspace
    torch.cuda.synchronize()

    def count(fn):
        ms, n = ctypes.c_double(0), ctypes.c_int64(0)
        L.dsmil_profile_enable(1)
        try:
            L.dsmil_profile_collect(0, ctypes.byref(ms), ctypes.byref(n))   # reset
            with torch.no_grad():
                fn()
            L.dsmil_profile_collect(0, ctypes.byref(ms), ctypes.byref(n))
        finally:
            L.dsmil_profile_enable(0)
        return int(n.value)
    n_fwd, n_bags = count(lambda: net(x)), count(lambda: net.forward_bags(bags))
    print(f"attend launches: forward {n_fwd}, forward_bags {n_bags}")
    assert n_fwd == PARENT_ATTEND_LAUNCHES_FORWARD
    assert n_bags == PARENT_ATTEND_LAUNCHES_FORWARD_BAGS


# ---- T6: dropout ---------------------------------------------------------------------------------------------------------------
def test_dropout_of_the_value_layer():
    N, K = 1000, 512
    x = torch.from_numpy(make_bag(33, N, K)).cuda()
    net, _ = _make_net(K, 2, 15, dropout_v=0.5)
    with torch.no_grad():
        ev = net.eval()(x)
        tr = net.train()(x)
    assert all(bool(torch.isfinite(t).all()) for t in tr)
    assert torch.equal(ev[0], tr[0]) and torch.equal(ev[2], tr[2])   # classes and A do not see the value layer
    assert not torch.equal(ev[3], tr[3]) and float((ev[3] - tr[3]).abs().max()) > 1e-4
    net0, _ = _make_net(K, 2, 15, dropout_v=0.0)
    with torch.no_grad():
        ev0 = net0.eval()(x)
        tr0 = net0.train()(x)
    for u, v in zip(ev0, tr0):
        assert torch.equal(u, v)
    assert torch.equal(ev0[3], ev[3])   # the same weights: eval does not depend on p
