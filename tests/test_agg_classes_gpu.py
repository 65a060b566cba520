"""The aggregator's routes at C > 2 classes (dsmil.py:43 "can handle multiple class"; train_tcga.py --num_classes) against
the fp64 oracle (oracle/agg_oracle.py) and the reference's own vectors (tests/golden/agg_golden_classes.npz).  Needs a real
MI355X.

The kernels at C > 2 are separate code from the C <= 2 fast kernels: class-pair loops (the last pair of an odd C runs with
c1 == c0), per-class hand-off flags, per-class partial slots.  Every measured call here runs on a NaN-poisoned workspace
(a warm-up call of the same sizes first, then every workspace word = 0xFFFFFFFF): a slot the call reads but did not write
shows up as a NaN instead of as whatever an earlier call left there.

Bars: fp32 — those of tests/test_agg_gpu.py through the tie-safe per-bag check (util.check_bag: logits, B and pred within
1e-4 of max(1, |ref|max), A within 1e-6 + 1e-3 rel, sum A = 1 within 1e-5; a critical instance that differs from the
oracle's must be a near-tie of the fp32 logits); bf16 storage — those of tests/test_agg_bf16_gpu.py::_check against the
oracle fed the bf16-rounded inputs and weights; gradients — those of tests/test_agg_bwd_gpu.py (2e-4 of each gradient's
max-abs + 2e-5)."""
import numpy as np
import pytest
import torch

import agg_oracle as orc
from inputs import make_bag, make_label
from test_agg_bwd_gpu import _autograd_f64
from test_agg_gpu import _play_ranks
from util import GOLDEN_CLASSES, check_bag, class_set_weights, poison_workspace, state_dict_from_npz

pytestmark = pytest.mark.gpu

KEYS = ("fc_w", "fc_b", "q0_w", "q0_b", "q2_w", "q2_b", "fcc_w", "fcc_b")


def _weights(K, C, seed, nonlinear=True, Kv=None):
    """A seeded weight set at the scales of test_agg_bf16_gpu.py::test_bf16_resident_tile_kernel (fcc over Kv)."""
    rng = np.random.default_rng(seed)
    Kv = K if Kv is None else Kv
    p = {"fc_w": rng.standard_normal((C, K), dtype=np.float32) * 0.05, "fc_b": rng.standard_normal(C, dtype=np.float32) * 0.1,
         "q0_w": rng.standard_normal((128, K), dtype=np.float32) * np.float32(1.0 / np.sqrt(K)),
         "q0_b": rng.standard_normal(128, dtype=np.float32) * 0.1,
         "q2_w": rng.standard_normal((128, 128), dtype=np.float32) * np.float32(1.0 / np.sqrt(128)),
         "q2_b": rng.standard_normal(128, dtype=np.float32) * 0.1,
         "fcc_w": rng.standard_normal((C, C, Kv), dtype=np.float32) * 0.05, "fcc_b": rng.standard_normal(C, dtype=np.float32) * 0.1}
    if not nonlinear:
        del p["q2_w"], p["q2_b"]
    return p


def _dev(w):
    return {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in w.items()}


def _net(w, K, C, nonlinear=True):
    from dsmil_wsi_amd import modules as M
    net = M.MILNet(M.FCLayer(in_size=K, out_size=C),
                   M.BClassifier(input_size=K, output_class=C, dropout_v=0.0, nonlinear=nonlinear))
    net.load_state_dict(state_dict_from_npz(w, nonlinear), strict=True)
    return net.eval().cuda()


def _poisoned(fn):
    """fn() once to size this stream's workspace, then again on a NaN-poisoned workspace; returns the second result."""
    from dsmil_wsi_amd import ops
    fn()
    poison_workspace(ops)
    out = fn()
    torch.cuda.synchronize()
    return out


def _fwd(x, lengths, p, **kw):
    from dsmil_wsi_amd import ops
    return _poisoned(lambda: [t.clone() for t in ops.agg_forward(x, lengths, p, **kw)])


def _worst():
    return {"classes": 0.0, "A": 0.0, "B": 0.0, "pred": 0.0}


def _check_bags(got, bags, w, which, tag, nonlinear=True, refs=None):
    """check_bag for the bags `which` of a batch output; returns the oracle outputs (for reuse across launch forms)."""
    off = np.concatenate([[0], np.cumsum([b.shape[0] for b in bags])])
    refs = refs if refs is not None else {}
    worst = _worst()
    for b in which:
        if b not in refs:
            refs[b] = orc.milnet_forward(bags[b], w, nonlinear=nonlinear, dtype="f64")
        check_bag(got, b, slice(int(off[b]), int(off[b + 1])), refs[b], worst, f"{tag} bag {b} ({bags[b].shape[0]} rows)")
        assert torch.isfinite(got[1][b]).all() and torch.isfinite(got[3][b]).all(), f"{tag} bag {b}: non-finite output"
    print(tag, {k: float("%.3g" % v) for k, v in worst.items()})
    return refs


# ---- the reference's own vectors at C > 2 ----------------------------------------------------------------------------------
GOLDEN_FWD = [("K64_C5_nl", 64, 5, True, 200), ("K166_C4_nl", 166, 4, True, 57), ("K512_C5_nl", 512, 5, True, 300),
              ("K64_C17_nl", 64, 17, True, 120), ("K64_C6_lin", 64, 6, False, 80)]


@pytest.mark.parametrize("ws,K,C,nonlinear,N", GOLDEN_FWD)
def test_forward_vs_reference_golden_many_classes(ws, K, C, nonlinear, N):
    z = np.load(GOLDEN_CLASSES)
    name = f"{ws}/fwd_N{N}"
    w = class_set_weights(z, ws)
    net = _net(w, K, C, nonlinear)
    x = torch.from_numpy(make_bag(int(z[f"{name}/seed"]), N, K)).cuda()
    with torch.no_grad():
        out = _poisoned(lambda: [t.clone() for t in net(x)])
    ref = tuple(z[f"{name}/{k}"] for k in ("classes", "pred", "A", "B", "idx"))
    idx = torch.from_numpy(np.argmax(out[0].cpu().numpy(), axis=0)[None])
    check_bag((out[0], out[1], out[2], out[3], idx), 0, slice(0, N), ref, _worst(), name)


# ---- lone bags: k_attend_hs (K % 4 == 0) and k_query_attend_split<1, 1, 6> (K = 166) -------------------------------------
@pytest.mark.parametrize("C", [3, 4, 5, 8, 17, 64])
@pytest.mark.parametrize("N", [1, 37, 10000])
def test_lone_bag_with_and_without_inline_query(C, N):
    """k_attend_hs with the critical query handed over inside the launch (one flag per class) and with k_qmax between the
    logits pass and the attend kernel (dsmil_agg_inline_query(0)): both against the oracle, and bit-identical."""
    from dsmil_wsi_amd import _native
    L = _native.lib()
    K = 512
    w = _weights(K, C, 300 + C)
    p = _dev(w)
    xh = make_bag(7000 + C + N, N, K)
    x = torch.from_numpy(xh).cuda()
    outs = []
    prev = L.dsmil_agg_inline_query(1)
    try:
        outs.append(_fwd(x, [N], p))
        L.dsmil_agg_inline_query(0)
        outs.append(_fwd(x, [N], p))
    finally:
        L.dsmil_agg_inline_query(prev if prev in (0, 1) else 1)
    refs = _check_bags(outs[0], [xh], w, [0], f"hs inline C {C} N {N}")
    _check_bags(outs[1], [xh], w, [0], f"hs k_qmax C {C} N {N}", refs=refs)
    for a, b in zip(*outs):
        assert torch.equal(a, b)


@pytest.mark.parametrize("N", [37, 10000])
def test_lone_bag_unaligned_width(N):
    """K = 166: rows are not 16-B aligned, the register-staged k_query_attend_split<1, 1, 6> runs; odd C = 5."""
    K, C = 166, 5
    w = _weights(K, C, 166)
    xh = make_bag(7100 + N, N, K)
    got = _fwd(torch.from_numpy(xh).cuda(), [N], _dev(w))
    _check_bags(got, [xh], w, [0], f"K 166 C 5 N {N}")


# ---- fp32 batches in the 128-row regime: k_attend_f2 (form 1 and 2 at C > 2), k_query_attend_split (form 0) ---------------
BATCH = [9000, 1, 9000, 33, 12000, 9000, 9000, 9000, 9000, 255]
BATCH_CHECK = [0, 1, 3, 4, 9]


@pytest.mark.parametrize("nonlinear", [True, False])
@pytest.mark.parametrize("C", [3, 4, 17])
@pytest.mark.parametrize("K", [128, 512])
def test_batch_forms_vs_oracle(K, C, nonlinear):
    """A ragged batch in the 128-row regime under dsmil_agg_batch_form 0, 1 and 2 (k_attend_f3 requires C <= 2, so forms 1 and
    2 both run k_attend_f2 here): every form against the oracle, never only against another form."""
    from dsmil_wsi_amd import _native
    L = _native.lib()
    assert L.dsmil_agg_tile_rows(len(BATCH), sum(BATCH)) == 128
    w = _weights(K, C, 400 + K + C, nonlinear)
    p = _dev(w)
    bags = [make_bag(7200 + K + C + i, n, K) for i, n in enumerate(BATCH)]
    x = torch.from_numpy(np.concatenate(bags)).cuda()
    refs = {}
    prev = L.dsmil_agg_batch_form(2)
    try:
        for form in (0, 1, 2):
            L.dsmil_agg_batch_form(form)
            got = _fwd(x, BATCH, p, nonlinear=nonlinear)
            refs = _check_bags(got, bags, w, BATCH_CHECK, f"form {form} K {K} C {C} nl {nonlinear}", nonlinear, refs)
    finally:
        L.dsmil_agg_batch_form(prev)


def test_batch_with_value_rows_and_with_caller_logits():
    """K = 256, C = 5 in the 128-row regime: `vals != feats` (passing_v: the value rows are another matrix) and caller-supplied
    instance logits (attention_map.py's separate b_classifier call)."""
    from dsmil_wsi_amd import _native
    L = _native.lib()
    K, C = 256, 5
    assert L.dsmil_agg_tile_rows(len(BATCH), sum(BATCH)) == 128
    rng = np.random.default_rng(256)
    w = _weights(K, C, 256)
    w["v_w"] = rng.standard_normal((K, K), dtype=np.float32) * np.float32(1.0 / np.sqrt(K))
    w["v_b"] = rng.standard_normal(K, dtype=np.float32) * 0.1
    p = _dev({k: v for k, v in w.items() if not k.startswith("v_")})
    bags = [make_bag(7300 + i, n, K) for i, n in enumerate(BATCH)]
    xh = np.concatenate(bags)
    vh = np.maximum(xh @ w["v_w"].T + w["v_b"], 0).astype(np.float32)
    x, v = torch.from_numpy(xh).cuda(), torch.from_numpy(vh).cuda()
    got = _fwd(x, BATCH, p, vals=v)
    off = np.concatenate([[0], np.cumsum(BATCH)])
    worst = _worst()
    for b in BATCH_CHECK:
        sl = slice(int(off[b]), int(off[b + 1]))
        cls = orc.instance_logits(bags[b].astype(np.float64), w["fc_w"].astype(np.float64), w["fc_b"].astype(np.float64))
        pred, A, B, idx = orc.bclassifier_forward(bags[b], cls, w, passing_v=True, dtype="f64")
        check_bag(got, b, sl, (cls, pred, A, B, idx), worst, f"passing_v bag {b}")
    print("passing_v", worst)
    # caller-supplied logits that are NOT the FC output: a random matrix moves every critical instance
    cin = torch.from_numpy(rng.standard_normal((sum(BATCH), C), dtype=np.float32)).cuda()
    got = _fwd(x, BATCH, p, classes_in=cin)
    worst = _worst()
    for b in BATCH_CHECK:
        sl = slice(int(off[b]), int(off[b + 1]))
        cls = cin[sl].cpu().numpy()
        pred, A, B, idx = orc.bclassifier_forward(bags[b], cls, w, dtype="f64")
        check_bag(got, b, sl, (cls, pred, A, B, idx), worst, f"classes_in bag {b}")
    print("classes_in", worst)


# ---- k_finish: workgroups of the grid (sized for the longest bag) that own nothing of a short bag ---------------------------
@pytest.mark.parametrize("C", [17, 33])
@pytest.mark.parametrize("Kv", [64, 512])
def test_finish_blocks_without_rows_or_k_run(Kv, C):
    """finish_blocks(max_rows, Kv) > ceil(Kv / 64) (one bag of more than 32 Kv rows): the short bags' workgroups past their
    rows and past the k-runs own no part of that bag and must still zero their C x C bag-head partials — all of them, not the
    first 256.  Every bag's pred against the oracle."""
    K = Kv
    long_rows = 32 * Kv + 3000
    lengths = [long_rows, 1, 100, 255]
    w = _weights(K, C, 500 + Kv + C)
    bags = [make_bag(7400 + Kv + C + i, n, K) for i, n in enumerate(lengths)]
    got = _fwd(torch.from_numpy(np.concatenate(bags)).cuda(), lengths, _dev(w))
    _check_bags(got, bags, w, range(len(lengths)), f"k_finish Kv {Kv} C {C}")


def test_finish_blocks_with_rows_but_no_k_run_many_classes():
    """C = 300 > 256 threads, K = 64 (one k-run), a bag of 5 000 rows (three finish workgroups): workgroups 1 and 2 own rows but
    no k-run and must zero their partials of all 300 output classes."""
    K, C, N = 64, 300, 5000
    w = _weights(K, C, 300300)
    xh = make_bag(7500, N, K)
    got = _fwd(torch.from_numpy(xh).cuda(), [N], _dev(w))
    _check_bags(got, [xh], w, [0], "k_finish C 300")


# ---- bf16 storage -----------------------------------------------------------------------------------------------------------
def _round_bf16(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(torch.bfloat16).to(torch.float32).numpy()


def _check_bf16(got, b, sl, ref, tag):
    """tests/test_agg_bf16_gpu.py::_check for one bag of a batch, with the tie-safe critical index of util.check_bag."""
    cls, pred, A, B = [o.float().cpu().numpy() for o in (got[0][sl], got[1][b:b + 1], got[2][sl], got[3][b:b + 1])]
    np.testing.assert_allclose(cls, ref[0], atol=1e-4, rtol=1e-5, err_msg=f"{tag}: logits")
    idx = got[4][b].cpu().numpy()
    if not np.array_equal(idx, ref[4]):
        gap = ref[0].max(axis=0) - ref[0][idx, np.arange(cls.shape[1])]
        assert np.all(gap <= 4e-6 * max(1.0, float(np.abs(ref[0]).max()))), f"{tag}: critical instance {idx} vs {ref[4]}"
        return
    np.testing.assert_allclose(A, ref[2], atol=1e-6, rtol=3e-2, err_msg=f"{tag}: A")
    np.testing.assert_allclose(B.reshape(ref[3].shape), ref[3], atol=2e-3, rtol=2e-2, err_msg=f"{tag}: B")
    np.testing.assert_allclose(pred, ref[1], atol=2e-3, rtol=2e-2, err_msg=f"{tag}: pred")
    np.testing.assert_allclose(A.sum(axis=0, dtype=np.float64), 1.0, atol=1e-4, err_msg=f"{tag}: sum A")


@pytest.mark.parametrize("C", [3, 5, 17])
@pytest.mark.parametrize("K", [256, 512])
def test_bf16_batch_and_lone_bag(K, C):
    """bf16 features: a batch in the 128-row regime (k_query_attend_bf16_dma: k_attend_bf16_res requires C <= 2; logits
    k_logits_stream<2, bf16> over class pairs) and a lone bag (k_query_attend_bf16<1>)."""
    from dsmil_wsi_amd import _native
    L = _native.lib()
    assert L.dsmil_agg_tile_rows(len(BATCH), sum(BATCH)) == 128
    w = _weights(K, C, 600 + K + C)
    wr = {k: _round_bf16(v) for k, v in w.items()}
    bags = [make_bag(7600 + K + C + i, n, K) for i, n in enumerate(BATCH)]
    x = torch.from_numpy(np.concatenate(bags)).cuda().to(torch.bfloat16)
    got = _fwd(x, BATCH, _dev(w))
    off = np.concatenate([[0], np.cumsum(BATCH)])
    for b in BATCH_CHECK:
        ref = orc.milnet_forward(_round_bf16(bags[b]), wr, dtype="f64")
        _check_bf16(got, b, slice(int(off[b]), int(off[b + 1])), ref, f"bf16 batch K {K} C {C} bag {b}")
    N = 3000
    xl = make_bag(7650 + K + C, N, K)
    got = _fwd(torch.from_numpy(xl).cuda().to(torch.bfloat16), [N], _dev(w))
    _check_bf16(got, 0, slice(0, N), orc.milnet_forward(_round_bf16(xl), wr, dtype="f64"), f"bf16 lone bag K {K} C {C}")


def test_bf16_module_forward_bags_many_classes():
    """module.bfloat16() + bf16 bags through MILNet.forward_bags at C = 5."""
    K, C = 512, 5
    w = _weights(K, C, 605)
    wr = {k: _round_bf16(v) for k, v in w.items()}
    net = _net(w, K, C).to(torch.bfloat16)
    bags = [make_bag(7700 + i, n, K) for i, n in enumerate(BATCH)]
    xb = [torch.from_numpy(b).cuda().to(torch.bfloat16) for b in bags]
    outs = _poisoned(lambda: [[t.clone() for t in o] for o in net.forward_bags(xb)])
    for b in BATCH_CHECK:
        o = outs[b]
        assert o[1].shape == (1, C)
        idx = torch.from_numpy(np.argmax(o[0].float().cpu().numpy(), axis=0)[None])
        ref = orc.milnet_forward(_round_bf16(bags[b]), wr, dtype="f64")
        _check_bf16((o[0], o[1], o[2], o[3], idx), 0, slice(0, bags[b].shape[0]), ref, f"bf16 module bag {b}")


# ---- row map, instance-sharded bag -----------------------------------------------------------------------------------------
def test_row_map_many_classes():
    """dropout_patches as an index list at C = 5: the batch through a row map against the oracle on the gathered rows."""
    from dsmil_wsi_amd import _native
    L = _native.lib()
    K, C = 256, 5
    rng = np.random.default_rng(5)
    w = _weights(K, C, 705)
    lengths = [9000] * 8
    assert L.dsmil_agg_tile_rows(len(lengths), sum(lengths)) == 128
    phys = make_bag(7800, 80000, K)
    rmap = rng.permutation(80000)[:sum(lengths)].astype(np.int64)
    got = _fwd(torch.from_numpy(phys).cuda(), lengths, _dev(w), row_map=torch.from_numpy(rmap).cuda())
    bags = [phys[rmap[9000 * b:9000 * (b + 1)]] for b in range(len(lengths))]
    _check_bags(got, bags, w, [0, 3, 7], "row_map C 5")


@pytest.mark.parametrize("C", [5, 17])
def test_instance_sharded_bag_many_classes(C):
    """dsmil_agg_shard_argmax / dsmil_agg_shard_attend with R = 3 ranks played in one process: against the oracle and the
    unsharded forward."""
    from dsmil_wsi_amd import dist as dd, ops
    K, N, R = 512, 10000, 3
    w = _weights(K, C, 800 + C)
    net = _net(w, K, C)
    xh = make_bag(7900 + C, N, K)
    x = torch.from_numpy(xh).cuda()
    shards = [dd.shard_range(N, r, R) for r in range(R)]
    def rank(r, g):   # every rank's call sequence starts on a poisoned workspace (the first pass of _play_ranks sizes it)
        poison_workspace(ops)
        return dd.sharded_bag_forward(net, x[shards[r][0]:shards[r][1]], shards[r][0], gather=g)
    outs = _play_ranks(rank, R)
    torch.cuda.synchronize()
    with torch.no_grad():
        full = net(x)
    for o in outs:
        np.testing.assert_allclose(o[1].cpu().numpy(), full[1].cpu().numpy(), atol=2e-6)
        np.testing.assert_allclose(o[3].cpu().numpy(), full[3].cpu().numpy(), atol=2e-6)
        assert torch.equal(o[4].cpu(), outs[0][4].cpu())
    got = (torch.cat([o[0] for o in outs]), outs[0][1], torch.cat([o[2] for o in outs]), outs[0][3],
           outs[0][4].reshape(1, C))
    _check_bags(got, [xh], w, [0], f"sharded C {C}")


# ---- backward, training objective, fused train step -----------------------------------------------------------------------
def _grad_err(got, ref, tag):
    worst = 0.0
    for k, r in ref.items():
        r = np.asarray(r, np.float64)
        g = got[k].detach().cpu().numpy().astype(np.float64) if torch.is_tensor(got[k]) else np.asarray(got[k], np.float64)
        scale = max(float(np.abs(r).max()), 1e-12)
        err = float(np.abs(g - r).max())
        assert err <= 2e-4 * scale + 2e-5, f"{tag} {k}: max err {err:.3e} vs scale {scale:.3e}"
        worst = max(worst, err / (2e-4 * scale + 2e-5))
    print(tag, "worst gradient error / bar", float("%.3g" % worst))


@pytest.mark.parametrize("C", [4, 17])
@pytest.mark.parametrize("N", [33, 3000, 70000])
def test_backward_dense_upstream_many_classes(C, N):
    """dsmil_agg_backward with dense random upstream gradients on pred, classes, A and B, against the fp64 autograd
    restatement; two runs bit-identical."""
    from dsmil_wsi_amd import ops
    K = 512
    rng = np.random.default_rng(900 + N + C)
    w = _weights(K, C, 900 + C)
    pg = _dev(w)
    x = torch.from_numpy(make_bag(8000 + N + C, N, K))
    xg = x.cuda()
    _, _, A, B, idx = _fwd(xg, [N], pg)
    g = {"pred": rng.standard_normal(C, dtype=np.float32), "classes": rng.standard_normal((N, C), dtype=np.float32),
         "A": rng.standard_normal((N, C), dtype=np.float32), "B": rng.standard_normal((C, K), dtype=np.float32)}
    g = {k: torch.from_numpy(v) for k, v in g.items()}
    gg = {k: v.cuda() for k, v in g.items()}

    def run():
        out = ops.agg_backward(xg, pg, A, B, idx, gg["pred"], g_classes=gg["classes"], g_A=gg["A"], g_B=gg["B"])
        return {k: v.clone() for k, v in out.items()}
    a = _poisoned(run)
    poison_workspace(ops)
    b = run()
    for k in a:
        assert torch.equal(a[k], b[k]), k
    ref = _autograd_f64(x, None, {k: torch.from_numpy(v) for k, v in w.items()}, idx[0].cpu(), True, g)
    _grad_err(a, {k: v.numpy() for k, v in ref.items()}, f"backward C {C} N {N}")


_PNAME = {"i_classifier.fc.0.weight": "fc_w", "i_classifier.fc.0.bias": "fc_b",
          "b_classifier.q.0.weight": "q0_w", "b_classifier.q.0.bias": "q0_b",
          "b_classifier.q.2.weight": "q2_w", "b_classifier.q.2.bias": "q2_b",
          "b_classifier.fcc.weight": "fcc_w", "b_classifier.fcc.bias": "fcc_b"}


@pytest.mark.parametrize("C", [3, 5, 64, 65])
def test_bag_loss_many_classes(C):
    """MILNet.bag_loss(...).backward(): the fused path (dsmil_agg_loss_head, C <= 64) and, at C = 65, the torch expression
    of the same objective over the native forward / backward — both against orc.train_loss_and_grads."""
    K, N = 512, 700
    w = _weights(K, C, 1000 + C)
    xh = make_bag(8100 + C, N, K)
    label = make_label(8100 + C, C)
    net = _net(w, K, C).train()
    x = torch.from_numpy(xh).cuda()
    y = torch.from_numpy(label).cuda()

    def run():
        net.zero_grad()
        loss, _, _ = net.bag_loss(x, y)
        loss.backward()
        return loss.item(), {_PNAME[k]: p.grad.clone() for k, p in net.named_parameters()}
    loss, grads = _poisoned(run)
    ref_loss, ref = orc.train_loss_and_grads(xh, label, w, dtype="f64")
    assert abs(loss - ref_loss) <= 1e-5 * abs(ref_loss), (loss, ref_loss)
    _grad_err(grads, ref, f"bag_loss C {C}")


def test_loss_head_and_train_step_refuse_more_than_64_classes():
    """The two entry points built on one wave of classes say so at C = 65 (MILNet.bag_loss then takes the torch expression,
    training.FusedTrainStep the generic path) and accept C = 64."""
    from dsmil_wsi_amd import ops
    for C, ok in ((64, True), (65, False)):
        cls = torch.zeros((10, C), device="cuda")
        pred = torch.zeros((1, C), device="cuda")
        idx = torch.zeros((1, C), dtype=torch.int64, device="cuda")
        lab = torch.zeros(C, device="cuda")
        if ok:
            ops.agg_loss_head(cls, pred, idx, lab)
        else:
            with pytest.raises(RuntimeError, match="unsupported"):
                ops.agg_loss_head(cls, pred, idx, lab)
    K, N, C = 64, 50, 65
    w = _dev(_weights(K, C, 65))
    params = [w[k] for k in KEYS]
    m = [torch.zeros_like(t) for t in params]
    v = [torch.zeros_like(t) for t in params]
    with pytest.raises(RuntimeError, match="unsupported"):
        ops.agg_train_step(torch.zeros((N, K), device="cuda"), torch.zeros(C, device="cuda"), params, m, v, 1, 1e-3,
                           (0.9, 0.999), 1e-8, 0.0)


@pytest.mark.parametrize("C", [3, 17, 64])
def test_train_step_gradient_from_first_moment(C):
    """dsmil_agg_train_step, one step with weight_decay = 0: the first Adam moment is (1 - beta1) g, so g = exp_avg / (1 - beta1)
    is the step's gradient — compared with the oracle's (the updated parameters are not: the first Adam step is nearly
    sign(g) and hides gradient errors)."""
    from dsmil_wsi_amd import ops
    K, N, b1 = 512, 1500, 0.9
    w = _weights(K, C, 1100 + C)
    xh = make_bag(8200 + C, N, K)
    label = make_label(8200 + C, C)
    x = torch.from_numpy(xh).cuda()
    y = torch.from_numpy(label).cuda()

    def run():
        params = [torch.from_numpy(np.ascontiguousarray(w[k])).cuda() for k in KEYS]
        m = [torch.zeros_like(t) for t in params]
        v = [torch.zeros_like(t) for t in params]
        loss = ops.agg_train_step(x, y, params, m, v, 1, 1e-3, (b1, 0.999), 1e-8, 0.0)
        return loss.clone(), m
    loss, m = _poisoned(run)
    ref_loss, ref = orc.train_loss_and_grads(xh, label, w, dtype="f64")
    assert abs(float(loss) - ref_loss) <= 1e-5 * abs(ref_loss), (float(loss), ref_loss)
    _grad_err({k: t / (1.0 - b1) for k, t in zip(KEYS, m)}, ref, f"train step C {C}")


# ---- FCLayer / IClassifier logits: k_fc ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [5, 17])
@pytest.mark.parametrize("K", [512, 166])
def test_fc_forward_many_classes(K, C):
    """dsmil_fc_forward on 100 001 rows: FCLayer alone and IClassifier(output_class = C) over an identity extractor — K = 512
    (k_fc<4>) and K = 166 through a view offset by one row (not 16-B aligned: k_fc<1>) — against fp64."""
    from dsmil_wsi_amd import modules as M
    N = 100_001
    rng = np.random.default_rng(1200 + K + C)
    wt = rng.standard_normal((C, K), dtype=np.float32) * 0.05
    bs = rng.standard_normal(C, dtype=np.float32) * 0.1
    big = torch.from_numpy(make_bag(8300 + K + C, N + 1, K)).cuda()
    x = big[1:] if K % 4 else big[:N]
    if K % 4:
        assert x.data_ptr() % 16 != 0
    ref = x.cpu().double().numpy() @ wt.T.astype(np.float64) + bs.astype(np.float64)
    fc = M.FCLayer(in_size=K, out_size=C).cuda()
    ic = M.IClassifier(torch.nn.Identity(), K, C).cuda()
    with torch.no_grad():
        fc.fc[0].weight.copy_(torch.from_numpy(wt))
        fc.fc[0].bias.copy_(torch.from_numpy(bs))
        ic.fc.weight.copy_(torch.from_numpy(wt))
        ic.fc.bias.copy_(torch.from_numpy(bs))
        feats, c1 = fc(x)
        _, c2 = ic(x)
    assert feats is x
    for c in (c1, c2):
        np.testing.assert_allclose(c.cpu().numpy(), ref, atol=1e-4, rtol=1e-5)
    print(f"fc K {K} C {C} max err", float(np.abs(c1.cpu().numpy() - ref).max()))
