"""The native value stream on bf16-stored rows (BClassifier(passing_v=True), dsmil.py:35-39,48, in front of the bf16-storage
aggregator): ops.value_proj on bf16 rows (dsmil_value_forward_bf16: k_value_proj_b16 / k_value_proj_b16_valu,
csrc/agg_value.h) and the module routes through it.  Needs a real MI355X.

(a) the projection against fp64 of the bf16-rounded operands, |V - ref| <= 2^-8 |ref| + 1.01 K 2^-24 S (derived in
    tests/test_value_b16_host.py, which shows the reference arithmetic reaches it); (b) bit-for-bit determinism, row
independence and image / no-image agreement; (c) the whole model against the fp64 oracle on rounded values at the bars of
tests/test_agg_bf16_gpu.py::_check (rounding V to bf16 adds at most 2^-9 relative error to B = A^T V: A >= 0 and V >= 0, no
cancellation — far inside that file's 2e-2); (d) the native entries the glue calls.

``MILNet.forward`` returns its results in the rows' dtype (bf16 here: existing behaviour, pinned by
test_agg_bf16_gpu.py::test_bf16_module_and_varlen_batch), and a bf16-rounded instance logit cannot sit within _check's 1e-4 of
anything.  So _check is applied to the fp32 results of the same native calls (``forward_bags`` of the one bag), and
``forward`` must return exactly those, rounded to bf16 — bit for bit, which asks more than a tolerance would."""
import ctypes

import numpy as np
import pytest
import torch

import agg_oracle as orc
from inputs import make_bag
from test_agg_bf16_gpu import _check
from util import build_net, load_weights
from value_b16_cases import SHAPES, bar, make_case, reference, round_bf16

pytestmark = pytest.mark.gpu


def _dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    return t if dtype is None else t.to(dtype)


# ---- (a) the projection against fp64 ---------------------------------------------------------------------------------------
def _proj_case(rows, K, Kv, bias_shift=0.0):
    from dsmil_wsi_amd import ops
    x, w, b = make_case(rows, K, Kv, bias_shift)
    V = ops.value_proj(_dev(x, torch.bfloat16), _dev(w), _dev(b))          # fp32 master weights: rounded inside
    assert V.dtype == torch.bfloat16 and tuple(V.shape) == (rows, Kv)
    ref, S = reference(round_bf16(x), round_bf16(w), round_bf16(b))
    err = np.abs(V.float().cpu().numpy().astype(np.float64) - ref)
    lim = bar(ref, S, K)
    print(f"value_proj bf16 {rows}x{K}x{Kv} shift {bias_shift:g}: max err {err.max():.3e}, worst err / bar "
          f"{float((err / lim)[lim > 0].max()):.3f}, clamped {float((ref == 0).mean()):.2f}")
    assert np.all(err <= lim)
    return ref


@pytest.mark.parametrize("rows,K,Kv", SHAPES)
def test_value_proj_b16_vs_fp64(rows, K, Kv):
    _proj_case(rows, K, Kv)


def test_value_proj_b16_negative_bias_clamps():
    ref = _proj_case(257, 512, 512, bias_shift=-1.0)
    assert (ref == 0).mean() >= 0.25


def test_value_proj_b16_takes_bf16_parameters():
    """The weights of a module after .bfloat16() give the bits the fp32 masters give (the same rounding, done outside)."""
    from dsmil_wsi_amd import ops
    x, w, b = make_case(129, 72, 68)
    xb = _dev(x, torch.bfloat16)
    assert torch.equal(ops.value_proj(xb, _dev(w), _dev(b)), ops.value_proj(xb, _dev(w, torch.bfloat16), _dev(b, torch.bfloat16)))


# ---- (b) determinism and row independence, bit for bit ---------------------------------------------------------------------
@pytest.mark.parametrize("rows,K,Kv", [(257, 512, 512), (257, 72, 68), (257, 1032, 64)])
def test_value_proj_b16_bits(rows, K, Kv):
    from dsmil_wsi_amd import _native, ops
    x, w, b = make_case(rows, K, Kv)
    xb, wd, bd = _dev(x, torch.bfloat16), _dev(w), _dev(b)
    V = ops.value_proj(xb, wd, bd)
    assert torch.equal(V, ops.value_proj(xb, wd, bd))                       # two runs
    a_, b_ = 33, 200
    assert torch.equal(V[a_:b_], ops.value_proj(xb[a_:b_], wd, bd))         # a row's bits do not depend on its place
    # packed == NULL: the weights are rounded into the workspace by the same call
    L = _native.lib()
    b_r = bd.to(torch.bfloat16).float().contiguous()
    ws = torch.empty(int(L.dsmil_value_workspace_bf16_bytes(rows, K, Kv)) + 256, dtype=torch.uint8, device="cuda")
    assert ws.data_ptr() % 256 == 0
    V2 = torch.empty_like(V)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    rc = L.dsmil_value_forward_bf16(p(xb), rows, K, Kv, p(wd), p(b_r), None, p(V2), p(ws), ws.numel(),
                                    ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0
    torch.cuda.synchronize()
    assert torch.equal(V, V2)


# ---- (c) whole model ---------------------------------------------------------------------------------------------------------
LENGTHS = (1, 37, 500)


def _model(K):
    """MILNet(FCLayer, BClassifier(passing_v=True)), C = 2, on the GPU with fp32 parameters, and the parameters under the
    oracle's names: K = 64 is the `passv` weight set, K = 512 is drawn as tests/test_value_gpu.py::_make_net draws it."""
    if K == 64:
        return build_net("passv", "cuda"), load_weights("passv")
    from dsmil_wsi_amd import modules as M
    net = M.MILNet(M.FCLayer(in_size=K, out_size=2),
                   M.BClassifier(input_size=K, output_class=2, dropout_v=0.0, nonlinear=True, passing_v=True)).eval()
    g = torch.Generator().manual_seed(40 + K)
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


_REFS = {}


def _bags_and_refs(K):
    """The three bags (host fp32) and their fp64 oracle results on bf16-rounded rows and parameters: computed once per K."""
    if K not in _REFS:
        _, p = _model(K)
        pr = {k: round_bf16(v) for k, v in p.items()}
        bags = [make_bag(8100 + K + n, n, K) for n in LENGTHS]
        _REFS[K] = (bags, [orc.milnet_forward(round_bf16(b), pr, passing_v=True, dtype="f64") for b in bags])
    return _REFS[K]


@pytest.mark.parametrize("kind", ["fp32_master", "bfloat16_module"])
@pytest.mark.parametrize("K", [64, 512])
def test_milnet_passing_v_on_bf16_rows(K, kind):
    net, _ = _model(K)
    if kind == "bfloat16_module":
        net = net.to(torch.bfloat16)
    bags, refs = _bags_and_refs(K)
    xs = [_dev(b, torch.bfloat16) for b in bags]
    with torch.no_grad():
        together = net.forward_bags(xs)                       # all three bags in one call
        for x, ref, n, tog in zip(xs, refs, LENGTHS, together):
            one = net.forward_bags([x])[0]                    # fp32 results of the one-bag native calls
            _check(one, ref, n)
            assert np.array_equal(np.argmax(one[0].cpu().numpy(), axis=0), ref[4])
            _check(tog, ref, n)
            assert np.array_equal(np.argmax(tog[0].cpu().numpy(), axis=0), ref[4])
            _check(tog, [t.float().cpu().numpy() for t in one], n)    # forward_bags equals the per-bag call
            fwd = net(x)                                      # forward: the same calls, results in the rows' dtype
            assert all(t.dtype == torch.bfloat16 for t in fwd) and fwd[1].shape == (1, 2) and fwd[3].shape == (1, 2, K)
            for got, want in zip(fwd, one):
                assert torch.equal(got, want.to(torch.bfloat16).reshape(got.shape))
        # graphed(37): the replay equals the eager call bit for bit, twice
        run = net.graphed(37, dtype=torch.bfloat16) if kind == "fp32_master" else net.graphed(37)
        eager = [t.clone() for t in net.forward_bags([xs[1]])[0]]
        for _ in range(2):
            got = run(xs[1])
            torch.cuda.synchronize()
            for u, v in zip(got, eager):
                assert u.dtype == torch.float32 and torch.equal(u.reshape(v.shape), v)
        _check(got, refs[1], 37)


def test_active_dropout_on_bf16_rows_keeps_the_torch_route():
    """An ACTIVE dropout of the value layer is torch's own: a .bfloat16() module in training mode still runs, through
    nn.Linear + ReLU, and classes / A — which do not see the value layer — equal the eval-mode results."""
    from dsmil_wsi_amd import modules as M
    net = M.MILNet(M.FCLayer(64, 2), M.BClassifier(64, 2, dropout_v=0.5, passing_v=True)).cuda().to(torch.bfloat16)
    x = _dev(make_bag(5, 100, 64), torch.bfloat16)
    with torch.no_grad():
        ev, tr = net.eval()(x), net.train()(x)
    assert torch.equal(ev[0], tr[0]) and torch.equal(ev[2], tr[2]) and not torch.equal(ev[3], tr[3])
    assert all(bool(torch.isfinite(t.float()).all()) for t in tr)


# ---- (d) route ---------------------------------------------------------------------------------------------------------------
PACKS = {"dsmil_agg_pack_split", "dsmil_agg_pack_f2", "dsmil_value_pack", "dsmil_agg_pack_bf16", "dsmil_value_pack_bf16"}
WORK = PACKS | {"dsmil_agg_forward_ex", "dsmil_agg_forward_bf16", "dsmil_agg_forward", "dsmil_value_forward",
                "dsmil_value_forward_bf16", "dsmil_fc_forward"}


class _Recorder:
    """Stands in for the loaded library (as in tests/test_glue_calls_gpu.py): attribute access hands out the real function
    wrapped to note its name."""

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


def test_bf16_passing_v_calls_the_bf16_entries_and_packs_once(monkeypatch):
    from dsmil_wsi_amd import _native, ops
    rec = _Recorder(_native.lib())
    monkeypatch.setattr(_native, "lib", lambda: rec)
    net = build_net("passv", "cuda")                          # a fresh module: a weight set nothing has packed yet
    xs = [_dev(make_bag(60 + n, n, 64), torch.bfloat16) for n in (5, 64, 33)]
    with torch.no_grad():
        net(xs[0])
        packs, calls = rec.take()
        assert calls == ["dsmil_value_forward_bf16", "dsmil_agg_forward_bf16"], calls
        assert sorted(packs) == ["dsmil_agg_pack_bf16", "dsmil_value_pack_bf16"], packs
        net(xs[1])
        packs, calls = rec.take()
        assert packs == [] and calls == ["dsmil_value_forward_bf16", "dsmil_agg_forward_bf16"], (packs, calls)
        net.forward_bags(xs)                                  # ONE projection over the concatenated rows, one aggregator call
        packs, calls = rec.take()
        assert packs == [] and calls == ["dsmil_value_forward_bf16", "dsmil_agg_forward_bf16"], (packs, calls)
        pool = ops.StreamPool(2)
        outs = [pool.run(net, xs[2]) for _ in range(2)]       # the second stream waits for the image, it does not cut another
        pool.join()
        packs, calls = rec.take()
        assert packs == [] and calls == ["dsmil_value_forward_bf16", "dsmil_agg_forward_bf16"] * 2, (packs, calls)
        ref = net(xs[2])
    torch.cuda.synchronize()
    for out in outs:
        for u, v in zip(out, ref):
            assert torch.equal(u, v)
