"""The one-call batch training step on the GPU: dsmil_agg_train_step_bags / dsmil_agg_train_step_bags_bf16 through
ops.agg_train_step_bags, training.FusedTrainStep.step_bags and training.train against the generic path they replace
(MILNet.batch_loss under autograd, loss.backward(), torch.optim.Adam.step()).  Lengths come from the boundary lists of
tests/bwd_b16_cases.py (one row, the 32- / 64- / 128-row tile edges, many tiles).  Needs a real MI355X."""
import ctypes
import io
import types
from contextlib import redirect_stdout

import numpy as np
import pytest
import torch

from bwd_b16_cases import BATCH
from inputs import make_bag
from util import VARIANT, build_net, poison_workspace

pytestmark = pytest.mark.gpu

G1 = list(BATCH)            # [1, 2, 127, 128, 129, 31, 700]
G2 = [33, 64, 65]
F32, B16 = torch.float32, torch.bfloat16
HP = dict(lr=1e-3, betas=(0.5, 0.9), weight_decay=1e-3)   # (the fused one-bag test's: six steps move the weights)

# (tag, lengths, row dtype, dropout rate of the row map)
CASES = [("tcga", G1, F32, 0.4), ("tcga", G2, F32, 0.0), ("tcga", G1, B16, 0.0), ("tcga", G2, B16, 0.4),
         ("linq", G1, F32, 0.0), ("linq", G2, F32, 0.0), ("linq", G1, B16, 0.0), ("linq", G2, B16, 0.0),
         ("tree", G1, F32, 0.0), ("tree", G2, F32, 0.0), ("tree", G1, B16, 0.0), ("tree", G2, B16, 0.0),
         ("musk", G1, F32, 0.0), ("musk", G2, F32, 0.0),
         ("tcga", [1], B16, 0.0), ("tcga", [700], B16, 0.0)]
IDS = [f"{t}-{'x'.join(map(str, L)) if len(L) < 4 else 'G1'}-{'bf16' if d is B16 else 'fp32'}{'-map' if p else ''}" for t, L, d, p in CASES]


def _batch(tag, lengths, dtype, drop, seed):
    """One batch: rows [sum(lengths), K] on the GPU in ``dtype``, labels [n, C], and with ``drop`` the concatenated per-bag
    index lists (lengths then count the kept rows) — what training.train builds for a group (training._group)."""
    K, C = VARIANT[tag][0], VARIANT[tag][1]
    x = torch.from_numpy(np.concatenate([make_bag(seed + 13 * i, n, K) for i, n in enumerate(lengths)])).cuda().to(dtype)
    labels = torch.zeros(len(lengths), C)
    for b in range(len(lengths)):
        labels[b, (b + seed) % C] = float((b + seed) % 2) if C == 1 else 1.0
    row_map, kept = None, list(lengths)
    if drop:
        gen = torch.Generator().manual_seed(seed)
        maps, off, kept = [], 0, []
        for n in lengths:
            keep = max(1, int(n * (1 - drop)))
            maps.append(torch.randperm(n, generator=gen)[:keep] + off)
            off += n
            kept.append(keep)
        row_map = torch.cat(maps).cuda()
    return x, kept, labels.cuda(), row_map


def _generic_step(T, net, opt, crit, x, lengths, labels, row_map):
    opt.zero_grad()
    loss, _, _, each = T.batch_loss(net, crit, x, lengths, labels, row_map)
    loss.backward()
    opt.step()
    return loss.detach(), each


def _state(net, opt):
    """Bit copies of the parameters and both Adam moments, by parameter name."""
    out = {}
    for n, p in net.named_parameters():
        st = opt.state[p]
        out[n] = (p.detach().clone(), st["exp_avg"].clone(), st["exp_avg_sq"].clone())
    return out


@pytest.mark.parametrize("tag,lengths,dtype,drop", CASES, ids=IDS)
def test_step_bags_follows_the_generic_path(tag, lengths, dtype, drop):
    """Six steps of FusedTrainStep.step_bags (a lone bf16 bag: FusedTrainStep.__call__) against the generic path from the
    same start, at the bars of test_fused_train_step_follows_the_generic_path: per-bag and mean losses to 1e-5 max(1, |loss|),
    parameters to 1e-4 of their scale, exp_avg to 2e-4 of its scale, equal step counts.
    Both paths run the same gradient kernels on the same bits (the step's loss head scales g_pred / g_max by the separate
    fp32 product of the generic backward; the forward cuts the image the generic path hands in) and adam_elem is
    torch.optim.Adam's arithmetic, so on the MI355X run of this file parameters, exp_avg and exp_avg_sq came out
    BIT-identical in every case, row maps included; that is asserted.  Per-bag losses are bit-identical too; the mean is
    the sum in bag order and may differ from torch.mean in the last bit."""
    from dsmil_wsi_amd import training as T
    nets = [build_net(tag, "cuda").train() for _ in range(2)]
    opts = [torch.optim.Adam(n.parameters(), **HP) for n in nets]
    crit = torch.nn.BCEWithLogitsLoss()
    fused = T.FusedTrainStep.create(nets[1], crit, opts[1])
    assert fused is not None
    lone = len(lengths) == 1
    for step in range(6):
        x, kept, labels, row_map = _batch(tag, lengths, dtype, drop, 900 + 31 * step)
        assert fused.accepts(x)
        if lone:
            opts[0].zero_grad()
            l0, _, _ = T.bag_loss(nets[0], crit, x, labels, row_map)
            l0.backward()
            opts[0].step()
            l1 = fused(x, labels, row_map)
            e0, e1 = l0.detach().reshape(1), l1.reshape(1)
        else:
            l0, e0 = _generic_step(T, nets[0], opts[0], crit, x, kept, labels, row_map)
            l1, e1 = fused.step_bags(x, kept, labels, row_map)
        a, b = [float(l0.detach())] + e0.tolist(), [float(l1)] + e1.tolist()
        print(f"step {step}: mean {a[0]:.7f} / {b[0]:.7f}, per-bag bit-equal {torch.equal(e0, e1)}")
        assert torch.equal(e0, e1), (step, a, b)
        for u, v in zip(a, b):
            assert abs(u - v) <= 1e-5 * max(1.0, abs(u)), (step, a, b)
    fused.sync()
    exact = True
    for (n0, p0), (n1, p1) in zip(nets[0].named_parameters(), nets[1].named_parameters()):
        a, b = p0.detach().cpu().numpy(), p1.detach().cpu().numpy()
        s0, s1 = opts[0].state[p0], opts[1].state[p1]
        same = np.array_equal(a, b) and torch.equal(s0["exp_avg"], s1["exp_avg"]) and torch.equal(s0["exp_avg_sq"], s1["exp_avg_sq"])
        print(f"{n0}: bit-identical {same}, max diff {float(np.abs(a - b).max()):.3e}")
        exact = exact and same
        np.testing.assert_allclose(b, a, atol=1e-4 * max(1e-3, float(np.abs(a).max())), rtol=0, err_msg=n0)
        assert float(s0["step"]) == float(s1["step"]) == 6.0
        np.testing.assert_allclose(s1["exp_avg"].cpu().numpy(), s0["exp_avg"].cpu().numpy(),
                                   atol=2e-4 * max(1e-6, float(s0["exp_avg"].abs().max())), rtol=0, err_msg=n0)
    assert exact


GRAD_CASES = [("tcga", G1, F32, 0.4), ("tcga", G1, B16, 0.0), ("linq", G2, B16, 0.0), ("tree", G2, F32, 0.0),
              ("musk", G1, F32, 0.0), ("tcga", [700], B16, 0.0)]


@pytest.mark.parametrize("tag,lengths,dtype,drop", GRAD_CASES, ids=[IDS[CASES.index(c)] for c in GRAD_CASES])
def test_step_bags_gradient_from_first_moment(tag, lengths, dtype, drop):
    """One step with lr = 0, weight_decay = 0 and zero moments: exp_avg = (1 - beta1) g, so exp_avg / (1 - beta1) is the
    step's gradient (the method of test_train_step_gradient_from_first_moment) — against the generic path's .grad on the
    same batch at the bar of tests/test_bwd_bags_gpu.py / test_bwd_b16_gpu.py, 2e-4 of the tensor's max-abs + 2e-5; the
    parameters must be bit-unchanged."""
    from dsmil_wsi_amd import training as T
    nets = [build_net(tag, "cuda").train() for _ in range(2)]
    crit = torch.nn.BCEWithLogitsLoss()
    b1 = 0.5
    opt = torch.optim.Adam(nets[1].parameters(), lr=0.0, betas=(b1, 0.9), weight_decay=0.0)
    fused = T.FusedTrainStep.create(nets[1], crit, opt)
    x, kept, labels, row_map = _batch(tag, lengths, dtype, drop, 77)
    before = {n: p.detach().clone() for n, p in nets[1].named_parameters()}
    loss0, _, _, each0 = T.batch_loss(nets[0], crit, x, kept, labels, row_map)
    loss0.backward()
    loss1, each1 = fused.step_bags(x, kept, labels, row_map)
    assert abs(float(loss0) - float(loss1)) <= 1e-5 * max(1.0, abs(float(loss0)))
    for (n0, p0), (n1, p1) in zip(nets[0].named_parameters(), nets[1].named_parameters()):
        assert torch.equal(p1.detach(), before[n1]), n1
        ref = p0.grad.double().cpu().numpy()
        got = (opt.state[p1]["exp_avg"].double() / (1.0 - b1)).cpu().numpy()
        err, scale = float(np.abs(got - ref).max()), float(np.abs(ref).max())
        print(f"{n0}: max err {err:.3e} vs scale {scale:.3e}")
        assert err <= 2e-4 * scale + 2e-5, f"{n0}: max err {err:.3e} vs scale {scale:.3e}"


def _fresh(tag):
    """A step's operands from a fixed start: (parameters, exp_avg, exp_avg_sq) as new tensors, non-zero moments."""
    net = build_net(tag, "cuda")
    w = dict(net.b_classifier._weights())
    lin = net.i_classifier.fc[0]
    params = [lin.weight, lin.bias, w["q0_w"], w["q0_b"], w["q2_w"], w["q2_b"], w["fcc_w"], w["fcc_b"]]
    params = [p.detach().clone() if p is not None else None for p in params]
    gen = torch.Generator().manual_seed(3)
    m = [(torch.randn(p.shape, generator=gen) * 1e-3).cuda() if p is not None else None for p in params]
    v = [(torch.rand(p.shape, generator=gen) * 1e-5).cuda() if p is not None else None for p in params]
    return params, m, v


@pytest.mark.parametrize("tag,lengths,dtype,drop", [("tcga", G1, F32, 0.4), ("tcga", G1, B16, 0.0), ("linq", G2, F32, 0.0),
                                                     ("tcga", [1], B16, 0.0)])
def test_poisoned_workspace_and_determinism(tag, lengths, dtype, drop):
    """Two runs of one step from the same state give equal bits (no atomics, fixed summation order), and so does a run on a
    workspace whose every word was set to 0xFFFFFFFF before it: the step reads nothing it has not written itself."""
    from dsmil_wsi_amd import ops
    x, kept, labels, row_map = _batch(tag, lengths, dtype, drop, 41)
    nonlinear = bool(VARIANT[tag][2])

    def run(poison):
        params, m, v = _fresh(tag)
        if poison:
            poison_workspace(ops)
        loss, each = ops.agg_train_step_bags(x, kept, labels, params, m, v, 3, 1e-3, (0.5, 0.9), 1e-8, 1e-3,
                                             nonlinear=nonlinear, row_map=row_map)
        torch.cuda.synchronize()
        return [loss.clone(), each.clone()] + [t for t in params + m + v if t is not None]
    first, again, poisoned = run(False), run(False), run(True)
    assert all(torch.isfinite(t).all() for t in first)
    for i, (a, b, c) in enumerate(zip(first, again, poisoned)):
        assert torch.equal(a, b), f"output {i}: two runs differ"
        assert torch.equal(a, c), f"output {i}: the poisoned workspace changed it"


@pytest.mark.parametrize("dtype", [F32, B16], ids=["fp32", "bf16"])
def test_refused_step_changes_nothing(dtype):
    """A refused step raises and leaves parameters, moments and FusedTrainStep.step as they were: C = 65 through ops and
    through step_bags (labels 65 wide: DSMIL_E_UNSUPPORTED), and a label pointer off its 4-byte alignment straight at the
    C entry (DSMIL_E_ALIGN) — every check of the entry runs before its first launch."""
    from dsmil_wsi_amd import _native, ops
    from dsmil_wsi_amd import training as T
    net = build_net("tcga", "cuda").train()
    opt = torch.optim.Adam(net.parameters(), **HP)
    crit = torch.nn.BCEWithLogitsLoss()
    fused = T.FusedTrainStep.create(net, crit, opt)
    x, kept, labels, _ = _batch("tcga", G2, dtype, 0.0, 5)
    fused.step_bags(x, kept, labels)
    fused.sync()
    before, step = _state(net, opt), fused.step
    wide = torch.zeros(len(kept), 65, device="cuda")
    with pytest.raises(RuntimeError, match="dsmil_agg_train_step_bags"):
        fused.step_bags(x, kept, wide)
    params = [p.data if p is not None else None for p in fused.params]
    with pytest.raises(RuntimeError, match="dsmil_agg_train_step_bags"):
        ops.agg_train_step_bags(x, kept, wide, params, fused.m, fused.v, 2, 1e-3, (0.5, 0.9), 1e-8, 0.0)
    # the C entry itself, labels + 2 bytes
    K, C = VARIANT["tcga"][0], VARIANT["tcga"][1]
    ptr = lambda t: (t.data_ptr() if t is not None else 0)
    p = _native.AggParams(*[ptr(t) for t in params], K, K, C, 1)
    arr = ctypes.c_void_p * 8
    m_arr, v_arr = arr(*[ptr(t) for t in fused.m]), arr(*[ptr(t) for t in fused.v])
    st = _native.AdamState(ctypes.cast(m_arr, ctypes.POINTER(ctypes.c_void_p)), ctypes.cast(v_arr, ctypes.POINTER(ctypes.c_void_p)),
                           2, 1e-3, 0.5, 0.9, 1e-8, 0.0)
    off = ops.offsets_tensor(kept, x.device)
    out = torch.zeros(1 + len(kept), device="cuda")
    L = _native.lib()
    entry = "dsmil_agg_train_step_bags_bf16" if dtype is B16 else "dsmil_agg_train_step_bags"
    ws = ops._workspace(x.device, getattr(L, entry + "_workspace_bytes")(len(kept), sum(kept), K, C, 1))
    rmap = () if dtype is B16 else (None,)
    rc = getattr(L, entry)(x.data_ptr(), off.data_ptr(), len(kept), sum(kept), max(kept), *rmap, labels.data_ptr() + 2,
                           ctypes.byref(p), ctypes.byref(st), out[1:].data_ptr(), out[0:1].data_ptr(), ws.data_ptr(), ws.numel(),
                           None)
    assert rc == -5
    torch.cuda.synchronize()
    assert fused.step == step == 1
    after = _state(net, opt)
    for n in before:
        for a, b in zip(before[n], after[n]):
            assert torch.equal(a, b), n
    assert float(out.abs().sum()) == 0.0


@pytest.mark.parametrize("dtype", [F32, B16], ids=["fp32", "bf16"])
def test_mixed_fused_and_generic_steps_continue_one_optimiser_state(dtype):
    """fused batch step, generic step (between sync() / resync()), fused batch step — against three generic steps from the
    same start: the optimiser state continues (step count 3, parameters and exp_avg at the trajectory bars), and inference
    after the fused steps sees the new weights (the packed-weight caches are keyed on the version counters)."""
    from dsmil_wsi_amd import training as T
    nets = [build_net("tcga", "cuda").train() for _ in range(2)]
    opts = [torch.optim.Adam(n.parameters(), **HP) for n in nets]
    crit = torch.nn.BCEWithLogitsLoss()
    fused = T.FusedTrainStep.create(nets[1], crit, opts[1])
    probe = torch.from_numpy(make_bag(1, 300, VARIANT["tcga"][0])).cuda().to(dtype)
    with torch.no_grad():
        start = nets[1].eval()(probe)[1].float().clone()
    nets[1].train()
    for step in range(3):
        x, kept, labels, row_map = _batch("tcga", G2, dtype, 0.0, 300 + step)
        _generic_step(T, nets[0], opts[0], crit, x, kept, labels, row_map)
        if step == 1:
            fused.sync()
            _generic_step(T, nets[1], opts[1], crit, x, kept, labels, row_map)
            fused.resync()
        else:
            fused.step_bags(x, kept, labels, row_map)
        assert fused.step == step + 1
    fused.sync()
    for (n0, p0), (n1, p1) in zip(nets[0].named_parameters(), nets[1].named_parameters()):
        a, b = p0.detach().cpu().numpy(), p1.detach().cpu().numpy()
        s0, s1 = opts[0].state[p0], opts[1].state[p1]
        assert float(s0["step"]) == float(s1["step"]) == 3.0
        np.testing.assert_allclose(b, a, atol=1e-4 * max(1e-3, float(np.abs(a).max())), rtol=0, err_msg=n0)
        np.testing.assert_allclose(s1["exp_avg"].cpu().numpy(), s0["exp_avg"].cpu().numpy(),
                                   atol=2e-4 * max(1e-6, float(s0["exp_avg"].abs().max())), rtol=0, err_msg=n0)
    with torch.no_grad():
        o0, o1 = nets[0].eval()(probe)[1].float(), nets[1].eval()(probe)[1].float()
    assert float((o1 - start).abs().max()) > 1e-4          # the forward reads the updated weights, not a cached image
    np.testing.assert_allclose(o1.cpu().numpy(), o0.cpu().numpy(), atol=1e-4 if dtype is F32 else 2e-2)


WORK = {"dsmil_agg_forward_ex", "dsmil_agg_forward_bf16", "dsmil_agg_forward", "dsmil_agg_loss_head", "dsmil_agg_loss_head_bags",
        "dsmil_agg_backward", "dsmil_agg_backward_ex", "dsmil_agg_backward_rows", "dsmil_agg_backward_bags",
        "dsmil_agg_backward_bags_bf16", "dsmil_agg_train_step", "dsmil_agg_train_step_bags", "dsmil_agg_train_step_bags_bf16",
        "dsmil_agg_pack_split", "dsmil_agg_pack_f2", "dsmil_agg_pack_bf16", "dsmil_adam_step"}


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


@pytest.mark.parametrize("dtype", [F32, B16], ids=["fp32", "bf16"])
def test_train_takes_one_native_call_per_group(monkeypatch, dtype):
    """training.train(bags_per_step = 4, dropout_patch = 0.3) with Adam on ten bags (three groups, the last one short), fp32
    and a bf16 cache: ONE dsmil_agg_train_step_bags[_bf16] per group and no other work entry — no forward, loss head or
    dsmil_agg_backward_bags* call, no weight packing from Python — and one progress line per bag, in order.  With
    args.fused_step = False the same run takes the generic entries."""
    from dsmil_wsi_amd import _native
    from dsmil_wsi_amd import training as T
    K, C = VARIANT["tcga"][0], VARIANT["tcga"][1]
    n = 10
    sizes = [40, 3, 129, 64, 300, 33, 2, 700, 65, 128]     # (dropout_patch 0.3 keeps int(0.7 n) rows: at least two per bag)
    bags = {i: (torch.from_numpy(make_bag(600 + i, sizes[i], K)).cuda().to(dtype), torch.tensor([[float(i % 2), float((i // 2) % 2)]]).cuda())
            for i in range(n)}

    class Cache:
        def get(self, item, feats_size=None):
            return bags[item]
    rec = _Recorder(_native.lib())
    monkeypatch.setattr(_native, "lib", lambda: rec)
    crit = torch.nn.BCEWithLogitsLoss()
    entry = "dsmil_agg_train_step_bags_bf16" if dtype is B16 else "dsmil_agg_train_step_bags"
    for fused_on in (True, False):
        net = build_net("tcga", "cuda").train()
        opt = torch.optim.Adam(net.parameters(), **HP)
        args = types.SimpleNamespace(feats_size=K, dropout_patch=0.3, bags_per_step=4, fused_step=fused_on)
        np.random.seed(3)
        torch.manual_seed(3)
        rec.calls.clear()
        buf = io.StringIO()
        with redirect_stdout(buf):
            mean = T.train(args, list(range(n)), net, crit, opt, cache=Cache())
        calls = [c for c in rec.calls if c in WORK]
        if fused_on:
            assert calls == [entry] * 3, calls
        else:
            assert entry not in calls and sum(c.startswith("dsmil_agg_backward_bags") for c in calls) == 3, calls
        lines = [s for s in buf.getvalue().split("\r") if s.strip()]
        assert [s.split("]")[0].strip() for s in lines] == [f"Training bag [{i}/{n}" for i in range(n)], lines
        assert np.isfinite(mean) and 0.0 < mean < 5.0
        assert float(opt.state[next(net.parameters())]["step"]) == 3.0
