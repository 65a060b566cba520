"""The class-weighted objective of the C-ABI (struct dsmil_bce_weights; dsmil_agg_loss_head_w, dsmil_agg_loss_head_bags_w,
dsmil_agg_train_step_bags_w, dsmil_agg_train_step_bags_bf16_w) is declared, exported and bound without a change of the ABI
version, each entry has its sibling's signature plus the weights in front of the stream, and refuses what its sibling refuses
with the same codes in the same order, before any launch — plus DSMIL_E_ALIGN for a weight pointer off its 4-byte alignment.
training._native_bce names the criteria the native objective computes.  CPU only: the pointers are aligned host memory that
no check dereferences as device memory, and every call here is a refused one."""
import ctypes
import os
import re

import pytest
import torch
import torch.nn as nn

import dsmil  # noqa: F401  (registers the dsmil_wsi_amd package)
import dsmil_wsi_amd._native as nat

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADS = ("dsmil_agg_loss_head", "dsmil_agg_loss_head_bags")
STEPS = ("dsmil_agg_train_step_bags", "dsmil_agg_train_step_bags_bf16")
INVALID, UNSUPPORTED, WORKSPACE, ALIGN = -1, -2, -3, -5


def test_weighted_symbols_are_declared_exported_and_bound():
    raw = open(os.path.join(ROOT, "include", "dsmil_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    lib = ctypes.CDLL(nat.LIB_PATH)
    assert re.search(r"typedef struct dsmil_bce_weights \{\s*const float\* pos_weight;\s*const float\* weight;\s*\} dsmil_bce_weights;", src)
    assert [f[0] for f in nat.BceWeights._fields_] == ["pos_weight", "weight"]
    assert ctypes.sizeof(nat.BceWeights) == 2 * ctypes.sizeof(ctypes.c_void_p)
    for sibling in HEADS + STEPS:
        name = sibling + "_w"
        assert re.search(r"\b%s\s*\(" % name, src), f"{name} is not declared in include/dsmil_hip.h"
        assert hasattr(lib, name), f"{name} is not exported"
        assert name in nat.SIGNATURES, f"{name} is not in the binding table"
        # the sibling's signature with `const dsmil_bce_weights*` in front of the stream
        res, args = nat.SIGNATURES[sibling]
        assert nat.SIGNATURES[name] == (res, args[:-1] + [ctypes.POINTER(nat.BceWeights)] + args[-1:])
        decl = re.search(r"\b%s\s*\(([^;]*)\)\s*;" % name, src).group(1)
        assert re.search(r"const dsmil_bce_weights\*\s*\w+,\s*void\*\s*stream\s*$", decl), decl
        # the contract in front of the declaration cites the reference lines it replaces
        doc = raw[:raw.index("int " + name + "(")]
        doc = doc[doc.rindex("/*"):]
        assert "train_mil.py:172-173" in doc and ":52-55" in doc, name
        assert not hasattr(lib, name + "_workspace_bytes")          # the sibling's size query answers for both
    assert int(re.search(r"#define DSMIL_ABI_VERSION (\d+)", raw).group(1)) == 6
    assert nat.lib().dsmil_abi_version() == 6


class _Mem:
    """256-byte aligned host memory for the pointers of a refused call."""

    def __init__(self):
        self.buf = (ctypes.c_char * 8192)()
        self.a = (ctypes.addressof(self.buf) + 255) // 256 * 256

    def weights(self, pos_off=0, w_off=0, pos=True, w=True):
        return nat.BceWeights(self.a + pos_off if pos else None, self.a + w_off if w else None)


def _head(entry, mem, C=2, loss=True, bw=None):
    p = ctypes.c_void_p(mem.a)
    out = p if loss else None
    fn = getattr(nat.lib(), entry + "_w")
    bw = ctypes.byref(bw) if bw is not None else None
    if entry == HEADS[0]:
        return fn(p, p, p, p, C, out, p, p, p, bw, None)
    return fn(p, p, p, p, p, 3, C, out, p, p, p, bw, None)


@pytest.mark.parametrize("entry", HEADS)
def test_weighted_loss_heads_refuse_as_their_siblings(entry):
    M = _Mem()
    p = ctypes.c_void_p(M.a)
    sib = getattr(nat.lib(), entry)
    # the sibling's codes, in the sibling's order: INVALID, then UNSUPPORTED (C = 65), then the weights' alignment
    assert _head(entry, M, loss=False, bw=M.weights()) == INVALID
    assert _head(entry, M, C=0, bw=M.weights()) == INVALID
    assert _head(entry, M, C=65, loss=False, bw=M.weights(pos_off=2)) == INVALID
    assert _head(entry, M, C=65, bw=M.weights()) == UNSUPPORTED
    assert _head(entry, M, C=65, bw=None) == UNSUPPORTED
    assert _head(entry, M, C=65, bw=M.weights(pos_off=2, w_off=1)) == UNSUPPORTED
    if entry == HEADS[0]:
        assert sib(p, p, p, p, 65, p, p, p, p, None) == UNSUPPORTED and sib(p, p, p, p, 2, None, p, p, p, None) == INVALID
    else:
        assert sib(p, p, p, p, p, 3, 65, p, p, p, p, None) == UNSUPPORTED
        assert sib(p, p, p, p, p, 3, 2, None, p, p, p, None) == INVALID
        assert sib(p, p, p, p, p, 0, 2, p, p, p, p, None) == INVALID
    for off in (1, 2, 3):
        assert _head(entry, M, bw=M.weights(pos_off=off)) == ALIGN
        assert _head(entry, M, bw=M.weights(w_off=off)) == ALIGN
        assert _head(entry, M, C=64, bw=M.weights(pos_off=off, w=False)) == ALIGN
        assert _head(entry, M, C=64, bw=M.weights(w_off=off, pos=False)) == ALIGN


class _StepArgs:
    """Arguments of one refused step (tests/test_step_bags_cabi.py): every pointer is 256-byte aligned host memory."""

    def __init__(self, K=64, C=2, step=1):
        self.mem = _Mem()
        a = self.a = self.mem.a
        self.params = nat.AggParams(a, a, a, a, a, a, a, a, K, K, C, 1)
        self.m = (ctypes.c_void_p * 8)(*([a] * 8))
        self.v = (ctypes.c_void_p * 8)(*([a] * 8))
        self.opt = nat.AdamState(ctypes.cast(self.m, ctypes.POINTER(ctypes.c_void_p)),
                                 ctypes.cast(self.v, ctypes.POINTER(ctypes.c_void_p)), step, 1e-3, 0.5, 0.9, 1e-8, 0.0)
        p = ctypes.c_void_p
        self.kw = dict(feats=p(a), offsets=p(a), n_bags=3, total=40, max_rows=20, row_map=None, labels=p(a),
                       params=ctypes.byref(self.params), opt=ctypes.byref(self.opt), loss_each=p(a), loss=p(a), ws=p(a),
                       ws_bytes=1 << 40, bw=None)

    def call(self, entry, weighted=True, **over):
        k = dict(self.kw, **over)
        rmap = (k["row_map"],) if entry == STEPS[0] else ()
        bw = ((ctypes.byref(k["bw"]) if k["bw"] is not None else None),) if weighted else ()
        return getattr(nat.lib(), entry + ("_w" if weighted else ""))(
            k["feats"], k["offsets"], k["n_bags"], k["total"], k["max_rows"], *rmap, k["labels"], k["params"], k["opt"],
            k["loss_each"], k["loss"], k["ws"], k["ws_bytes"], *bw, None)


@pytest.mark.parametrize("entry", STEPS)
def test_weighted_steps_refuse_as_their_siblings(entry):
    p = ctypes.c_void_p
    A = _StepArgs()
    good, bad_pos, bad_w = A.mem.weights(), A.mem.weights(pos_off=2), A.mem.weights(w_off=1, pos=False)
    # every refusal of the sibling, with the sibling's code, whatever the weights are
    for bw in (None, good, bad_pos, bad_w, A.mem.weights(pos=False, w=False)):
        for kw, code in (({"loss": None}, INVALID), ({"feats": None}, INVALID), ({"n_bags": 0}, INVALID),
                         ({"ws": p(A.a + 16), "ws_bytes": 16}, ALIGN), ({"labels": p(A.a + 2), "ws_bytes": 16}, ALIGN)):
            assert A.call(entry, bw=bw, **kw) == code == A.call(entry, weighted=False, **kw), (kw, code)
        assert _StepArgs(C=65).call(entry, bw=bw, ws=p(A.a + 16), ws_bytes=16) == UNSUPPORTED     # before any launch
        assert _StepArgs(C=65, step=0).call(entry, bw=bw) == INVALID
        assert A.call(entry, bw=bw, total=(1 << 30) + 1, max_rows=5) == UNSUPPORTED
    # a weight pointer off its 4-byte alignment: DSMIL_E_ALIGN, behind UNSUPPORTED and in front of WORKSPACE
    assert A.call(entry, bw=bad_pos, ws_bytes=16) == ALIGN
    assert A.call(entry, bw=bad_w, ws_bytes=16) == ALIGN
    assert _StepArgs(C=64).call(entry, bw=bad_w, ws_bytes=16) == ALIGN
    # aligned weights, a NULL struct, two NULL members: the sibling's workspace check, against the sibling's size
    size = getattr(nat.lib(), entry + "_workspace_bytes")(3, 40, 64, 2, 1)
    for bw in (None, good, A.mem.weights(pos=False, w=False)):
        assert A.call(entry, bw=bw, ws_bytes=16) == WORKSPACE
        assert A.call(entry, bw=bw, ws_bytes=size - 1) == WORKSPACE
    assert A.call(entry, weighted=False, ws_bytes=size - 1) == WORKSPACE


class _Sub(nn.BCEWithLogitsLoss):
    pass


class _Override(nn.BCEWithLogitsLoss):
    def forward(self, input, target):
        return super().forward(input, target) * 2


def test_native_bce_accepts_per_class_weights_only():
    from dsmil_wsi_amd.training import _native_bce
    t = torch.tensor
    assert _native_bce(nn.BCEWithLogitsLoss()) == (None, None)
    assert _native_bce(nn.BCEWithLogitsLoss(), 3) == (None, None)
    assert _native_bce(_Sub()) == (None, None)
    C = 3
    # 0-dim (what train_mil.py:172 builds), [1], [C], [1, C] — as pos_weight, as weight, as both
    for w in (t(2.5), t([2.5]), t([0.5, 1.0, 2.0]), t([[0.5, 1.0, 2.0]]), t([[2.5]]), t([1.0, 2.0, 3.0], dtype=torch.float64)):
        crit = nn.BCEWithLogitsLoss(pos_weight=w)
        got = _native_bce(crit, C)
        assert got is not None and got[0] is crit.pos_weight and got[1] is None
        crit = nn.BCEWithLogitsLoss(weight=w)
        got = _native_bce(crit, C)
        assert got is not None and got[1] is crit.weight and got[0] is None
        crit = _Sub(weight=w, pos_weight=t(3.0))
        got = _native_bce(crit, C)
        assert got is not None and got[0] is crit.pos_weight and got[1] is crit.weight
        assert _native_bce(crit) is not None                       # without C: the shape alone
    # rejected: another reduction, a shape that is not per class, an element count that is neither 1 nor C, an overridden
    # forward, another loss
    assert _native_bce(nn.BCEWithLogitsLoss(reduction="sum")) is None
    assert _native_bce(nn.BCEWithLogitsLoss(reduction="none", pos_weight=t(2.0))) is None
    for w in (t([[0.5], [1.0], [2.0]]), t([[0.5, 1.0, 2.0], [0.5, 1.0, 2.0]]), torch.ones(1, 1, C)):
        assert _native_bce(nn.BCEWithLogitsLoss(pos_weight=w), C) is None
        assert _native_bce(nn.BCEWithLogitsLoss(weight=w), C) is None
    for w in (t([0.5, 1.0]), t([[0.5, 1.0, 2.0, 4.0]]), torch.ones(0)):
        assert _native_bce(nn.BCEWithLogitsLoss(pos_weight=w), C) is None
        assert _native_bce(nn.BCEWithLogitsLoss(pos_weight=t(2.0), weight=w), C) is None
    assert _native_bce(nn.BCEWithLogitsLoss(pos_weight=t([0.5, 1.0])), 2) is not None
    assert _native_bce(_Override()) is None
    assert _native_bce(_Override(pos_weight=t(2.0)), C) is None
    assert _native_bce(nn.BCELoss()) is None
    assert _native_bce(nn.MSELoss()) is None
    assert _native_bce(None) is None


def test_fused_train_step_declines_off_the_gpu():
    """FusedTrainStep.create on CPU parameters: None for the weighted criterion as for the stock one (the CPU path did not move)."""
    import dsmil as mil
    from dsmil_wsi_amd.training import FusedTrainStep
    net = mil.MILNet(mil.FCLayer(8, 1), mil.BClassifier(input_size=8, output_class=1))
    opt = torch.optim.Adam(net.parameters(), lr=1e-3)
    assert FusedTrainStep.create(net, nn.BCEWithLogitsLoss(torch.tensor(2.0)), opt) is None
    assert FusedTrainStep.create(net, nn.BCEWithLogitsLoss(), opt) is None
