"""The one-call batch training step of the C-ABI (dsmil_agg_train_step_bags, dsmil_agg_train_step_bags_bf16 and their
workspace queries; csrc/agg_bwd_bags.h) is declared, exported and bound without a change of the ABI version, and its size /
error paths answer without a device, in the documented order: DSMIL_E_INVALID, DSMIL_E_UNSUPPORTED, DSMIL_E_ALIGN,
DSMIL_E_WORKSPACE, all before the first launch.  CPU only: the pointers are aligned host memory that no check dereferences
as device memory."""
import ctypes
import os
import re

import pytest

import dsmil  # noqa: F401  (registers the dsmil_wsi_amd package)
import dsmil_wsi_amd._native as nat

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("dsmil_agg_train_step_bags", "dsmil_agg_train_step_bags_bf16")
SYMBOLS = ENTRIES + tuple(e + "_workspace_bytes" for e in ENTRIES)
INVALID, UNSUPPORTED, WORKSPACE, ALIGN = -1, -2, -3, -5


def test_step_bags_symbols_are_declared_exported_and_bound():
    raw = open(os.path.join(ROOT, "include", "dsmil_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    lib = ctypes.CDLL(nat.LIB_PATH)
    for name in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, src), f"{name} is not declared in include/dsmil_hip.h"
        assert hasattr(lib, name), f"{name} is not exported"
        assert name in nat.SIGNATURES, f"{name} is not in the binding table"
    assert int(re.search(r"#define DSMIL_ABI_VERSION (\d+)", raw).group(1)) == 6
    assert nat.lib().dsmil_abi_version() == 6
    # the bf16 entry is the fp32 one without its row_map argument, the row pointer untyped
    f32, b16 = nat.SIGNATURES[ENTRIES[0]], nat.SIGNATURES[ENTRIES[1]]
    assert b16[0] is f32[0] and b16[1][0] is ctypes.c_void_p
    assert b16[1][1:] == f32[1][1:5] + f32[1][6:]
    assert nat.SIGNATURES[SYMBOLS[2]] == nat.SIGNATURES[SYMBOLS[3]]
    # the contract cites the reference lines it replaces
    doc = raw[raw.index("one training step on a BATCH of bags per C call"):raw.index("size_t dsmil_agg_train_step_bags_workspace_bytes")]
    assert "train_tcga.py:60-75" in doc


def test_step_bags_workspace_sizes():
    L = nat.lib()
    f32, b16 = L.dsmil_agg_train_step_bags_workspace_bytes, L.dsmil_agg_train_step_bags_bf16_workspace_bytes
    for size in (f32, b16):
        for bad in ((0, 1000, 512, 2, 1), (-1, 1000, 512, 2, 1), (4, 0, 512, 2, 1), (4, -7, 512, 2, 1), (4, 3, 512, 2, 1),
                    (4, 1000, 0, 2, 1), (4, 1000, 512, 0, 1)):
            assert size(*bad) == 0, bad
    assert b16(4, 1000, 20, 2, 1) == 0 and f32(4, 1000, 20, 2, 1) > 0         # bf16 rows need K % 8 == 0
    for shape in ((1, 1, 512, 2, 1), (1, 700, 512, 2, 1), (7, 1118, 512, 2, 1), (3, 162, 1024, 1, 0), (64, 640000, 512, 2, 1)):
        n, T, K, C, nl = shape
        # the batched forward's workspace + the batched backward's + the eight gradient tensors, at the least
        parts = L.dsmil_agg_workspace_bytes(n, T, K, K, C) + L.dsmil_agg_backward_bags_workspace_bytes(n, T, K, K, C)
        if not nl:   # (that query answers for the two-layer query, the larger layout)
            parts = L.dsmil_agg_workspace_bytes(n, T, K, K, C)
        grads = 4 * (C * K + C + 128 * K + 128 + (128 * 128 + 128 if nl else 0) + C * C * K + C)
        assert f32(*shape) >= parts + grads, shape
        # bf16: plus the rounded parameter set and its packed image
        assert b16(*shape) >= f32(*shape) + grads + L.dsmil_agg_packed_bf16_bytes(K), shape


class _Args:
    """Arguments of one refused call: every pointer is 256-byte aligned host memory unless a test moves it."""

    def __init__(self, K=64, C=2, nonlinear=1, Kv=None, step=1):
        self.buf = (ctypes.c_char * 8192)()
        self.a = (ctypes.addressof(self.buf) + 255) // 256 * 256
        a = self.a
        self.params = nat.AggParams(a, a, a, a, a, a, a, a, K, K if Kv is None else Kv, C, nonlinear)
        self.m = (ctypes.c_void_p * 8)(*([a] * 8))
        self.v = (ctypes.c_void_p * 8)(*([a] * 8))
        self.opt = nat.AdamState(ctypes.cast(self.m, ctypes.POINTER(ctypes.c_void_p)),
                                 ctypes.cast(self.v, ctypes.POINTER(ctypes.c_void_p)), step, 1e-3, 0.5, 0.9, 1e-8, 0.0)
        p = ctypes.c_void_p
        self.kw = dict(feats=p(a), offsets=p(a), n_bags=3, total=40, max_rows=20, row_map=None, labels=p(a),
                       params=ctypes.byref(self.params), opt=ctypes.byref(self.opt), loss_each=p(a), loss=p(a), ws=p(a),
                       ws_bytes=1 << 40)

    def call(self, entry, **over):
        k = dict(self.kw, **over)
        rmap = (k["row_map"],) if entry == ENTRIES[0] else ()
        return getattr(nat.lib(), entry)(k["feats"], k["offsets"], k["n_bags"], k["total"], k["max_rows"], *rmap, k["labels"],
                                         k["params"], k["opt"], k["loss_each"], k["loss"], k["ws"], k["ws_bytes"], None)


@pytest.mark.parametrize("entry", ENTRIES)
def test_invalid_arguments_are_refused_first(entry):
    A = _Args()
    for kw in ({"feats": None}, {"offsets": None}, {"labels": None}, {"params": None}, {"opt": None}, {"loss_each": None},
               {"loss": None}, {"ws": None}, {"n_bags": 0}, {"n_bags": -2}, {"total": 0}, {"total": 2}, {"max_rows": 0},
               {"max_rows": 41}):
        assert A.call(entry, **kw) == INVALID, kw
    # INVALID wins over everything behind it: a misaligned, short workspace and C = 65 in the same call
    p = ctypes.c_void_p
    assert _Args(step=0).call(entry, ws=p(A.a + 16), ws_bytes=16) == INVALID            # opt->step <= 0
    assert _Args(step=0, C=65).call(entry, ws_bytes=16) == INVALID
    assert _Args(step=-3).call(entry) == INVALID
    assert _Args(Kv=32).call(entry, ws=p(A.a + 16), ws_bytes=16) == INVALID             # v is Identity: Kv == K
    assert _Args(Kv=32, C=65).call(entry) == INVALID
    B = _Args()
    B.params.fcc_b = None
    assert B.call(entry, ws_bytes=16) == INVALID
    B = _Args()
    B.m[2] = None                                                                       # a moment of a live tensor
    assert B.call(entry, ws_bytes=16) == INVALID
    B = _Args(nonlinear=0)                                                              # the one-layer query has no q2_*
    B.params.q2_w = None; B.params.q2_b = None; B.m[4] = None; B.v[5] = None
    assert B.call(entry, ws_bytes=16) == WORKSPACE


@pytest.mark.parametrize("entry", ENTRIES)
def test_refusal_order_behind_invalid(entry):
    p = ctypes.c_void_p
    A = _Args()
    # UNSUPPORTED before ALIGN and WORKSPACE
    assert _Args(C=65).call(entry, ws=p(A.a + 16), ws_bytes=16) == UNSUPPORTED
    assert _Args(C=64).call(entry, ws_bytes=16) == WORKSPACE
    assert A.call(entry, total=(1 << 30) + 1, max_rows=5, ws=p(A.a + 16)) == UNSUPPORTED
    assert A.call(entry, n_bags=65536, total=1 << 20, ws=p(A.a + 16)) == UNSUPPORTED    # the batched forward's limit
    k20 = _Args(K=20).call(entry, ws=p(A.a + 16), ws_bytes=16)
    assert k20 == (UNSUPPORTED if entry == ENTRIES[1] else ALIGN)                       # K = 20: the bf16 entry only
    assert _Args(K=20).call(ENTRIES[0], ws_bytes=16) == WORKSPACE
    # ALIGN before WORKSPACE: the workspace, the labels, the outputs; the rows (bf16) / the query biases (fp32)
    assert A.call(entry, ws=p(A.a + 16), ws_bytes=16) == ALIGN
    assert A.call(entry, labels=p(A.a + 2), ws_bytes=16) == ALIGN
    assert A.call(entry, loss_each=p(A.a + 1), ws_bytes=16) == ALIGN
    assert A.call(entry, loss=p(A.a + 2), ws_bytes=16) == ALIGN
    if entry == ENTRIES[1]:
        assert A.call(entry, feats=p(A.a + 8), ws_bytes=16) == ALIGN
    else:
        B = _Args()
        B.params.q0_b = B.a + 4
        assert B.call(entry, ws_bytes=16) == ALIGN
        assert A.call(entry, row_map=p(A.a + 4), ws_bytes=16) == ALIGN
    # WORKSPACE last: one byte short of what the query says
    size = getattr(nat.lib(), entry + "_workspace_bytes")(3, 40, 64, 2, 1)
    assert size > 0
    assert A.call(entry, ws_bytes=16) == WORKSPACE
    assert A.call(entry, ws_bytes=size - 1) == WORKSPACE
