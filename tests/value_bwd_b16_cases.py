"""Shapes, seeded operands, fp64 reference and bar of the value layer's parameter gradients on bf16-stored rows
(dsmil_value_backward_bf16: k_value_tn_b16, csrc/agg_value.h), shared by tests/test_value_bwd_b16_host.py (the bar is
reachable by the kernel's arithmetic; the mask is torch's select; the module cases are conclusive) and
tests/test_value_bwd_b16_gpu.py (the kernel and the modules meet the bar).

    gZ = V > 0 ? g_vals : 0        g_v_w [Kv, K] = gZ^T x        g_v_b [Kv] = colsum gZ          (dsmil.py:35-39 behind g_vals)

Operands: x, v_w, v_b of value_b16_cases.make_case rounded to bf16; V = the bf16 rounding of the fp64 max(0, x_b w_b^T +
b_b); g_vals = default_rng(seed).standard_normal, fp32.  Reference: the two contractions in fp64.  Bar: the backward's own in
this project, bwd_b16_cases.bar — 2e-4 of the tensor's max-abs + 2e-5."""
import functools

import numpy as np
import torch

import value_b16_cases as vc
from bwd_b16_cases import bar, max_err, round_bf16   # noqa: F401  (the GPU and host tests take them from here)
from inputs import make_bag

# (rows, K, Kv) and what each can break
SHAPES = [(1, 64, 64),                         # a single row
          (31, 64, 64), (33, 64, 64),          # the 32-row step edge
          (64, 64, 64), (65, 64, 64),          # a second row range of one row (S = 2)
          (129, 64, 64),                       # S = 3 with a one-row tail
          (129, 72, 68),                       # partial column slab and partial unit tile
          (257, 512, 512), (700, 512, 512),    # S = 5 and 11, 8 x 4 slabs
          (300, 1024, 1024),                   # R = 128
          (65, 1032, 64)]                      # K past 1024
BITS = [(700, 512, 512), (129, 72, 68)]        # two runs, the same bits
MODULE_CASES = [(K, N) for K in (64, 512) for N in (33, 129, 700)]   # (K, rows of the bag); C = 2
BAND_CAP = 2e-3                                # the share of V's entries a module case may leave undecided (see mask_band)


def vtn_plan(rows, K, Kv):
    """(S, R) of csrc/agg_value.h's vtn_plan restated: S row ranges of R rows (a multiple of 64), ~384 workgroups."""
    nslab = ((K + 63) // 64) * ((Kv + 127) // 128)
    s = max(1, 384 // nslab)
    r = (rows + s - 1) // s
    r = (r + 63) // 64 * 64
    return (rows + r - 1) // r, r


@functools.lru_cache(maxsize=None)
def make_case(rows, K, Kv):
    """(x_b [rows, K], V_b [rows, Kv], g_vals [rows, Kv]): fp32 arrays, the first two exactly representable in bf16."""
    x, w, b = vc.make_case(rows, K, Kv)
    xb, wb, bb = round_bf16(x), round_bf16(w), round_bf16(b)
    V = round_bf16(vc.reference(xb, wb, bb)[0].astype(np.float32))
    g = np.random.default_rng(5000 + rows + K + Kv).standard_normal((rows, Kv)).astype(np.float32)
    for a in (xb, V, g):
        a.setflags(write=False)
    return xb, V, g


def masked(V, g):
    """gZ: a SELECT on V (torch's threshold_backward) — whatever g holds at a masked position, the result there is 0."""
    return np.where(np.asarray(V) > 0, g, np.zeros((), np.asarray(g).dtype))


@functools.lru_cache(maxsize=None)
def reference(rows, K, Kv):
    """fp64 (g_v_w [Kv, K], g_v_b [Kv]) of make_case(rows, K, Kv): computed once, shared, read-only."""
    xb, V, g = make_case(rows, K, Kv)
    out = grads_f64(xb, V, g)
    for a in out:
        a.setflags(write=False)
    return out


def grads_f64(x, V, g_vals):
    gz = masked(V, np.asarray(g_vals, np.float64))
    return gz.T @ np.asarray(x, np.float64), gz.sum(0)


# ---- the module cases ----------------------------------------------------------------------------------------------------------
ORACLE_NAMES = {"i_classifier.fc.0.weight": "fc_w", "i_classifier.fc.0.bias": "fc_b", "b_classifier.q.0.weight": "q0_w",
                "b_classifier.q.0.bias": "q0_b", "b_classifier.q.2.weight": "q2_w", "b_classifier.q.2.bias": "q2_b",
                "b_classifier.v.1.weight": "v_w", "b_classifier.v.1.bias": "v_b",
                "b_classifier.fcc.weight": "fcc_w", "b_classifier.fcc.bias": "fcc_b"}


def module_net(K):
    """MILNet(FCLayer, BClassifier(passing_v=True)), C = 2, fp32 parameters, on the CPU: K = 64 is the `passv` weight set,
    K = 512 is drawn as tests/test_value_b16_gpu.py::_model draws it."""
    from util import build_net
    if K == 64:
        return build_net("passv", "cpu")
    from dsmil_wsi_amd import modules as M
    net = M.MILNet(M.FCLayer(in_size=K, out_size=2),
                   M.BClassifier(input_size=K, output_class=2, dropout_v=0.0, nonlinear=True, passing_v=True)).eval()
    g = torch.Generator().manual_seed(40 + K)
    for m in net.modules():
        if isinstance(m, (torch.nn.Linear, torch.nn.Conv1d)):
            torch.nn.init.orthogonal_(m.weight, generator=g)
            with torch.no_grad():
                m.bias.copy_(0.05 * torch.randn(m.bias.shape, generator=g))
    return net


def module_params(net):
    """The ten parameters under the oracle's names, each rounded to bf16 (what the bf16 path computes with), fp32 arrays."""
    return {ORACLE_NAMES[k]: round_bf16(v.detach().float().cpu().numpy()) for k, v in net.named_parameters()}


def module_rows(K, N):
    """The bag of a module case: fp32, exactly representable in bf16."""
    return round_bf16(make_bag(8400 + K + N, N, K))


def mask_band(x, p):
    """(z_ref, decided) for the value layer of a module case: z_ref = x_b w_b^T + b_b in fp64, and where |z_ref| exceeds the
    bf16 forward's accumulation bar 1.01 K 2^-24 S (value_b16_cases.bar's second term) — there the sign of the device's
    fp32 sum, hence its ReLU mask, is the reference's."""
    x64, w64, b64 = (np.asarray(t, np.float64) for t in (x, p["v_w"], p["v_b"]))
    z = x64 @ w64.T + b64
    S = np.abs(x64) @ np.abs(w64).T + np.abs(b64)
    return z, np.abs(z) > 1.01 * x.shape[1] * 2.0 ** -24 * S
