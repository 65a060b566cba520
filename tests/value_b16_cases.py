"""Shapes, seeded operands, fp64 reference and bar of the bf16 value projection, shared by tests/test_value_b16_host.py (the
bar is reachable by the reference arithmetic) and tests/test_value_b16_gpu.py (the kernels meet it)."""
import numpy as np
import torch

from inputs import make_bag

# (rows, K, Kv)
SHAPES = [(1, 64, 64), (37, 64, 64),
          (129, 72, 68),        # K not a multiple of 32, Kv not a multiple of a column tile
          (257, 512, 512), (300, 1024, 1024),
          (65, 1032, 64)]       # K > 1024: the plain kernel


def round_bf16(a):
    """fp32 array -> its bf16 rounding (torch's, round to nearest even) as fp32."""
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(torch.bfloat16).to(torch.float32).numpy()


def make_case(rows, K, Kv, bias_shift=0.0):
    """Rows seeded on the host (make_bag), weights seeded per case as tests/test_value_gpu.py::_make_net draws them
    (orthogonal weight, small random bias): fp32 x [rows, K], v_w [Kv, K], v_b [Kv]."""
    x = make_bag(7000 + rows + K, rows, K)
    g = torch.Generator().manual_seed(300 + K + Kv)
    w = torch.empty(Kv, K)
    torch.nn.init.orthogonal_(w, generator=g)
    b = 0.05 * torch.randn(Kv, generator=g) + bias_shift
    return x, w.numpy().copy(), b.numpy().astype(np.float32)


def reference(xb, wb, bb):
    """ref = max(0, x_b w_b^T + b_b) in fp64 and S = |x_b| |w_b|^T + |b_b| of the bf16-rounded operands."""
    x, w, b = (np.asarray(t, np.float64) for t in (xb, wb, bb))
    return np.maximum(x @ w.T + b, 0.0), np.abs(x) @ np.abs(w).T + np.abs(b)


def bar(ref, S, K):
    """|V - ref| <= 2^-8 |ref| + 1.01 K 2^-24 S, elementwise."""
    return 2.0 ** -8 * np.abs(ref) + 1.01 * K * 2.0 ** -24 * S
