"""The arithmetic of the bf16 value projection (k_value_proj_b16, csrc/agg_value.h) restated in numpy, and the bar of
tests/test_value_b16_gpu.py shown to be reachable by that arithmetic alone:

    V[n, j] = bf16_rne(max(0, fp32 sum_k x_b[n, k] w_b[j, k] + b_b[j]))

with bf16-rounded operands (their products are exact in fp32), fp32 accumulation in two different k groupings — sequential,
and blocks of 16 summed pairwise (a tree over the blocks) — and round-to-nearest-even to bf16.  Against the fp64 result:

    |V - ref| <= 2^-8 |ref| + 1.01 K 2^-24 S,      S = |x_b| |w_b|^T + |b_b|

(second term: the worst case of an fp32 sum of K terms in any order; first term: the final rounding, 2^-9 relative, doubled
because the accumulation error can carry the fp32 sum across a rounding boundary).  CPU only."""
import numpy as np
import pytest

from value_b16_cases import SHAPES, bar, make_case, reference, round_bf16


def _to_bf16_rne(a):
    """fp32 -> bf16 (round to nearest even), returned as fp32; integer arithmetic, as csrc/agg_common.h's f2bf."""
    u = np.ascontiguousarray(a, np.float32).view(np.uint32).astype(np.uint64)
    u = (u + 0x7FFF + ((u >> 16) & 1)) >> 16 << 16
    return u.astype(np.uint32).view(np.float32)


def test_rounding_helper_is_torchs():
    rng = np.random.default_rng(0)
    a = (rng.standard_normal(100000) * np.exp(rng.uniform(-20, 20, 100000))).astype(np.float32)
    assert np.array_equal(_to_bf16_rne(a), round_bf16(a))


def _sequential(x, w):
    """fp32 sum over k = 0, 1, ... in turn: [rows, Kv]."""
    acc = np.zeros((x.shape[0], w.shape[0]), np.float32)
    for k in range(x.shape[1]):
        acc += x[:, k:k + 1] * w[None, :, k]          # exact products, one fp32 rounding per add
    return acc


def _blocks_pairwise(x, w):
    """fp32 sums of blocks of 16 k (sequential inside a block), the block sums added pairwise."""
    parts = [_sequential(x[:, k:k + 16], w[:, k:k + 16]) for k in range(0, x.shape[1], 16)]
    while len(parts) > 1:
        parts = [parts[i] + parts[i + 1] if i + 1 < len(parts) else parts[i] for i in range(0, len(parts), 2)]
    return parts[0]


@pytest.mark.parametrize("rows,K,Kv", SHAPES)
@pytest.mark.parametrize("grouping", ["sequential", "blocks16_pairwise"])
def test_reference_arithmetic_meets_the_bar(rows, K, Kv, grouping):
    x, w, b = make_case(rows, K, Kv)
    n = min(rows, 48)                                   # (the arithmetic is row by row: 48 rows of each shape)
    xb, wb, bb = round_bf16(x[:n]), round_bf16(w), round_bf16(b)
    acc = (_sequential if grouping == "sequential" else _blocks_pairwise)(xb, wb)
    V = _to_bf16_rne(np.maximum(acc + bb[None, :], np.float32(0)))
    ref, S = reference(xb, wb, bb)
    err = np.abs(V.astype(np.float64) - ref)
    lim = bar(ref, S, K)
    print(f"{grouping} {rows}x{K}x{Kv}: worst err / bar {float((err / lim)[lim > 0].max()):.3f}")
    assert np.all(err <= lim)


def test_negative_bias_case_clamps_a_quarter():
    x, w, b = make_case(257, 512, 512, bias_shift=-1.0)
    ref, _ = reference(round_bf16(x), round_bf16(w), round_bf16(b))
    assert (ref == 0).mean() >= 0.25
