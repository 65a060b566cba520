"""k_attend_f3 on the 16x16x32 MFMA shape (csrc/agg_f3.h): the 16-row halves of a tile are where the fragment and accumulator
layouts of that shape can go wrong, so the batch puts bags of 1, 15, 16, 17, 31, 32, 33 and 47 rows between twelve long ones
(workgroup runs cross the bag boundaries), scales one long bag by 300 and one by 1e-3, and runs the K = 128 .. 512 instantiations
with one and two classes (W2 resident and W2's second plane streamed).  Checked: the fp64 oracle at the bars of
tests/test_agg_gpu.py::test_batch_form_f2_vs_oracle_and_six_product_form, run-to-run bit identity, and agreement with
k_attend_f2 (dsmil_agg_batch_form(1)) at that test's between-form bars."""
import functools

import numpy as np
import pytest
import torch

import agg_oracle as orc
from inputs import make_bag

pytestmark = pytest.mark.gpu

SHAPES = [(128, 1), (512, 1), (512, 2), (384, 2)]
SHORT = [1, 15, 16, 17, 31, 32, 33, 47]
LENGTHS = [n for s in SHORT for n in (5300, s)] + [5300] * 4          # twelve long bags, the short ones between them
SCALES = {2: 300.0, 4: 1e-3}                                            # bag index -> feature scale
ORACLE_BAGS = [i for i, n in enumerate(LENGTHS) if n < 100] + [2, 4]   # every short bag, the two scaled long ones


def _weights(K, C):
    rng = np.random.default_rng(1600 + K + C)
    w = {"fc_w": rng.normal(0, 0.05, (C, K)), "fc_b": rng.normal(0, 0.05, (C,)), "q0_w": rng.normal(0, 0.06, (128, K)),
         "q0_b": rng.normal(0, 0.05, (128,)), "q2_w": rng.normal(0, 0.08, (128, 128)), "q2_b": rng.normal(0, 0.05, (128,)),
         "fcc_w": rng.normal(0, 0.05, (C, C, K)), "fcc_b": rng.normal(0, 0.05, (C,))}
    return {k: v.astype(np.float32) for k, v in w.items()}


@functools.lru_cache(maxsize=None)
def _case(K, C):
    """The batch through form 2 twice and through form 1 once, and the oracle on ORACLE_BAGS (computed once per shape)."""
    from dsmil_wsi_amd import ops, _native
    L = _native.lib()
    assert len(LENGTHS) == 20 and LENGTHS.count(5300) == 12
    assert L.dsmil_agg_tile_rows(len(LENGTHS), sum(LENGTHS)) == 128
    w = _weights(K, C)
    p = {k: torch.from_numpy(v).cuda() for k, v in w.items()}
    bags = [make_bag(1600 + K + i, n, K) * np.float32(SCALES.get(i, 1.0)) for i, n in enumerate(LENGTHS)]
    x = torch.from_numpy(np.concatenate(bags)).cuda()
    prev = L.dsmil_agg_batch_form(2)
    try:
        route = _native.forward_route(total_rows=sum(LENGTHS), max_rows=max(LENGTHS), n_bags=len(LENGTHS), K=K, Kv=K, C=C,
                                      nonlinear=1, packed_split=True)
        assert _native.ATTEND[route.attend] == "f3"
        run1 = [t.cpu().numpy() for t in ops.agg_forward(x, LENGTHS, p)]
        run2 = [t.cpu().numpy() for t in ops.agg_forward(x, LENGTHS, p)]
        L.dsmil_agg_batch_form(1)
        f2 = [t.cpu().numpy() for t in ops.agg_forward(x, LENGTHS, p)]
    finally:
        L.dsmil_agg_batch_form(prev)
    ref = {b: orc.milnet_forward(bags[b], w, dtype="f64") for b in ORACLE_BAGS}
    return run1, run2, f2, ref


def _slices():
    off = np.concatenate([[0], np.cumsum(LENGTHS)])
    return [slice(int(off[b]), int(off[b + 1])) for b in range(len(LENGTHS))]


@pytest.mark.parametrize("K,C", SHAPES)
def test_f3_shape_vs_oracle(K, C):
    got, _, _, ref = _case(K, C)
    sl = _slices()
    for b in ORACLE_BAGS:
        r = ref[b]
        sc = max(1.0, float(np.abs(r[3]).max()))   # B and pred scale with the features
        np.testing.assert_allclose(got[0][sl[b]], r[0], atol=1e-4 * max(1.0, float(np.abs(r[0]).max())), rtol=1e-5, err_msg=f"classes, bag {b}")
        np.testing.assert_allclose(got[2][sl[b]], r[2], atol=1e-6, rtol=1e-3, err_msg=f"A, bag {b}")
        np.testing.assert_allclose(got[3][b:b + 1], r[3], atol=1e-4 * sc, rtol=1e-5, err_msg=f"B, bag {b}")
        np.testing.assert_allclose(got[1][b:b + 1], r[1], atol=1e-4 * sc, rtol=1e-5, err_msg=f"pred, bag {b}")
        assert np.array_equal(got[4][b], r[4]), f"idx, bag {b}"


@pytest.mark.parametrize("K,C", SHAPES)
def test_f3_shape_two_runs_bit_identical(K, C):
    run1, run2, _, _ = _case(K, C)
    for name, a, b in zip(("classes", "pred", "A", "B", "idx"), run1, run2):
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), name


@pytest.mark.parametrize("K,C", SHAPES)
def test_f3_shape_vs_k_attend_f2(K, C):
    got, _, f2, _ = _case(K, C)
    sl = _slices()
    assert np.array_equal(got[0], f2[0]) and np.array_equal(got[4], f2[4])   # the logits pass is the same launch
    for b in range(len(LENGTHS)):
        sc = max(1.0, float(np.abs(f2[3][b]).max()))
        np.testing.assert_allclose(got[2][sl[b]], f2[2][sl[b]], atol=2e-7, rtol=2e-4, err_msg=f"A, bag {b}")
        np.testing.assert_allclose(got[3][b:b + 1], f2[3][b:b + 1], atol=2e-5 * sc, rtol=1e-5, err_msg=f"B, bag {b}")
        np.testing.assert_allclose(got[1][b:b + 1], f2[1][b:b + 1], atol=2e-5 * sc, rtol=1e-5, err_msg=f"pred, bag {b}")
