"""The numpy oracle (oracle/agg_oracle.py) at C > 2 against vectors produced by the reference itself
(tests/golden/make_golden.py --classes ran the reference's dsmil.py with seeded orthogonal weights, which the file holds).
Same bars as tests/test_oracle_golden.py.  CPU only."""
import hashlib

import numpy as np
import pytest

import agg_oracle as orc
from inputs import make_bag
from util import GOLDEN_CLASSES, class_set_weights

# (weight set, K, C, nonlinear, N)
FWD_CASES = [("K64_C5_nl", 64, 5, True, 200), ("K166_C4_nl", 166, 4, True, 57), ("K512_C5_nl", 512, 5, True, 300),
             ("K64_C17_nl", 64, 17, True, 120), ("K64_C6_lin", 64, 6, False, 80)]
GRAD_CASES = [("K64_C5_nl", 64, 5, 200), ("K166_C4_nl", 166, 4, 57)]
KEYS = ("fc_w", "fc_b", "q0_w", "q0_b", "q2_w", "q2_b", "fcc_w", "fcc_b")


@pytest.fixture(scope="module")
def gc():
    return np.load(GOLDEN_CLASSES)


def _input(gc, name, K, N):
    x = make_bag(int(gc[f"{name}/seed"]), N, K)
    assert hashlib.sha256(x.tobytes()).hexdigest() == str(gc[f"{name}/x_sha"]), \
        "seeded input stream differs from the one the golden vectors were generated with"
    return x


@pytest.mark.parametrize("ws,K,C,nonlinear,N", FWD_CASES)
def test_forward_matches_reference_many_classes(gc, ws, K, C, nonlinear, N):
    name = f"{ws}/fwd_N{N}"
    p = class_set_weights(gc, ws)
    assert p["fc_w"].shape == (C, K) and p["fcc_w"].shape == (C, C, K) and ("q2_w" in p) == nonlinear
    x = _input(gc, name, K, N)
    classes, pred, A, B, idx = orc.milnet_forward(x, p, nonlinear=nonlinear)
    ref_cls = gc[f"{name}/classes"]
    assert ref_cls.shape == (N, C)
    np.testing.assert_allclose(classes, ref_cls, atol=2e-5, rtol=1e-5)
    assert np.array_equal(ref_cls[idx, np.arange(C)], ref_cls.max(axis=0))
    assert np.array_equal(idx, gc[f"{name}/idx"])
    np.testing.assert_allclose(pred, gc[f"{name}/pred"], atol=2e-5, rtol=1e-5)
    np.testing.assert_allclose(A, gc[f"{name}/A"], atol=1e-6, rtol=1e-4)
    np.testing.assert_allclose(B, gc[f"{name}/B"], atol=2e-5, rtol=1e-5)
    np.testing.assert_allclose(A.sum(axis=0, dtype=np.float64), 1.0, atol=1e-5)


@pytest.mark.parametrize("ws,K,C,N", GRAD_CASES)
def test_gradients_match_reference_autograd_many_classes(gc, ws, K, C, N):
    name = f"{ws}/grad_N{N}"
    p = class_set_weights(gc, ws)
    x = _input(gc, name, K, N)
    label = gc[f"{name}/label"]
    assert label.shape == (C,) and label.sum() == 1.0
    loss, g = orc.train_loss_and_grads(x, label, p, dtype="f64")
    assert abs(loss - float(gc[f"{name}/loss"])) < 2e-6
    for k in KEYS:
        ref = gc[f"{name}/g_{k}"]
        scale = max(1e-6, float(np.abs(ref).max()))
        np.testing.assert_allclose(g[k], ref, atol=2e-5 * scale + 1e-8, rtol=2e-4, err_msg=k)
