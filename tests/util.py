"""Helpers shared by the tests: MILNet built from the example weight sets (dsmil-wsi_amd/synthetic.py), the weight sets of the
C > 2 golden file, the tie-safe per-bag parity check and the workspace poison of the GPU tests."""
import os

import numpy as np

import dsmil  # noqa: F401  (registers the package)
from dsmil_wsi_amd.synthetic import VARIANT, build_net, load_weights, state_dict_from_npz  # noqa: F401

GOLDEN_CLASSES = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "agg_golden_classes.npz")


def class_set_weights(z, name):
    """Weight set `name` (e.g. "K64_C5_nl") of tests/golden/agg_golden_classes.npz as fp32 arrays (stored fp16-exact)."""
    pre = f"{name}/w/"
    return {k[len(pre):]: z[k].astype(np.float32) for k in z.files if k.startswith(pre)}


def check_bag(got, b, sl, ref, worst, tag):
    """One bag of a batch output `got` = (classes, pred, A, B, idx) against the oracle's `ref`; returns False when the
    critical instance differs by a near-tie of the fp32 logits (A / B then belong to another instance: not compared)."""
    cls, pred, A, B = [o.cpu().numpy() for o in (got[0][sl], got[1][b:b + 1], got[2][sl], got[3][b:b + 1])]
    idx = got[4][b].cpu().numpy()
    C = cls.shape[1]
    sc_c = max(1.0, float(np.abs(ref[0]).max()))
    np.testing.assert_allclose(cls, ref[0], atol=1e-4 * sc_c, rtol=1e-5, err_msg=f"{tag}: instance logits")
    worst["classes"] = max(worst["classes"], float(np.abs(cls - ref[0]).max() / sc_c))
    if not np.array_equal(idx, ref[4]):
        # tie-safe: the oracle's logits at our index must be its column maxima up to the fp32 rounding of the logits
        gap = ref[0].max(axis=0) - ref[0][idx, np.arange(C)]
        assert np.all(gap <= 4e-6 * sc_c), f"{tag}: critical instance {idx} vs {ref[4]}, logit gap {gap}"
        return False
    sc = max(1.0, float(np.abs(ref[3]).max()))   # B and pred scale with the features
    np.testing.assert_allclose(A, ref[2], atol=1e-6, rtol=1e-3, err_msg=f"{tag}: A")
    np.testing.assert_allclose(A.sum(axis=0, dtype=np.float64), 1.0, atol=1e-5, err_msg=f"{tag}: sum A")
    np.testing.assert_allclose(B, ref[3], atol=1e-4 * sc, rtol=1e-5, err_msg=f"{tag}: B")
    np.testing.assert_allclose(pred, ref[1], atol=1e-4 * sc, rtol=1e-5, err_msg=f"{tag}: pred")
    worst["A"] = max(worst["A"], float((np.abs(A - ref[2]) / (1e-6 + 1e-3 * np.abs(ref[2]))).max()))
    worst["B"] = max(worst["B"], float(np.abs(B - ref[3]).max() / sc))
    worst["pred"] = max(worst["pred"], float(np.abs(pred - ref[1]).max() / sc))
    return True


def poison_workspace(ops):
    """Every word of the native workspace of the current stream (q_max, hand-off flags, tile partials) becomes
    0xFFFFFFFF = NaN / "flag set": a read of anything the CURRENT call has not written shows up as a NaN or, for a
    flag that was not cleared, as a tile that did not wait."""
    if ops._ws_last[0] is not None:
        ops._ws_last[0].fill_(0xFF)
