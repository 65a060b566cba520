"""The arithmetic of k_value_tn_b16 (csrc/agg_value.h) restated in numpy, and the cases of
tests/test_value_bwd_b16_gpu.py shown to be sound without a device:

  * gZ = V > 0 ? g_vals : 0 is cut into three truncated bf16 planes (exact: 3 x 8 significand bits hold an fp32 value), each
    plane is multiplied with the ONE bf16 plane of x (products exact in fp32) and accumulated in fp32, smallest plane first;
    per-range partials (vtn_plan) are added in range order.  That arithmetic meets the bar — bwd_b16_cases.bar, 2e-4 of the
    tensor's max-abs + 2e-5 — on every shape, so the bar is reachable and the kernel is asked for nothing its form cannot give;
  * the mask is torch's threshold_backward select, NaN / inf at masked positions included;
  * the module cases are conclusive: the share of value-layer pre-activations too close to zero for the forward's fp32 sum to
    fix their sign is <= 1e-3 in each (the GPU test's cap is 2e-3).
CPU only."""
import numpy as np
import pytest
import torch

import value_bwd_b16_cases as cs


def _planes(a):
    """The three truncated bf16 planes of an fp32 array (csrc/agg_split.h's split3), as fp32 arrays."""
    a = np.ascontiguousarray(a, np.float32)
    hi = (a.view(np.uint32) & np.uint32(0xFFFF0000)).view(np.float32)
    r1 = a - hi
    mid = (r1.view(np.uint32) & np.uint32(0xFFFF0000)).view(np.float32)
    return hi, mid, r1 - mid


def test_the_three_planes_are_exact():
    rng = np.random.default_rng(0)
    a = (rng.standard_normal(100000) * np.exp(rng.uniform(-20, 20, 100000))).astype(np.float32)
    h, m, l = _planes(a)
    assert np.array_equal(h.astype(np.float64) + m.astype(np.float64) + l.astype(np.float64), a.astype(np.float64))
    for p in (h, m, l):
        assert np.array_equal(cs.round_bf16(p), p)      # each plane is a bf16 value


def _emulate(rows, K, Kv):
    """fp32 accumulation of the three exact plane products per row range, the ranges added in order."""
    x, V, g = cs.make_case(rows, K, Kv)
    gz = cs.masked(V, g)
    S, R = cs.vtn_plan(rows, K, Kv)
    g_w, g_b = np.zeros((Kv, K), np.float32), np.zeros(Kv, np.float32)
    for s in range(S):
        sl = slice(s * R, min(rows, (s + 1) * R))
        acc = np.zeros((Kv, K), np.float32)
        for p in reversed(_planes(gz[sl])):             # smallest plane first
            acc += p.T @ x[sl]                           # (fp32 in, fp32 out: an fp32-accumulated product)
        g_w += acc
        g_b += gz[sl].sum(0, dtype=np.float32)
    return g_w, g_b


@pytest.mark.parametrize("rows,K,Kv", cs.SHAPES)
def test_three_plane_products_in_fp32_meet_the_bar(rows, K, Kv):
    ref_w, ref_b = cs.reference(rows, K, Kv)
    g_w, g_b = _emulate(rows, K, Kv)
    for name, got, ref in (("g_v_w", g_w, ref_w), ("g_v_b", g_b, ref_b)):
        err, lim = cs.max_err(got, ref), cs.bar(ref)
        print(f"{rows}x{K}x{Kv} {name}: err {err:.3e}, bar {lim:.3e}")
        assert err <= lim


def test_shapes_cover_one_and_several_row_ranges():
    plans = {s: cs.vtn_plan(*s) for s in cs.SHAPES}
    assert plans[(64, 64, 64)][0] == 1 and plans[(65, 64, 64)][0] == 2 and plans[(129, 64, 64)][0] == 3
    assert plans[(257, 512, 512)][0] == 5 and plans[(700, 512, 512)][0] == 11 and plans[(300, 1024, 1024)][1] == 128
    assert any(S == 1 for S, _ in plans.values()) and any(S > 1 for S, _ in plans.values())
    assert all(R % 64 == 0 for _, R in plans.values())
    assert any(K > 1024 for _, K, _ in cs.SHAPES) and any(K % 64 and Kv % 128 for _, K, Kv in cs.SHAPES)


def test_workspace_entry_agrees_with_the_restated_plan():
    """The library's own plan, seen through the workspace size: S partials of [Kv, K] and [Kv] floats, each 256-B padded."""
    import dsmil  # noqa: F401  (registers the dsmil_wsi_amd package)
    import dsmil_wsi_amd._native as nat
    al = lambda n: (n + 255) // 256 * 256
    for rows, K, Kv in cs.SHAPES:
        S, _ = cs.vtn_plan(rows, K, Kv)
        assert nat.lib().dsmil_value_backward_bf16_workspace_bytes(rows, K, Kv) == al(S * Kv * K * 4) + al(S * Kv * 4)


def test_mask_is_torchs_threshold_backward_select():
    rng = np.random.default_rng(1)
    V = cs.round_bf16(rng.standard_normal((40, 24)).astype(np.float32))
    V[:, 3] = 0.0
    V[0, :] = 0.0
    V[1, :] = -0.0
    assert np.signbit(V[1]).all() and not V[1].any()
    g = rng.standard_normal(V.shape).astype(np.float32)
    dead = ~(V > 0)
    g[dead] = np.resize(np.array([np.nan, np.inf, -np.inf], np.float32), int(dead.sum()))
    want = torch.ops.aten.threshold_backward(torch.from_numpy(g), torch.from_numpy(V), 0.0).numpy()
    got = cs.masked(V, g)
    assert np.isfinite(got).all() and np.array_equal(got, want)
    assert np.array_equal(got[0], np.zeros(24, np.float32)) and np.array_equal(got[1], np.zeros(24, np.float32))
    g_w, g_b = cs.grads_f64(rng.standard_normal((40, 16)), V, g)
    assert np.isfinite(g_w).all() and np.isfinite(g_b).all() and not g_w[3].any() and g_b[3] == 0.0


@pytest.mark.parametrize("K,N", cs.MODULE_CASES)
def test_module_cases_are_conclusive(K, N):
    p = cs.module_params(cs.module_net(K))
    z, decided = cs.mask_band(cs.module_rows(K, N), p)
    share = 1.0 - float(decided.mean())
    print(f"K={K} N={N}: share of |z_ref| inside the accumulation bar {share:.2e}, live {float((z > 0).mean()):.2f}")
    assert share <= 1e-3
    assert 0.05 <= float((z > 0).mean()) <= 0.95          # the mask is neither empty nor full
