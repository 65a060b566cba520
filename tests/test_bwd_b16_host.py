"""The reference of the bf16-row backward (tests/bwd_b16_cases.py) on the host: (i) formula_f64 IS the gradient — it equals
fp64 torch autograd of the reference expression when fed the exact forward's A, B; (ii) the kernel bar of
tests/test_bwd_b16_gpu.py is reachable — the same formula in fp32 stays inside it at every case; (iii) the host deviation
of check (g) is what the issue measured (3e-5 .. 1.3e-3 of max-abs for the tanh query, 0 for the linear one).  CPU only."""
import numpy as np
import pytest

import bwd_b16_cases as bc


@pytest.mark.parametrize("tag,N", [c for c in bc.CASES if c[1] <= 700] + [("tcga", 5000)])
def test_formula_is_the_autograd_gradient(tag, N):
    """1e-10 of each tensor's max-abs; the absolute 1e-12 is for gradients that are exactly zero in exact arithmetic (the
    query stream of a one-row bag, whose softmax is constant: fp64 leaves ~1e-14 there, as the kernel bar's 2e-5 does)."""
    x, p, g = bc.make_case(tag, N)
    _, _, nonlinear = bc.variant(tag)
    exact, (_, _, A, B, idx) = bc.autograd_f64(x, p, g, nonlinear)
    got = bc.formula_f64(x, None, p, A, B, idx, g, nonlinear)
    for k, r in exact.items():
        err, scale = bc.max_err(got[k], r), float(np.abs(r).max())
        print(f"{tag} N={N} {k}: err {err:.3e} scale {scale:.3e}")
        assert err <= 1e-10 * scale + 1e-12, (tag, N, k, err, scale)


@pytest.mark.parametrize("tag,N", bc.CASES)
def test_kernel_bar_is_reachable_in_fp32(tag, N):
    """The formula in fp32 (numpy: fp32 operands, fp32 results) against formula_f64, both fed the same fp32 A, B, idx."""
    x, p, g = bc.make_case(tag, N)
    _, _, nonlinear = bc.variant(tag)
    _, _, A, B, idx = bc.forward(x, p, nonlinear, np.float32, round_hidden=True)
    ref = bc.formula_f64(x, None, p, A, B, idx, g, nonlinear)
    got = bc.formula(x, None, p, A, B, idx, g, nonlinear, np.float32)
    for k, r in ref.items():
        err = bc.max_err(got[k], r)
        print(f"{tag} N={N} {k}: err {err:.3e} = {err / bc.bar(r):.4f} of the bar")
        assert err <= bc.bar(r), (tag, N, k, err, bc.bar(r))


@pytest.mark.parametrize("tag,N", bc.HOST_DEV_CASES)
def test_host_deviation_of_the_hidden_rounding(tag, N):
    dev = bc.dev_host(tag, N)
    print(tag, N, {k: f"{v:.2e}" for k, v in dev.items()})
    _, _, nonlinear = bc.variant(tag)
    if not nonlinear:
        assert all(v <= 1e-12 for v in dev.values()), dev      # no hidden layer: nothing is rounded
    else:
        # a rounding of the hidden layer moves A, B — and with them the gradient — by a fraction of a bf16 ulp (2^-8)
        assert 0 < max(dev.values()) < 2.0 ** -8, dev


def test_bag_cache_dtype_and_train_tcga_flag():
    import torch
    import train_tcga as tt
    from dsmil_wsi_amd import training as T
    stacked = torch.arange(30, dtype=torch.float32).reshape(5, 6) / 7
    f32, lab = T.BagCache(torch.device("cpu"), 4).get(stacked)
    b16, lab2 = T.BagCache(torch.device("cpu"), 4, dtype=torch.bfloat16).get(stacked)
    assert f32.dtype == torch.float32 and b16.dtype == torch.bfloat16 and lab.dtype == lab2.dtype == torch.float32
    assert torch.equal(f32, stacked[:, :4]) and torch.equal(b16, stacked[:, :4].to(torch.bfloat16)) and torch.equal(lab, lab2)
    with pytest.raises(ValueError):
        T.BagCache(torch.device("cpu"), 4, dtype=torch.float16)
    p = tt.build_parser()
    assert p.parse_args([]).feats_dtype == "fp32" and p.parse_args(["--feats_dtype", "bf16"]).feats_dtype == "bf16"
    flag = next(a for a in p._actions if "--feats_dtype" in a.option_strings)
    assert "NOT a flag of the reference" in flag.help
    with pytest.raises(SystemExit):
        p.parse_args(["--feats_dtype", "fp16"])
