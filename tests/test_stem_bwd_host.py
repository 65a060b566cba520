"""The bars of tests/stem_bwd_cases.py are reachable and sharp, without a device: a numpy emulation of the stated arithmetic (the
gather in window row-major order, fp32 element operations, serial runs, a fixed tree, partials in chunk order) meets every bar
on every case and is bit-exact on the EXACT cases; the mutants — the last winner on ties, no ReLU mask, the windows at
2 o .. 2 o + 2, an odd pixel collecting only its first window, the x^ mean(q x^) term dropped, mean q dropped — are not.  The
closed form is the fp64 autograd gradient, the gather is the scatter, and the seeds of the stem and model checks keep their
margins.  CPU only."""
import numpy as np
import pytest

import stem_bwd_cases as sc


def test_the_closed_form_is_the_fp64_autograd_gradient():
    for shape in ((2, 9, 7, 8), (1, 8, 8, 4), (2, 1, 5, 4)):
        err = sc.autograd_check(*shape)
        print(f"{shape}: closed form against fp64 autograd {err:.3e}")
        assert err <= 1e-12


@pytest.mark.parametrize("name", [c[0] for c in sc.CASES])
def test_the_gather_is_the_scatter(name):
    """What a pixel collects from its (at most four) windows is what the windows that name it send: the gather's geometry."""
    inp = sc.case(name)
    _, B, H1, W1, C, _ = sc.BY_NAME[name]
    g64 = sc.scatter(inp["g"], inp["win"], H1, W1)[0]
    g32 = sc.gather32(inp["g"], inp["win"], H1, W1)
    assert np.abs(g32 - g64).max() <= 3 * sc.U32 * np.abs(g64).max()
    assert np.array_equal(g32 != 0, g64 != 0) or H1 * W1 == 1


@pytest.mark.parametrize("name", [c[0] for c in sc.CASES])
def test_the_emulation_meets_the_bar(name):
    _, B, H1, W1, C, _ = sc.BY_NAME[name]
    assert sc.PLANS[name][:6] == sc.plan_of(B, H1, W1, C)                     # the emulation's order is the pinned plan's
    inp = sc.case(name)
    got = sc.emulate(inp, chunk=sc.PLANS[name][2], win=inp["win"])
    wst = sc.worst_ratio(got, sc.expected(name))
    print(f"{name}: worst err / bar {wst:.4f}")
    assert wst <= 1
    if H1 * W1 == 1:
        assert not got.any()
    else:
        assert got.any() and not got[0, :, :, sc.MASKED_CH].any()              # the fully masked channel: exact zeros


@pytest.mark.parametrize("name", [c[0] for c in sc.EXACT_CASES])
def test_the_emulation_is_exact_on_the_exact_cases(name):
    inp, ref = sc.exact_case(name)
    got = sc.emulate(inp, win=inp["win"])
    assert np.array_equal(got.astype(np.float64), ref) and np.any(ref != 0)
    assert np.array_equal(sc.emulate(inp).astype(np.float64), ref)             # the rule applied by the emulation itself


@pytest.mark.parametrize("mutant", sc.MUTANTS)
def test_the_checks_see_the_mutants(mutant):
    """Each mutant misses the bar on every random case with more than one pixel — except the tie rule, which random cases (no
    ties, asserted by their builder) cannot see: it misses bit-equality on every EXACT case."""
    if mutant == "last_winner_on_ties":
        for name, *_ in sc.EXACT_CASES:
            inp, ref = sc.exact_case(name)
            assert not np.array_equal(sc.emulate(inp, mutant=mutant).astype(np.float64), ref), name
        return
    seen = 0
    for name, B, H1, W1, C, mag in sc.CASES:
        if H1 * W1 == 1:
            continue
        if mutant in ("first_window_only", "windows_from_2o") and H1 * W1 <= 4:
            continue                                                          # 2 x 2: one window over the whole map either way
        wst = sc.worst_ratio(sc.emulate(sc.case(name), mutant=mutant), sc.expected(name))
        assert wst > 1, (name, wst)
        seen += 1
    assert seen >= 5


def test_zero_cases_give_exact_zeros():
    for name in ("p_5x7", "p_16x17", "p_27x26"):
        inp = dict(sc.case(name), g=np.zeros_like(sc.case(name)["g"]))
        assert not sc.emulate(inp).any() and not sc.closed_form(inp)[0].any()
        assert not sc.expected(name)[0][0, :, :, sc.MASKED_CH].any()           # the fully masked channel of the reference


def test_the_seeds_of_the_stem_and_model_checks_keep_their_margins():
    for name, *_ in sc.STEMS:
        sc.stem_inputs(name)                                                  # asserts its margin
    assert sc.model_stem_margin(sc.MODEL_SEED) >= sc.MARGIN
