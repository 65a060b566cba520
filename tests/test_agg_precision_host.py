"""The bars of tests/agg_precision_cases.py, checked where no kernel runs: (1) a plain fp32 numpy evaluation of the chain
(fast_tanh restated) stays inside every bar of both route kinds, (2) every one-plane variant of the fp64 chain — x, W1, H or W2
rounded once to fp16, H to bf16, the value rows to fp16, x to fp16 in the instance logits — lies at least 8 bars away on the
statistic it touches, whichever kind's bar is asked, (3) every bag the GPU test sends is tie-free: the reference's top two
instance logits of a class are at least 100 classes bars apart, so the critical index is exact and no bag is ever left out.
A case is one weight set with its bags of the 32-row regime (agg_precision_cases.SMALL): its statistic is the worst bag's, as
in the GPU test, where the case is one launch.  CPU only."""
import numpy as np
import pytest

import agg_precision_cases as ac

BATCH_SETS = [(128, 1), (512, 1), (512, 2), (384, 2), (256, 5), "tcga"]     # the sets tests/test_agg_precision_gpu.py batches
FACTOR = 8.0


def test_case_tables():
    assert len(ac.BATCH) == 436 and sum(n for n, _ in ac.BATCH) == 11968
    assert sum(n for n, _ in ac.BATCH) / 128 + len(ac.BATCH) >= 512               # the 128-row regime (tests/test_route_cabi.py)
    assert sorted({n for n, _ in ac.BATCH}) == sorted(ac.SHORT + [400]) and [n for n, _ in ac.BATCH].count(400) == 4
    assert {f for _, f in ac.BATCH} == {f for _, f in ac.SMALL} == set(ac.FLAVOURS)
    assert [n for n, _ in ac.SMALL] == [1, 31, 33, 64, 65, 400, 400]
    assert "c16" not in ac.SETS and ac.dims("tcga") == (512, 2)


def test_fast_tanh_restated_meets_its_bound():
    """b_tanh of the docstring against the fp32 restatement (numpy's exp2 and division are within the 1 ulp granted to v_exp_f32
    and v_rcp_f32), over the arguments the hidden layer produces and far into both saturations."""
    z = np.concatenate([np.linspace(-12, 12, 200001), np.linspace(-1e-3, 1e-3, 20001), [-100.0, 100.0, 0.0]]).astype(np.float32)
    q = np.tanh(z.astype(np.float64))
    bound = ac.U * ((2 * np.abs(z) + 1) * (1 - q * q) + 3 * (1 - q) + 1)
    err = np.abs(ac.fast_tanh32(z).astype(np.float64) - q)
    print(f"fast_tanh restated: worst error / bound {float((err / bound).max()):.3f}, worst error {float(err.max()):.2e}")
    assert np.all(err <= bound)
    assert float(err[np.abs(z) < 1e-3].max()) <= 5 * ac.U          # "a few u of 1.0" near 0, not a few u of tanh z


def test_cuts_are_the_kernels():
    """The two cuts as the docstring states them: fp16 planes hold a row-scaled value to 2 u (normal low plane), the dropped
    product is below 4 u |x w|; the bf16 three-plane cut is exact and drops less than 2^-20 (1 + 2^-8) |x w|."""
    rng = np.random.default_rng(7)
    x = (rng.standard_normal((64, 256)) * 10.0 ** rng.uniform(-1, 1, (64, 1))).astype(np.float32)
    sc = ac.f2_scale(np.abs(x).max(axis=1, keepdims=True))
    assert np.all(np.abs(x).max(axis=1, keepdims=True) * sc >= 2.0 ** 13) and np.all(np.abs(x).max(axis=1, keepdims=True) * sc < 2.0 ** 14)
    r, h1 = ac.cut_f16x2(x, sc)
    ax = np.abs(x).astype(np.float64)
    assert np.all(np.abs(r) <= np.maximum(2 * ac.U * ax, 2.0 ** -25 / sc))
    assert np.all(np.abs(h1) <= 2.0 ** -11 * (1 + 2.0 ** -10) * ax + 2.0 ** -25 / sc)
    m, lo = ac.cut_bf16x3(x)
    assert np.all(np.abs(m) < 2.0 ** -7 * ax + 1e-300) and np.all(np.abs(lo) < 2.0 ** -14 * ax + 1e-300)
    h = x.astype(np.float64) - m - lo
    assert np.array_equal(h.astype(np.float32).view(np.uint32) & 0xFFFF, np.zeros(x.shape, np.uint32))     # the high plane is a bf16 value


@pytest.mark.parametrize("s", ac.SETS, ids=ac.set_name)
def test_plain_fp32_meets_every_bar(s):
    w = ac.weights(s)
    worst = {kind: dict.fromkeys(ac.STATS, 0.0) for kind in ac.KINDS}
    for x, r in ac.small_case(s):
        got = ac.chain32(x, w)
        for kind in ac.KINDS:
            ra = ac.ratios(got, r, kind)
            assert ra["idx"], (ac.set_name(s), r.n)
            for st in ac.STATS:
                worst[kind][st] = max(worst[kind][st], ra[st])
    for kind in ac.KINDS:
        print(f"{ac.set_name(s)} fp32 numpy, error / {kind} bar: " + ", ".join(f"{st} {worst[kind][st]:.3f}" for st in ac.STATS))
        for st in ac.STATS:
            assert worst[kind][st] <= 1.0, (ac.set_name(s), kind, st, worst[kind][st])


@pytest.mark.parametrize("s", ac.SETS, ids=ac.set_name)
def test_one_plane_variants_are_8_bars_away(s):
    w = ac.weights(s)
    lines = []
    for v, (_, _, st) in ac.VARIANTS.items():
        best = dict.fromkeys(ac.KINDS, 0.0)
        for x, r in ac.small_case(s):
            got = ac.chain64(x, w, v)
            for kind in ac.KINDS:
                best[kind] = max(best[kind], ac.ratios(got, r, kind)[st])
        lines.append(f"{v} ({st}) " + " / ".join(f"{best[kind]:.1f}" for kind in ac.KINDS))
        for kind in ac.KINDS:
            assert best[kind] >= FACTOR, (ac.set_name(s), v, kind, best[kind])
    print(f"{ac.set_name(s)} one-plane variants, error / bar ({' / '.join(ac.KINDS)}): " + "; ".join(lines))


@pytest.mark.parametrize("s", ac.SETS, ids=ac.set_name)
def test_cases_are_tie_free(s):
    w = ac.weights(s)
    layouts = [("small", len(ac.SMALL))] + ([("batch", len(ac.BATCH))] if s in BATCH_SETS else [])
    for name, count in layouts:
        for i in range(count):
            assert ac.tie_margin(ac.make_case_bag(s, name, i), w) >= 1.0, (ac.set_name(s), name, i)


def test_batch_sample_in_plain_fp32():
    """The batch's bags are short (1 .. 47 rows) with four of 400: one run of the short lengths and one long bag per flavour, at
    one weight set, through the same fp32 evaluation — the bars do not depend on a bag being long."""
    s = (512, 2)
    w = ac.weights(s)
    for i in list(range(24)) + [i for i, (n, _) in enumerate(ac.BATCH) if n == 400]:
        x = ac.make_case_bag(s, "batch", i)
        r = ac.reference(x, w)
        got = ac.chain32(x, w)
        for kind in ac.KINDS:
            ra = ac.ratios(got, r, kind)
            assert ra["idx"] and all(ra[st] <= 1.0 for st in ac.STATS), (i, kind, ra)
