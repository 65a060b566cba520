"""The stage bars of tests/agg_bwd_precision_cases.py, checked where no kernel runs:
(a) a numpy restatement of every stage — plane stages as six plane products added window by window in fp32, the others plain fp32
    in the stated order — stays inside the bar on every element of every case up to 400 rows, and so does a plain float32 matmul in
    the plane stages;
(b) mutants of the restatement miss the bar of the stage they touch: by 8 bars and more with one operand of a plane stage on its
    high plane, (1 - Q^2) formed from a bf16 Q, the critical rows' g_q term left out, D without its sum A g_A part; by 2 bars
    and more with one of the six products dropped — (h,l), (l,h) or (m,m) — in each of stages 4a, 6, 7 and 10;
(c) at 65 600 rows the per-range rule of stage 7 holds on one restated range and sees a dropped product there, while the same
    loss over all rows as ONE contraction is printed (it hides under that contraction's own bar);
(d) every case's tables are pinned: lengths, the four-wave arithmetic, R and S of the layout query against the formula.
CPU only; the layout numbers come from the library's host-only query."""
import copy

import numpy as np
import pytest

import agg_bwd_precision_cases as bc
import agg_precision_cases as ac
import dsmil_wsi_amd._native as nat

FACTOR_PLANE, FACTOR_DROP = 8.0, 2.0
DROPS = ((0, 2), (2, 0), (1, 1))                                 # (plane of a, plane of b): (h,l), (l,h), (m,m)
IDS = [c.name for c in bc.HOST_CASES]


@pytest.fixture(scope="module")
def state():
    """{case name: (inputs, the restatement's values)}: made once per case, read by every check below and never changed."""
    cache = {}

    def get(c):
        if c.name not in cache:
            i, _ = bc.host_inputs(c)
            cache[c.name] = (i, bc.emulate(i))
        return cache[c.name]
    return get


def _name(p):
    return "(" + ",".join(bc.PLANE_NAME[k] for k in p) + ")"


def _flat(res):
    return {f"{st}.{k}": v for st, r in res.items() for k, v in r.items()}


@pytest.mark.parametrize("c", bc.HOST_CASES, ids=IDS)
def test_restatement_meets_every_stage_bar(c, state):
    i, d = state(c)
    res = _flat(bc.check_all(i, d))
    print(f"{c.name} six-product restatement, error / bar: " + ", ".join(f"{k} {v:.3f}" for k, v in res.items()))
    assert all(v <= 1.0 for v in res.values()), res
    dp = bc.emulate(i, plain=True)
    resp = {f"{st}.{k}": v for st in bc.PLANE_STAGES if st in bc.case_stages(c) for k, v in bc.CHECKS[st](i, dp).items()}
    print(f"{c.name} plain float32 matmul, error / bar: " + ", ".join(f"{k} {v:.3f}" for k, v in resp.items()))
    assert all(v <= 1.0 for v in resp.values()), resp


def _plane_mutants(i, d):
    """(label, stage, output, mm6 keywords, contraction length) of every plane-stage mutant the case has."""
    out = []
    stages = bc.case_stages(i.case)
    rows_min = min(bc.range_rows(i, s)[1] - bc.range_rows(i, s)[0] for s in range(i.S))

    def both(stage, key, mk, klen):
        for kw in (dict(hi_a=True), dict(hi_b=True)):
            out.append((f"{stage}.{key} {'a' if 'hi_a' in kw else 'b'} on its high plane", stage, key, mk(kw), klen, FACTOR_PLANE))
        for p in DROPS:
            out.append((f"{stage}.{key} without {_name(p)}", stage, key, mk(dict(drop=p)), klen, FACTOR_DROP))
    if i.nonlinear:
        both("4a", "H", lambda kw: ("layer1", kw), i.K)
        both("4a", "Q", lambda kw: ("layer2", kw), bc.QD)
        both("6", "gH", lambda kw: kw, bc.QD)
        both("7", "part1", lambda kw: ("part1", kw), rows_min)
    else:
        both("4a", "Q", lambda kw: ("layer1", kw), i.K)
    both("7", "part0", lambda kw: ("part0", kw), rows_min)
    if "10" in stages:
        both("10", "g_feats", lambda kw: kw, bc.QD)
    return out


@pytest.mark.parametrize("c", bc.HOST_CASES, ids=IDS)
def test_mutants_miss_the_bar_of_their_stage(c, state):
    i, d = state(c)
    lines, bad = [], []
    for label, stage, key, mut, klen, factor in _plane_mutants(i, d):
        if stage == "10" and i.N == 1:
            # One row: A == 1 and gA + g_A - D cancels to its own roundings (softmax over one row is constant), so gs, gz2 and
            # gH are rounding noise and the contraction's share of g_x lies under the roundings of the class tail: nothing
            # a bar on g_x could see.  Stages 4a, 6 and 7 still see every mutant at one row.
            assert np.abs(d["gs"]).max() <= 4 * bc.U * np.abs(d["gA"].astype(np.float64) + i.g_A).max()
            continue
        dm = copy.copy(d)
        bc.EMUS[stage](i, dm, mut)
        r = bc.CHECKS[stage](i, dm)[key]
        lines.append(f"{label} {r:.1f}")
        if not r >= factor:
            bad.append((label, r, factor))
    for label, stage, key, mut in (("(1 - Q^2) from bf16 Q", "5", "gz2", "Q_bf16"), ("g_q left out", "5", "gz2", "no_gq"),
                                   ("D without sum A g_A", "1", "D", "D_without_AgA")):
        if mut == "Q_bf16" and not i.nonlinear:
            continue
        dm = copy.copy(d)
        bc.EMUS[stage](i, dm, mut)
        r = bc.CHECKS[stage](i, dm)[key]
        lines.append(f"{label} {r:.3g}")
        if not r >= FACTOR_PLANE:
            bad.append((label, r, FACTOR_PLANE))
    print(f"{c.name} mutants, error / bar: " + "; ".join(lines))
    assert not bad, bad


def test_stage7_is_a_per_range_rule_at_65600_rows():
    """One 704-row range of the 65 600-row case, restated: inside the bar, and a dropped product is seen there; the same loss
    over ALL rows as one contraction is printed against that contraction's bar (it is the reason the partials are checked)."""
    c = bc.BY_NAME["w4dma_K128_65600"]
    i, lay = bc.host_inputs(c)
    assert (i.R, i.S) == (704, 94)
    d = {}
    for st in ("1", "2", "3", "4a", "4b", "5", "6"):
        bc.EMUS[st](i, d)
    s = 40
    r0, r1 = bc.range_rows(i, s)
    a, x = np.ascontiguousarray(d["gH"][r0:r1].T), np.ascontiguousarray(i.x[r0:r1].T)
    ref, det, r2 = bc.plane_ref(a, x)
    bar = bc.plane_bar(det, r2)
    ok = bc.ratio(bc.mm6(a, x), ref, bar)
    drops = {_name(p): bc.ratio(bc.mm6(a, x, drop=p), ref, bar) for p in DROPS}
    hi = bc.ratio(bc.mm6(a, x, hi_b=True), ref, bar)
    # all rows as one contraction: the kept products in fp64 (no rounding at all), one product left out, against the whole-N bar
    aN, xN = np.ascontiguousarray(d["gH"].T), np.ascontiguousarray(i.x.T)
    refN, detN, r2N = bc.plane_ref(aN, xN)
    pa, pb = bc.planes(aN), bc.planes(xN)
    whole = {_name(p): float((np.abs(pa[p[0]] @ pb[p[1]].T) / bc.plane_bar(detN, r2N)).max()) for p in DROPS}
    print(f"65 600 rows, range {s} ({r1 - r0} rows), error / bar: restated {ok:.3f}; x on its high plane {hi:.0f}; dropped " +
          ", ".join(f"{k} {v:.1f}" for k, v in drops.items()) + "; the same drop over all rows as one contraction: " +
          ", ".join(f"{k} {v:.2f}" for k, v in whole.items()))
    assert ok <= 1.0
    assert hi >= FACTOR_PLANE and all(v >= FACTOR_DROP for v in drops.values()), (hi, drops)


def _formula(N, K, nonlinear):
    """bwd_layout's R and S, tn_rows and the 32-row tiles, restated."""
    nslab = -(-K // 64) + (2 if nonlinear else 0)
    st = min(max(384 // nslab, 1), 256)
    R = max(((-(-N // st)) + 32) // 64 * 64, 64)
    small = max(-(-(-(-N // 256)) // 32) * 32, 128)
    return R, -(-N // R), small, -(-N // small), -(-N // 32)


def test_case_tables():
    assert [b[0] for b in bc.BATCH_BAGS] == [1, 31, 33, 64, 65, 400, 17]
    assert [(n, f) for n, f, _ in bc.BATCH_BAGS[:6]] == ac.SMALL[:6]
    assert len(bc.CASES) == len(bc.BY_NAME) == 4 * 7 + 9
    assert {c.s for c in bc.CASES if c.name.startswith("hs_")} == {(512, 2), (128, 1), (1024, 2), (256, 5)}
    assert [c.name for c in bc.CASES if c.gx] == [f"hs_K512_C2_{n}{f}" for n, f in ac.SMALL] + ["bags_K512_C2"]
    assert 65600 // 128 >= 512 and 65600 == 512 * 128 + 64 and 65599 // 128 < 512 + 1       # 512 full 128-row tiles and a 64-row one
    assert ac.dims("linq") == (64, 3) and "q2_w" not in ac.weights("linq")
    for c in bc.CASES:
        x, lengths = bc.case_rows(c.name)
        K, C = ac.dims(c.s)
        N, nb = len(x), (0 if c.entry == "one" else len(lengths))
        assert x.shape == (N, K) and sum(lengths) == N and list(lengths) == [b[0] for b in c.bags]
        lay = nat.backward_layout(nb, N, K, K, C, int(c.nonlinear), int(not c.misalign), 1)
        assert nat.BWD_TILE[lay.tile] == c.tile, (c.name, lay.tile)
        assert (lay.R, lay.S, lay.small_rows, lay.splits, lay.T32) == _formula(N, K, c.nonlinear), c.name
        assert lay.S * lay.R >= N > (lay.S - 1) * lay.R
        if c.sample:
            i_rows = 2 + 512
            assert (lay.R, lay.S) == (704, 94) and i_rows < N
