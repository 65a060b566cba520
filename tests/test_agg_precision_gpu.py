"""The fp32-feature routes of the aggregator forward (ops.agg_forward -> dsmil_agg_forward_ex) against the fp64 oracle at the
DERIVED bars of tests/agg_precision_cases.py — the bars a kernel that lost an operand plane misses by 8 and more
(tests/test_agg_precision_host.py), where the parity bars of tests/test_agg_gpu.py let it pass.  Per bag and class: the
log-attention error, |sum A - 1|, B, pred, classes (each as error / bar, at most 1) and the exact critical index.

32-row regime (one launch of seven bags of 1 .. 400 rows unless said otherwise):
    k_attend_hs with the critical query inside the launch, and with the k_qmax launch (dsmil_agg_inline_query(0));
    k_query_attend_split register-staged (K = 166); a lone bag at K = 1024; V given as its own tensor at (K, C) = (256, 5).
128-row regime (436 bags of 1 .. 47 rows with four of 400 between them, 11 968 rows: the smallest batch of these lengths with
total_rows / 128 + n_bags >= 512):
    k_attend_f3 (dsmil_agg_batch_form 2), k_attend_f2 (form 1; and by default at C = 5), k_query_attend_split with six plane
    products (form 0), k_attend_f3 through a row map over a larger physical tensor.
The route is asked from the library before every launch (_native.forward_route with the call's own operands) and every launch
runs a second time on a poisoned workspace; both runs meet the bars.  bf16-stored features state another precision and are
tests/test_agg_bf16_gpu.py's."""
import contextlib
import functools

import numpy as np
import pytest
import torch

import agg_precision_cases as ac
from util import poison_workspace

pytestmark = pytest.mark.gpu


@contextlib.contextmanager
def knob(name, value):
    """A run-time knob of the library for the length of the block (None: leave it alone)."""
    from dsmil_wsi_amd import _native
    fn = getattr(_native.lib(), name)
    old = fn(value) if value is not None else None
    try:
        yield
    finally:
        if value is not None:
            fn(old)


@functools.lru_cache(maxsize=None)
def _bags(s, layout, only):
    idxs = range(len(ac.LAYOUTS[layout])) if only is None else [only]
    return tuple(ac.make_case_bag(s, layout, i) for i in idxs)


@functools.lru_cache(maxsize=None)
def _refs(s, layout, only, kind):
    """The fp64 references and bars of the bags, made once per (weight set, layout, route kind) and left unchanged."""
    return tuple(ac.reference(x, ac.weights(s), (kind,)) for x in _bags(s, layout, only))


def _check(s, layout, expect, only=None, batch_form=None, inline_query=None, vals_separate=False, row_map=False):
    from dsmil_wsi_amd import ops, _native
    L = _native.lib()
    w = ac.weights(s)
    K, C = ac.dims(s)
    bags = _bags(s, layout, only)
    lengths = [len(x) for x in bags]
    total = sum(lengths)
    assert L.dsmil_agg_tile_rows(len(lengths), total) == (128 if layout == "batch" else 32)
    p = {k: torch.from_numpy(v).cuda() for k, v in w.items()}
    x_log = np.concatenate(bags)
    rmap = None
    if row_map:     # logical row i lives at physical row rmap[i] of a tensor with 64 more rows, which hold NaN
        rmap = np.random.default_rng(5).permutation(total + 64)[:total].astype(np.int64)
        phys = np.full((total + 64, K), np.nan, np.float32)
        phys[rmap] = x_log
        x = torch.from_numpy(phys).cuda()
    else:
        x = torch.from_numpy(x_log).cuda()
    kw = {}
    if vals_separate:
        kw["vals"] = x.clone()
    if row_map:
        kw["row_map"] = torch.from_numpy(rmap).cuda()
    with knob("dsmil_agg_batch_form", batch_form), knob("dsmil_agg_inline_query", inline_query):
        route = _native.forward_route(total_rows=total, max_rows=max(lengths), n_bags=len(lengths), K=K, Kv=K, C=C, nonlinear=1,
                                      vals_separate=vals_separate, row_map=row_map, packed_split=L.dsmil_agg_mlp_form() != 0)
        got_route = {"attend": _native.ATTEND[route.attend], "qmax": _native.QMAX[route.qmax], "attend_vec": route.attend_vec,
                     "attend_nw": route.attend_nw, "attend_np": route.attend_np, "nw": route.nw}
        assert {k: got_route[k] for k in expect} == expect, got_route
        runs = []
        for again in (False, True):
            if again:
                poison_workspace(ops)
            runs.append([t.cpu().numpy() for t in ops.agg_forward(x, lengths, p, **kw)])
    kind = ac.route_kind(got_route["attend"])
    refs = _refs(s, layout, only, kind)
    off = np.concatenate([[0], np.cumsum(lengths)])
    worst = dict.fromkeys(ac.STATS, 0.0)
    bad = []
    for run, (classes, pred, A, B, idx) in enumerate(runs):
        for b, r in enumerate(refs):
            sl = slice(int(off[b]), int(off[b + 1]))
            ra = ac.ratios((classes[sl], pred[b], A[sl], B[b], idx[b]), r, kind)
            for st in ac.STATS:
                worst[st] = max(worst[st], ra[st])
            if not ra["idx"] or any(not ra[st] <= 1.0 for st in ac.STATS):
                bad.append((run, b, r.n, ra))
    print(f"{ac.set_name(s)} {layout} {got_route['attend']} ({kind}) error / bar: " + ", ".join(f"{st} {worst[st]:.3f}" for st in ac.STATS))
    assert not bad, f"{len(bad)} (run, bag, rows, error / bar) beyond the {kind} bars, first: {bad[:3]}"


HS_SETS = [(128, 1), (512, 1), (512, 2), (384, 2), "tcga"]


@pytest.mark.parametrize("s", HS_SETS, ids=ac.set_name)
def test_hs_inline_query(s):
    _check(s, "small", dict(attend="hs", qmax="inline", nw=1))


def test_hs_with_the_qmax_launch():
    _check((512, 2), "small", dict(attend="hs", qmax="launch", nw=1), inline_query=0)


def test_split_register_staged_k166():
    _check((166, 1), "small", dict(attend="split", attend_vec=1, attend_nw=1, attend_np=6, qmax="launch"))


def test_lone_bag_k1024():
    _check((1024, 2), "small", dict(attend="hs", qmax="inline", nw=1), only=5)


def test_vals_as_their_own_tensor_c5():
    _check((256, 5), "small", dict(attend="hs", nw=1), vals_separate=True)


@pytest.mark.parametrize("s", HS_SETS, ids=ac.set_name)
def test_batch_f3(s):
    _check(s, "batch", dict(attend="f3", nw=4), batch_form=2)


@pytest.mark.parametrize("s", [(128, 1), (512, 2)], ids=ac.set_name)
def test_batch_f2(s):
    _check(s, "batch", dict(attend="f2", nw=4), batch_form=1)


@pytest.mark.parametrize("s", [(384, 2), (512, 2)], ids=ac.set_name)
def test_batch_split_six_products(s):
    _check(s, "batch", dict(attend="split", attend_np=6, attend_nw=4, attend_vec=4), batch_form=0)


def test_batch_f2_by_default_c5():
    from dsmil_wsi_amd import _native
    assert _native.lib().dsmil_agg_batch_form(-1) == 2
    _check((256, 5), "batch", dict(attend="f2", nw=4))


def test_batch_f3_through_a_row_map():
    _check((512, 2), "batch", dict(attend="f3", nw=4), batch_form=2, row_map=True)
