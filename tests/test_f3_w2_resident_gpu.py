"""k_attend_f3 at K = 512 with W2's second fp16 plane resident in registers (csrc/agg_f3.h, W2_RES), C = 1 (the shipped c16
weights) and C = 2 (tcga), against the fp64 oracle at the derived bars of tests/agg_precision_cases.py — no tolerance of its own.

Two batches per weight set:
    "four"   bags of 70, 33, 1 and 64 rows: more than one 32-row tile, a partial tile, a one-row bag, a bag change inside a
             workgroup's run.  Alone they are a 32-row-regime call: the bars are those of the route the library reports.
    "batch"  the same four bags in front of 508 bags of 1 .. 33 rows: n_bags = 512 puts the call into the 128-row regime, where
             fp32 bags with a two-layer query and C <= 2 take k_attend_f3.  The route is asserted (a library whose route
             function sends this shape elsewhere skips, saying where); the four bags then cross tiles, bags and workgroup
             runs inside the f3 launch itself.
Every launch runs a second time on a poisoned workspace; both runs meet the bars and agree bit for bit."""
import functools

import numpy as np
import pytest
import torch

import agg_precision_cases as ac
from inputs import make_bag
from util import poison_workspace

pytestmark = pytest.mark.gpu

K = 512
FOUR = (70, 33, 1, 64)
TAIL = (1, 2, 33, 3)                       # lengths of the 508 bags behind the four, in turn
LAYOUT = {"four": FOUR, "batch": FOUR + tuple(TAIL[i % len(TAIL)] for i in range(508))}
SETS = ("c16", "tcga")                     # (K, C) = (512, 1), (512, 2)


@functools.lru_cache(maxsize=None)
def _bag(s, i, n):
    """Bag i (n rows) for weight set s: seeded, at scale 1 / 3 / spread in turn, tie-free as agg_precision_cases.make_case_bag's
    (the top two logits of a class at least 200 bars apart, else the next seed)."""
    seed = 8100 + i + (500000 if s == "tcga" else 0)
    flavour = ac.FLAVOURS[i % 3]
    while True:
        x = make_bag(seed, n, K, 3.0 if flavour == "s3" else 1.0)
        if flavour == "spread":
            f = 10.0 ** np.random.default_rng(seed + 50000).uniform(-1.0, 1.0, (n, 1))
            x = (x * f.astype(np.float32)).astype(np.float32)
        if ac.tie_margin(x, ac.weights(s)) >= 2.0:
            x.setflags(write=False)
            return x
        seed += 100000


@functools.lru_cache(maxsize=None)
def _refs(s, layout, kind):
    """fp64 references and bars, once per (weight set, layout, route kind); the four bags are bags 0 .. 3 of both layouts."""
    return tuple(ac.reference(_bag(s, i, n), ac.weights(s), (kind,)) for i, n in enumerate(LAYOUT[layout]))


def _run(s, layout, want_f3):
    from dsmil_wsi_amd import ops, _native
    L = _native.lib()
    assert ac.dims(s) == (K, 1 if s == "c16" else 2)
    C = ac.dims(s)[1]
    lengths = list(LAYOUT[layout])
    total = sum(lengths)
    route = _native.forward_route(total_rows=total, max_rows=max(lengths), n_bags=len(lengths), K=K, Kv=K, C=C, nonlinear=1,
                                  vals_separate=False, row_map=False, packed_split=L.dsmil_agg_mlp_form() != 0)
    attend = _native.ATTEND[route.attend]
    if want_f3 and attend != "f3":
        pytest.skip(f"dsmil_agg_forward_route sends {len(lengths)} bags / {total} rows at K = {K}, C = {C} to {attend}, not to f3")
    kind = ac.route_kind(attend)
    p = {k: torch.from_numpy(v).cuda() for k, v in ac.weights(s).items()}
    x = torch.from_numpy(np.concatenate([_bag(s, i, n) for i, n in enumerate(lengths)])).cuda()
    runs = []
    for again in (False, True):
        if again:
            poison_workspace(ops)
        runs.append([t.cpu().numpy() for t in ops.agg_forward(x, lengths, p)])
    for a, b in zip(*runs):
        assert np.array_equal(a, b), "two runs of the same call differ"
    refs = _refs(s, layout, kind)
    off = np.concatenate([[0], np.cumsum(lengths)])
    classes, pred, A, B, idx = runs[0]
    worst = dict.fromkeys(ac.STATS, 0.0)
    bad = []
    for b, r in enumerate(refs):
        sl = slice(int(off[b]), int(off[b + 1]))
        ra = ac.ratios((classes[sl], pred[b], A[sl], B[b], idx[b]), r, kind)
        for st in ac.STATS:
            worst[st] = max(worst[st], ra[st])
        if not ra["idx"] or any(not ra[st] <= 1.0 for st in ac.STATS):
            bad.append((b, r.n, ra))
    print(f"{s} {layout} {attend} ({kind}) error / bar: " + ", ".join(f"{st} {worst[st]:.3f}" for st in ac.STATS))
    assert not bad, f"{len(bad)} (bag, rows, error / bar) beyond the {kind} bars, first: {bad[:3]}"


@pytest.mark.parametrize("s", SETS)
def test_four_bags(s):
    _run(s, "four", want_f3=False)


@pytest.mark.parametrize("s", SETS)
def test_four_bags_inside_an_f3_batch(s):
    _run(s, "batch", want_f3=True)
