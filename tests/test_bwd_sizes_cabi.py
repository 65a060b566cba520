"""The aggregator backward's and training steps' workspace queries answer what they answered before the two launch
sequences got one workspace layout (csrc/agg_bwd.hip: bwd_layout with n_bags == 0 for the one bag, param_sizes for the
steps): callers size and cache their workspaces from these numbers, so a refactor of the host side must not move any of
them.  The expected values in tests/golden/bwd_sizes.json were recorded from the library before that refactor
(tools/bwd_host_check.py sizes).  dsmil_agg_backward_layout (FOR TESTS: where a call leaves its intermediates, and the row tile
of its step 4) answers from the same layout function: its offsets ascend on 256-byte boundaries inside the size the queries
answer, its row ranges cover the rows, and its tile follows the rule the launch sequences state.  Pure host code: no GPU."""
import ctypes
import itertools
import json
import os
import re

import dsmil_wsi_amd._native as nat

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "bwd_sizes.json")
# every branch of the layouts: the 32-row tile count of gqp (31 / 32 / 33), k_tn_split's 64-row ranges (64 / 65),
# k_tn_small's 128-row minimum and its 256 ranges (65535 / 65536), the sizes the benchmarks use (10000, 640000)
ROWS = (1, 31, 32, 33, 64, 65, 65535, 65536, 10000, 640000)
KS = (64, 166, 512, 1024)
KV_OTHER = 96
CS = (1, 2, 4, 5, 16)
N_BAGS = (1, 3, 64)
BAD = (0, -1)


def cases():
    """{query: [argument tuples]} in a fixed order; the fixture holds one answer per tuple."""
    one = [(n, k, kv, c) for n, k, c in itertools.product(ROWS, KS, CS) for kv in (k, KV_OTHER)]
    bags = [(b, n, k, kv, c) for b in N_BAGS for (n, k, kv, c) in one if n >= b]
    step = [(n, k, c, nl) for n, k, c, nl in itertools.product(ROWS, KS, CS, (0, 1))]
    step_bags = [(b, n, k, c, nl) for b in N_BAGS for (n, k, c, nl) in step if n >= b]
    # a zero or negative argument answers 0 (the entries refuse those sizes as invalid); total_rows < n_bags for the steps
    def bad(good):
        return [good[:i] + (v,) + good[i + 1:] for i in range(len(good)) for v in BAD]
    one += bad((1500, 512, 512, 2))
    bags += bad((3, 1500, 512, 512, 2))
    step += [t for t in bad((1500, 512, 2, 1)) if t[3] == 1]            # (nonlinear is a flag: every value is a size)
    step_bags += [t for t in bad((3, 1500, 512, 2, 1)) if t[4] == 1] + [(3, 2, 512, 2, 1), (64, 63, 512, 2, 0)]
    step_bags_b16 = step_bags + [(3, 1500, 166, 2, 1), (1, 33, 516, 2, 1)]   # K % 8 != 0: the bf16 step has no such size
    return {
        "dsmil_agg_backward_workspace_bytes": one,
        "dsmil_agg_backward_rows_workspace_bytes": one,
        "dsmil_agg_backward_bags_workspace_bytes": bags,
        "dsmil_agg_backward_bags_bf16_workspace_bytes": bags,
        "dsmil_agg_train_step_workspace_bytes": step,
        "dsmil_agg_train_step_bags_workspace_bytes": step_bags,
        "dsmil_agg_train_step_bags_bf16_workspace_bytes": step_bags_b16,
    }


def query():
    """Every size the C-ABI answers for cases(), as the JSON-able dict the fixture holds."""
    L = nat.lib()
    return {name: [int(getattr(L, name)(*t)) for t in args] for name, args in cases().items()}


def test_backward_size_queries_equal_the_recorded_values():
    with open(GOLDEN) as f:
        want = json.load(f)
    got, args = query(), cases()
    assert set(got) == set(want)
    for name in want:
        assert len(want[name]) == len(args[name]), name
        for t, g, w in zip(args[name], got[name], want[name]):
            assert g == w, (name, t, g, w)


def test_fixture_brackets_the_layout_branches():
    """The table is not degenerate: refused sizes answer 0, accepted ones do not, a batch of one bag is larger than the
    one-bag call (idle tile slots, the row -> bag table), and the bf16 batch answers what the fp32 batch does."""
    with open(GOLDEN) as f:
        want = json.load(f)
    args = cases()
    for name in want:
        for t, w in zip(args[name], want[name]):
            refused = min(t[:-1] if "train_step" in name else t) <= 0 or \
                ("bags" in name and t[1] < t[0]) or ("step_bags_bf16" in name and t[2] % 8 != 0)
            assert (w == 0) == refused, (name, t, w)
    one = dict(zip(args["dsmil_agg_backward_workspace_bytes"], want["dsmil_agg_backward_workspace_bytes"]))
    bags = dict(zip(args["dsmil_agg_backward_bags_workspace_bytes"], want["dsmil_agg_backward_bags_workspace_bytes"]))
    for (b, n, k, kv, c), w in bags.items():
        if b == 1 and w:
            assert w > one[(n, k, kv, c)], (n, k, kv, c)
    assert want["dsmil_agg_backward_bags_bf16_workspace_bytes"] == want["dsmil_agg_backward_bags_workspace_bytes"]
    assert want["dsmil_agg_backward_rows_workspace_bytes"] == want["dsmil_agg_backward_workspace_bytes"]


ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_layout_query_is_declared_exported_and_bound():
    text = open(os.path.join(ROOT, "include", "dsmil_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    name = "dsmil_agg_backward_layout"
    assert re.search(r"\b%s\s*\(" % name, src), f"{name} is not declared in include/dsmil_hip.h"
    assert hasattr(ctypes.CDLL(nat.LIB_PATH), name) and name in nat.SIGNATURES
    assert int(re.search(r"#define DSMIL_ABI_VERSION (\d+)", text).group(1)) == 6 and nat.lib().dsmil_abi_version() == 6
    block = text[:text.index("#define DSMIL_BWD_TILE_HS")]
    assert "FOR TESTS" in block[block.rindex("/*"):]
    # the struct as the header declares it: seventeen offsets and the total (uint64), T32 (int64), six int32
    assert ctypes.sizeof(nat.AggBwdLayout) == 18 * 8 + 8 + 6 * 4
    assert [int(re.search(r"#define DSMIL_BWD_TILE_%s (\d)" % t.upper(), text).group(1)) for t in nat.BWD_TILE] == [0, 1, 2, 3]
    out = nat.AggBwdLayout()
    L = nat.lib()
    assert L.dsmil_agg_backward_layout(0, 100, 512, 512, 2, 1, 1, 1, None) == nat.DSMIL_E_INVALID
    for bad in ((-1, 100, 512, 512, 2), (0, 0, 512, 512, 2), (3, 2, 512, 512, 2), (0, 100, 0, 512, 2), (0, 100, 512, 0, 2), (0, 100, 512, 512, 0)):
        assert L.dsmil_agg_backward_layout(*bad, 1, 1, 1, ctypes.byref(out)) == nat.DSMIL_E_INVALID, bad


def test_layout_query_offsets_ranges_and_tile():
    L = nat.lib()
    # the grid of this file, the boundary of the four-wave regime, and the shapes tests/test_agg_bwd_precision_gpu.py sends
    shapes = [(n, k, kv, c) for n, k, c in itertools.product(ROWS + (65600, 128 * 512 - 1, 128 * 512), KS, CS) for kv in (k, KV_OTHER)]
    shapes += [(n, k, k, c) for (k, c) in ((512, 2), (128, 1), (1024, 2), (256, 5), (166, 1), (64, 3)) for n in (1, 31, 33, 64, 65, 400, 611)]
    regions = nat.AggBwdLayout.REGIONS
    for (n, k, kv, c), nonlinear, nb in itertools.product(shapes, (0, 1), (0, 1, 7)):
        if n < nb:
            continue
        for rows16, w16 in ((1, 1), (0, 1), (1, 0)):
            lay = nat.backward_layout(nb, n, k, kv, c, nonlinear, rows16, w16)
            off = [getattr(lay, r) for r in regions]
            tag = (nb, n, k, kv, c, nonlinear, rows16, w16)
            assert all(o % 256 == 0 for o in off) and off == sorted(off) and off[0] == 0, tag
            size = L.dsmil_agg_backward_bags_workspace_bytes(nb, n, k, kv, c) if nb else L.dsmil_agg_backward_workspace_bytes(n, k, kv, c)
            end = lay.part_b + lay.splits * 128 * 4
            # The size queries do not know the query's form and answer the larger of the two layouts.  That is the nonlinear one
            # only while both forms get the same number of row ranges: with two column slabs fewer the linear query gets more
            # ranges (TN_WGS / nslab), and from a few thousand rows on ITS partials make the larger layout.  The queries
            # answered the nonlinear size alone before this test existed, and a linear-query call sized by them was refused.
            other = nat.backward_layout(nb, n, k, kv, c, 1 - nonlinear, rows16, w16).total
            assert end <= lay.total <= size == max(lay.total, other), tag
            if nonlinear and lay.total >= other:
                assert lay.total == size, tag
            assert lay.S * lay.R >= n > (lay.S - 1) * lay.R and lay.R % 64 == 0, tag
            assert lay.splits * lay.small_rows >= n > (lay.splits - 1) * lay.small_rows and lay.T32 == (n + 31) // 32, tag
            # every region is large enough for what the docstring of the query says it holds
            sets = max(nb, 1)
            qtiles = n // 32 + nb + 1 if nb else lay.T32
            need = {"gB": sets * c * kv, "Dv": sets * c, "qmax": sets * c * 128, "gq": sets * c * 128, "gA": n * c, "gs": n * c,
                    "gz2": n * 128, "Hb": n * 128, "Qb": n * 128, "gH": n * 128, "gqp": qtiles * c * 128, "part0": lay.S * 128 * k,
                    "part1": lay.S * 128 * 128, "pb0": lay.S * 128, "pb1": lay.S * 128, "part": lay.splits * c * k}
            for r, nxt in zip(regions, regions[1:]):
                assert getattr(lay, nxt) - getattr(lay, r) >= 4 * need[r], (tag, r)
            # the tile rule, from the launch sequences' own statements
            tile = nat.BWD_TILE[lay.tile]
            four, staged = n // 128 >= 512, (k % 4 != 0 or not rows16)
            assert tile.startswith("w4") == (four and not (nb and staged)), tag       # N / 128 >= 512 gives four-wave ...
            assert tile.endswith("_reg") == staged, tag                               # K % 4 != 0 or unaligned rows: register-staged
            assert not (nb and tile == "w4_reg"), tag                                 # ... but no four-wave register-staged form over slots
            assert lay.qrow_vec == (4 if (k % 4 == 0 and rows16 and w16) else 1), tag
