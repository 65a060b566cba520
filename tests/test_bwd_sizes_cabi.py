"""The aggregator backward's and training steps' workspace queries answer what they answered before the two launch
sequences got one workspace layout (csrc/agg_bwd.hip: bwd_layout with n_bags == 0 for the one bag, param_sizes for the
steps): callers size and cache their workspaces from these numbers, so a refactor of the host side must not move any of
them.  The expected values in tests/golden/bwd_sizes.json were recorded from the library before that refactor
(tools/bwd_host_check.py sizes).  Pure host code: no GPU."""
import itertools
import json
import os

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
