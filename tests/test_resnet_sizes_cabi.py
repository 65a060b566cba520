"""The embedder's size queries answer what they answered before the host code got its conv plans (csrc/resnet_fwd.hip:
plan_conv / plan_stem): workspace bytes, packed-image bytes per precision, conv and norm-channel counts and the feature width
are observable through the C-ABI and cached by callers, so a refactor of the host side must not move any of them.  The
expected values in tests/golden/resnet_sizes.json were recorded from the library before that refactor
(tools/embed_plan_check.py sizes).  Pure host code: no GPU."""
import json
import os

import dsmil_wsi_amd._native as nat

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "resnet_sizes.json")
DEPTHS = (18, 34, 50, 101)
BATCHES = (1, 2, 7, 33, 256, 257)
SIZES = ((32, 32), (33, 47), (64, 70), (96, 160), (224, 224), (225, 231), (256, 256))


def query():
    """Every size the C-ABI answers, as the JSON-able dict the fixture holds."""
    L = nat.lib()
    out = {}
    for d in DEPTHS:
        out[str(d)] = {
            "num_convs": int(L.dsmil_resnet_num_convs(d)),
            "norm_channels": int(L.dsmil_resnet_norm_channels(d)),
            "feature_dim": int(L.dsmil_resnet_feature_dim(d)),
            "packed_bytes": int(L.dsmil_resnet_packed_bytes(d)),
            "packed_bytes_ex": [int(L.dsmil_resnet_packed_bytes_ex(d, p)) for p in range(4)],
            "workspace_bytes": {f"{B}x{H}x{W}": int(L.dsmil_resnet_workspace_bytes(d, B, H, W))
                                for B in BATCHES for (H, W) in SIZES},
        }
    return out


def test_resnet_size_queries_equal_the_recorded_values():
    with open(GOLDEN) as f:
        want = json.load(f)
    got = query()
    assert set(got) == set(want)
    for d in want:
        assert len(want[d]["workspace_bytes"]) == len(BATCHES) * len(SIZES)
        for k in want[d]:
            assert got[d][k] == want[d][k], (d, k)
