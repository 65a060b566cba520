"""The value layer's size entries against a restatement of csrc/agg_value.h's layouts (vp_nks, vp_ntp, the two weight images,
vtn_plan, the two backward workspaces), and the return code of calls that break SEVERAL conditions at once: which refusal an
entry reaches first is part of its behaviour, and the two dtypes order theirs differently.  Every call of the table is
refused before any launch and dereferences nothing.  CPU only."""
import ctypes

import pytest

import dsmil  # noqa: F401  (registers the dsmil_wsi_amd package)
import dsmil_wsi_amd._native as nat
from value_bwd_b16_cases import vtn_plan

OK, E_INVALID, E_UNSUPPORTED, E_WORKSPACE, E_ALIGN = 0, -1, -2, -3, -5
ROWS = (1, 63, 64, 65, 200, 1000, 10000, 640000)
WIDTHS = ((8, 4), (64, 64), (72, 68), (166, 166), (512, 512), (1024, 256), (1056, 64))
MAX_K = 1024       # widest K of the MFMA kernels: wider rows take the plain kernels, which read v_w itself


def al(n):
    return (n + 255) // 256 * 256


def nks(K):        # 16-k steps, K padded to 32
    return 2 * ((K + 31) // 32)


def ntp(Kv):       # 32-column tiles, padded to groups of four
    return ((Kv + 31) // 32 + 3) // 4 * 4


def image_bytes(K, Kv):        # fp32 rows: two fp16 planes and a 256-B trailer
    return nks(K) * ntp(Kv) * 2 * 64 * 16 + 256


def image_b16_bytes(K, Kv):    # bf16 rows: one bf16 plane
    return nks(K) * ntp(Kv) * 64 * 16


def partials_bytes(rows, K, Kv):
    S, _ = vtn_plan(rows, K, Kv)
    return al(S * Kv * K * 4) + al(S * Kv * 4)


@pytest.mark.parametrize("K,Kv", WIDTHS)
def test_size_entries_equal_the_restated_layouts(K, Kv):
    L = nat.lib()
    assert L.dsmil_value_packed_bytes(K, Kv) == image_bytes(K, Kv)
    assert L.dsmil_value_packed_bf16_bytes(K, Kv) == image_b16_bytes(K, Kv)
    for rows in ROWS:
        S, R = vtn_plan(rows, K, Kv)
        assert S >= 1 and R % 64 == 0 and S * R >= rows > (S - 1) * R
        assert L.dsmil_value_workspace_bf16_bytes(rows, K, Kv) == (al(image_b16_bytes(K, Kv)) if K <= MAX_K else 0)
        # fp32: the forward's image leads, the partials follow; bf16: the partials start the workspace
        assert L.dsmil_value_workspace_bytes(rows, K, Kv) == al(image_bytes(K, Kv)) + partials_bytes(rows, K, Kv)
        assert L.dsmil_value_backward_bf16_workspace_bytes(rows, K, Kv) == partials_bytes(rows, K, Kv)


def test_size_entries_answer_zero_for_non_positive_arguments():
    L = nat.lib()
    for bad in (0, -1, -8):
        for f in (L.dsmil_value_packed_bytes, L.dsmil_value_packed_bf16_bytes):
            assert f(bad, 64) == 0 and f(64, bad) == 0
        for f in (L.dsmil_value_workspace_bytes, L.dsmil_value_workspace_bf16_bytes, L.dsmil_value_backward_bf16_workspace_bytes):
            assert f(bad, 64, 64) == 0 and f(10, bad, 64) == 0 and f(10, 64, bad) == 0


def _calls():
    """{entry: call(**overrides)} over one set of good operands; `a` is 256-B aligned, nothing is dereferenced."""
    L = nat.lib()
    buf = (ctypes.c_char * 4096)()
    a = (ctypes.addressof(buf) + 255) // 256 * 256
    p = ctypes.c_void_p
    good = dict(x=p(a), V=p(a), g=p(a), w=p(a), b=p(a), img=p(a), map=None, gw=p(a), gb=p(a), gx=p(a), ws=p(a), nb=1 << 62,
                rows=10, K=64, Kv=64, acc=0)

    def bind(f):
        return lambda **kw: f(dict(good, **kw))
    return a, p, buf, {
        "pack": bind(lambda c: L.dsmil_value_pack(c["w"], c["K"], c["Kv"], c["img"], None)),
        "pack_b16": bind(lambda c: L.dsmil_value_pack_bf16(c["w"], c["K"], c["Kv"], c["img"], None)),
        "fwd": bind(lambda c: L.dsmil_value_forward(c["x"], c["rows"], c["K"], c["Kv"], c["w"], c["b"], c["img"], c["map"], c["V"],
                                                    c["ws"], c["nb"], None)),
        "fwd_b16": bind(lambda c: L.dsmil_value_forward_bf16(c["x"], c["rows"], c["K"], c["Kv"], c["w"], c["b"], c["img"], c["V"],
                                                             c["ws"], c["nb"], None)),
        "bwd": bind(lambda c: L.dsmil_value_backward(c["x"], c["V"], c["g"], c["rows"], c["K"], c["Kv"], c["map"], c["gw"], c["gb"],
                                                     c["ws"], c["nb"], None)),
        "bwd_b16": bind(lambda c: L.dsmil_value_backward_bf16(c["x"], c["V"], c["g"], c["rows"], c["K"], c["Kv"], c["gw"], c["gb"],
                                                              c["ws"], c["nb"], None)),
        "rows": bind(lambda c: L.dsmil_value_backward_rows(None, c["V"], c["g"], c["rows"], c["K"], c["Kv"], c["w"], None, c["acc"],
                                                           c["gx"], c["ws"], c["nb"], None)),
    }


def test_multi_fault_calls_return_the_first_refusal_of_their_entry():
    a, p, _buf, call = _calls()
    HUGE = 1 << 40                      # rows * Kv / 256 beyond 2^31 - 1
    GRID = dict(K=1 << 23, Kv=1 << 23)  # 2^17 x 2^16 slabs of the parameter backward: beyond 2^31 - 1 workgroups
    table = [
        # ---- the pack entries: operands, then the image's alignment
        ("pack", dict(w=None, img=p(a + 8)), E_INVALID),
        ("pack", dict(K=0, img=p(a + 8)), E_INVALID),
        ("pack", dict(img=p(a + 8)), E_ALIGN),
        ("pack_b16", dict(w=None, img=p(a + 8)), E_INVALID),
        ("pack_b16", dict(Kv=-4, img=p(a + 8)), E_INVALID),
        ("pack_b16", dict(img=p(a + 8)), E_ALIGN),
        # ---- fp32 forward: operands, row bound, (wide K), image: caller's | ws NULL, ws alignment, ws size; image alignment
        ("fwd", dict(x=None, rows=HUGE, img=p(a + 8)), E_INVALID),
        ("fwd", dict(rows=HUGE, img=p(a + 8)), E_UNSUPPORTED),
        ("fwd", dict(rows=HUGE, K=1056), E_UNSUPPORTED),                       # the bound comes before the wide-K kernel
        ("fwd", dict(rows=HUGE, img=None, ws=None), E_UNSUPPORTED),
        ("fwd", dict(img=p(a + 8), ws=None), E_ALIGN),                         # an image is given: a NULL ws is no fault
        ("fwd", dict(img=p(a + 8), ws=p(a + 16), nb=0), E_ALIGN),
        ("fwd", dict(img=None, ws=None, nb=0), E_INVALID),
        ("fwd", dict(img=None, ws=p(a + 16), nb=0), E_ALIGN),                  # misaligned and short: alignment first
        ("fwd", dict(img=None, nb=0), E_WORKSPACE),
        ("fwd", dict(img=None, nb=image_bytes(64, 64) - 1), E_WORKSPACE),
        # ---- bf16 forward: operands, K % 8 / Kv % 4, rows / V alignment, row bound, (wide K), then the image as above
        ("fwd_b16", dict(V=None, K=166), E_INVALID),
        ("fwd_b16", dict(K=166, Kv=166, x=p(a + 8)), E_UNSUPPORTED),           # bad K % 8 and a misaligned pointer
        ("fwd_b16", dict(Kv=66, V=p(a + 2), img=p(a + 8)), E_UNSUPPORTED),
        ("fwd_b16", dict(K=1056, Kv=66), E_UNSUPPORTED),                       # Kv % 4 holds for the plain kernel too
        ("fwd_b16", dict(x=p(a + 8), rows=HUGE), E_ALIGN),                     # alignment before the row bound
        ("fwd_b16", dict(V=p(a + 2), rows=HUGE, K=1056), E_ALIGN),
        ("fwd_b16", dict(rows=HUGE, K=1056), E_UNSUPPORTED),
        ("fwd_b16", dict(rows=HUGE, img=None, ws=None), E_UNSUPPORTED),
        ("fwd_b16", dict(x=p(a + 8), img=None, ws=None), E_ALIGN),             # the rows' alignment before the NULL ws
        ("fwd_b16", dict(img=p(a + 8), ws=None), E_ALIGN),
        ("fwd_b16", dict(img=None, ws=None, nb=0), E_INVALID),
        ("fwd_b16", dict(img=None, ws=p(a + 16), nb=0), E_ALIGN),
        ("fwd_b16", dict(img=None, nb=image_b16_bytes(64, 64) - 1), E_WORKSPACE),
        # ---- fp32 parameter backward: operands (ws among them), ws alignment, ws size, grid bound LAST
        ("bwd", dict(ws=None, nb=0, **GRID), E_INVALID),
        ("bwd", dict(ws=p(a + 16), nb=0), E_ALIGN),
        ("bwd", dict(ws=p(a + 16), **GRID), E_ALIGN),                          # grid overflow and a misaligned ws
        ("bwd", dict(nb=0, **GRID), E_WORKSPACE),
        ("bwd", dict(**GRID), E_UNSUPPORTED),
        # ---- bf16 parameter backward: operands, K % 8 / Kv % 4, grid bound, alignment, ws size
        ("bwd_b16", dict(ws=None, K=166), E_INVALID),
        ("bwd_b16", dict(K=166, Kv=166, x=p(a + 8), ws=p(a + 16), nb=0), E_UNSUPPORTED),
        ("bwd_b16", dict(ws=p(a + 16), **GRID), E_UNSUPPORTED),                # the same pair as above: the bound first here
        ("bwd_b16", dict(nb=0, **GRID), E_UNSUPPORTED),
        ("bwd_b16", dict(V=p(a + 4), nb=0), E_ALIGN),
        ("bwd_b16", dict(ws=p(a + 16), nb=0), E_ALIGN),
        # ---- input-row backward: operands, alignment of a given ws, grid bound
        ("rows", dict(V=None, ws=p(a + 16)), E_INVALID),
        ("rows", dict(ws=p(a + 16), rows=1 << 36, K=1 << 20), E_ALIGN),
        ("rows", dict(ws=None, rows=1 << 36, K=1 << 20), E_UNSUPPORTED),       # 2^14 slabs x 2^29 row tiles
    ]
    for entry, kw, want in table:
        assert call[entry](**kw) == want, (entry, kw)
