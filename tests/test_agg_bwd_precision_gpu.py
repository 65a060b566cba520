"""The fp32 aggregator backward (ops.agg_backward -> dsmil_agg_backward_ex / _rows, ops.agg_backward_bags -> dsmil_agg_backward_bags)
STAGE BY STAGE against fp64 at the derived bars of tests/agg_bwd_precision_cases.py — the bars a backward that lost one plane
product misses by 2 and more and one that lost an operand plane by hundreds (tests/test_agg_bwd_precision_host.py), where the
end-to-end bar of tests/test_agg_bwd_gpu.py and its siblings lets both pass.  Every stage's reference is fp64 of the device's OWN
inputs of that stage, read back from the workspace at the offsets dsmil_agg_backward_layout answers.

Per case: the forward, the workspace poisoned, the backward, one synchronisation, the regions read back; the row tile the layout
query names is the one the case is there for; every stage's error / bar is printed and at most 1.
  hidden-split 64-row tile, one bag   (K, C) = (512, 2), (128, 1), (1024, 2), (256, 5) at 1, 31, 33, 64, 65, 400, 400 rows; the input
                                      rows' gradient (stage 10) at (512, 2)
  one-wave register-staged tile       K = 166 at 33 and 400 rows; K = 512 at 65 rows on rows whose address is 4 mod 16
  four-wave LDS-DMA tile              (128, 1) at 65 600 rows = 512 full 128-row tiles and a 64-row one: stages 4 - 6 on 514 rows,
                                      stage 7 on 8 of the 94 row ranges, the rest in full
  linear query                        the linq weights at 65 rows (no stage 6; stage 7 on gz2)
  the caller's value rows             (256, 5) at 65 rows, vals its own tensor, want_g_vals (stage 9; stage 2 on vals)
  batch entry                         bags of 1, 31, 33, 64, 65, 400, 17 rows at (512, 2) (with stage 10) and at (166, 1): per-bag
                                      heads, tile slots, idle slots
  row map                             (512, 2) at 65 rows through a row map over a larger NaN-filled tensor
The bf16-row entries state another precision (tests/test_bwd_b16_gpu.py); the train-step entries reuse these kernels.
The rows, weights and upstream gradients of a case are made once (functools.lru_cache in the cases file) and left unchanged; a
stage's fp64 reference is a function of the device's own values and is formed per run."""
import functools

import numpy as np
import pytest
import torch

import agg_bwd_precision_cases as bc
import agg_precision_cases as ac
from util import poison_workspace

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _weights_dev(s):
    return {k: _dev(v) for k, v in ac.weights(s).items()}


def _dev(a):
    return torch.from_numpy(np.array(a)).cuda()          # (a copy: the cases' arrays are read-only)


def _region(ws, off, shape):
    n = int(np.prod(shape))
    return ws[off:off + 4 * n].view(torch.float32).reshape(shape).cpu().numpy()


def _run(c):
    """One case on the device: (inputs, the device's values of every stage, the layout)."""
    from dsmil_wsi_amd import ops, _native
    x_log, lengths = bc.case_rows(c.name)
    K, C = ac.dims(c.s)
    N, nb = len(x_log), len(lengths)
    p = _weights_dev(c.s)
    kw = {"nonlinear": c.nonlinear}
    if c.row_map:       # logical row i lives at physical row rmap[i] of a tensor with 64 more rows, which hold NaN
        rmap = np.random.default_rng(5).permutation(N + 64)[:N].astype(np.int64)
        phys = np.full((N + 64, K), np.nan, np.float32)
        phys[rmap] = x_log
        x = _dev(phys)
        kw["row_map"] = _dev(rmap)
    elif c.misalign:    # the same rows one float further: a contiguous view whose address is 4 mod 16
        buf = torch.zeros(N * K + 4, dtype=torch.float32, device="cuda")
        x = buf[1:1 + N * K].view(N, K)
        x.copy_(_dev(x_log))
        assert x.is_contiguous() and x.data_ptr() % 16 == 4
    else:
        x = _dev(x_log)
    if c.own_vals:
        kw["vals"] = _dev(bc.case_vals(c.name))
    up = {k: _dev(v) for k, v in bc.case_upstream(c.name).items()}
    L = _native.lib()
    one = c.entry == "one"
    need = L.dsmil_agg_backward_workspace_bytes(N, K, K, C) if one else L.dsmil_agg_backward_bags_workspace_bytes(nb, N, K, K, C)
    ops._workspace(x.device, need)       # the forward and the backward then share one buffer: the poison below is what the backward finds
    # the forward reads the rows wherever they are aligned: its outputs are the backward's INPUTS here, not what is under test
    x_fwd = _dev(x_log) if c.misalign else x
    _, _, A, B, idx = ops.agg_forward(x_fwd, list(lengths), p, **kw)
    poison_workspace(ops)
    if one:
        g = ops.agg_backward(x, p, A, B, idx, up["g_pred"][0], g_classes=up["g_classes"], g_A=up["g_A"], g_B=up["g_B"][0],
                             g_max=up["g_max"][0], want_g_vals=c.own_vals, want_g_feats=c.gx, **kw)
    else:
        g = ops.agg_backward_bags(x, list(lengths), p, A, B, idx, up["g_pred"], g_classes=up["g_classes"], g_A=up["g_A"],
                                  g_B=up["g_B"], g_max=up["g_max"], want_g_vals=c.own_vals, want_g_feats=c.gx, **kw)
    torch.cuda.synchronize()
    lay = _native.backward_layout(0 if one else nb, N, K, K, C, int(c.nonlinear), int(x.data_ptr() % 16 == 0),
                                  int(p["q0_w"].data_ptr() % 16 == 0))
    ws = ops._ws_last[0]
    assert ws.numel() >= lay.total and ws.data_ptr() % 256 == 0
    i = bc.build_inputs(c, A.cpu().numpy(), B.cpu().numpy(), idx.cpu().numpy(), lay)
    S, sp = int(lay.S), int(lay.splits)
    d = {"gB": _region(ws, lay.gB, (nb, C, K)), "Dv": _region(ws, lay.Dv, (nb, C)), "qmax": _region(ws, lay.qmax, (nb, C, 128)),
         "gq": _region(ws, lay.gq, (nb, C, 128)), "gA": _region(ws, lay.gA, (N, C)), "gs": _region(ws, lay.gs, (N, C)),
         "gz2": _region(ws, lay.gz2, (N, 128)), "Q": _region(ws, lay.Qb, (N, 128)),
         "part0": _region(ws, lay.part0, (S, 128, K)), "pb0": _region(ws, lay.pb0, (S, 128)),
         "part": _region(ws, lay.part, (sp, C, K)), "part_b": _region(ws, lay.part_b, (sp, C))}
    if c.nonlinear:
        d.update(H=_region(ws, lay.Hb, (N, 128)), gH=_region(ws, lay.gH, (N, 128)),
                 part1=_region(ws, lay.part1, (S, 128, 128)), pb1=_region(ws, lay.pb1, (S, 128)))
    # gqp: one [C, 128] partial per 32-row tile; bag b's first tile slot is offsets[b] / 32 + b in the batch, the tile itself in the one bag
    slots = N // 32 + nb + 1 if not one else int(lay.T32)
    gqp = _region(ws, lay.gqp, (slots, C, 128))
    d["gqp"] = [gqp[(0 if one else int(i.off[b]) // 32 + b):][:-(-lengths[b] // 32)] for b in range(nb)]
    for k, t in g.items():
        d["g_" + k] = t.cpu().numpy()
    return i, d, lay


def _check(name):
    from dsmil_wsi_amd import _native
    c = bc.BY_NAME[name]
    i, d, lay = _run(c)
    assert _native.BWD_TILE[lay.tile] == c.tile, (name, _native.BWD_TILE[lay.tile])
    res = {f"{st}.{k}": v for st, r in bc.check_all(i, d).items() for k, v in r.items()}
    print(f"{name} [{c.tile}] error / bar: " + ", ".join(f"{k} {v:.3f}" for k, v in res.items()))
    bad = {k: v for k, v in res.items() if not v <= 1.0}
    assert not bad, f"{name}: stages beyond their bars: {bad}"


@pytest.mark.parametrize("s", bc.HS_SETS, ids=ac.set_name)
def test_hidden_split_tile_one_bag(s):
    for c in bc.CASES:
        if c.name.startswith("hs_") and c.s == s:
            _check(c.name)


@pytest.mark.parametrize("name", ["w1reg_K166_33", "w1reg_K166_400", "w1reg_unaligned_K512_65"])
def test_one_wave_register_staged_tile(name):
    _check(name)


def test_four_wave_dma_tile_65600_rows():
    _check("w4dma_K128_65600")


def test_linear_query():
    _check("linq_65")


def test_callers_value_rows():
    _check("own_vals_K256_C5_65")


@pytest.mark.parametrize("name", ["bags_K512_C2", "bags_K166_C1"])
def test_batch_entry(name):
    _check(name)


def test_through_a_row_map():
    _check("rowmap_K512_65")
