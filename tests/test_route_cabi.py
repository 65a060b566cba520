"""The aggregator forward's route (dsmil_agg_forward_route, csrc/agg_fwd.hip pick_route): which kernels a call takes, asked
without a device.  The expected routes below were written down from the launch ladder of agg_forward_impl as it stood
BEFORE the route function existed (one if / else-if chain of ~220 lines), not from the new code's answers.  CPU only."""
import contextlib
import ctypes

import dsmil  # noqa: F401  (registers the dsmil_wsi_amd package)
import dsmil_wsi_amd._native as nat

CUS = 256    # an unpartitioned MI355X; passed in, so that no device is asked
BATCH = dict(n_bags=64, total_rows=640000, max_rows=10000)      # 128-row regime (total / 128 + bags >= 512), uniform
RAGGED = dict(n_bags=64, total_rows=600000, max_rows=10000)     # ... and bags of unequal length
LONE = dict(n_bags=1, total_rows=1500, max_rows=1500)           # 32-row regime
FEW = dict(n_bags=8, total_rows=40000, max_rows=5000)           # 32-row regime, (79 + 2) * 8 = 648 workgroups > 2 * 256
LONG = dict(n_bags=1, total_rows=100000, max_rows=100000)       # one bag in the 128-row regime (a shard)


def route(shape, K=512, Kv=None, C=2, nonlinear=1, **kw):
    r = nat.forward_route(K=K, Kv=K if Kv is None else Kv, C=C, nonlinear=nonlinear, cus=CUS, **dict(shape, **kw))
    d = {n: getattr(r, n) for n, _ in nat.AggRoute._fields_}
    for field, names in (("logits", nat.LOGITS), ("qmax", nat.QMAX), ("image", nat.IMAGE), ("attend", nat.ATTEND),
                         ("finish", nat.FINISH)):
        d[field] = names[d[field]]
    return d


@contextlib.contextmanager
def knob(name, value):
    fn = getattr(nat.lib(), name)
    old = fn(value)
    try:
        yield
    finally:
        fn(old)


def check(got, **want):
    bad = {k: (got[k], v) for k, v in want.items() if got[k] != v}
    assert not bad, f"(got, expected): {bad}\nfull route: {got}"


def test_defaults_of_the_runtime_knobs():
    L = nat.lib()
    assert (L.dsmil_agg_batch_form(-1), L.dsmil_agg_inline_query(-1), L.dsmil_agg_logits_form(-1)) == (2, 1, 1)


def test_fp32_batches():
    # k_attend_f3: two-layer query, C <= 2, K % 128 == 0, K <= 512, v = Identity
    f3 = dict(nw=4, r0=128, logits="stream", logits_cp=2, prologue=0, rowmax=1, qmax="launch", qmax_vec=4, qmax_threads=1024,
              ragged=0, ragged_attend=0, image="f2_cut", attend="f3", finish="vec4", finish_rows=32, pred=1)
    check(route(BATCH), **f3)
    check(route(BATCH, packed_f2=1, packed_split=1), **dict(f3, image="f2_caller"))
    check(route(BATCH, row_map=1), **f3)
    check(route(BATCH, C=1), **dict(f3, logits_cp=1))
    check(route(BATCH, K=128), **f3)
    check(route(RAGGED), **dict(f3, ragged=1, ragged_attend=1, tile_attend=32, tile_logits=128))
    # k_attend_f2: the other resident form — one-layer query, C > 2, or dsmil_agg_batch_form(1)
    f2 = dict(f3, attend="f2", finish_rows=64)
    check(route(BATCH, nonlinear=0), **f2)
    check(route(BATCH, C=3), **f2)
    check(route(BATCH, C=17, K=256), **f2)
    check(route(RAGGED, C=3), **dict(f2, ragged=1, ragged_attend=0, tile_attend=32, tile_logits=128))
    with knob("dsmil_agg_batch_form", 1):
        check(route(BATCH), **f2)
    # k_query_attend_split on 128-row tiles: dsmil_agg_batch_form(0), V != feats, K outside the resident kernels, given classes
    split = dict(f3, rowmax=0, image="split_cut", attend="split", attend_nw=4, attend_vec=4, attend_np=6, attend_xe=0,
                 attend_tu=8, finish_rows=128)
    with knob("dsmil_agg_batch_form", 0):
        check(route(BATCH), **split)
        check(route(BATCH, packed_split=1, packed_f2=1), **dict(split, image="split_caller"))
        check(route(RAGGED), **dict(split, ragged=1, ragged_attend=0))
    check(route(BATCH, vals_separate=1), **split)
    check(route(BATCH, vals_separate=1, Kv=384), **split)
    check(route(BATCH, K=1024), **split)
    check(route(BATCH, K=192), **split)
    check(route(BATCH, classes_given=1), **dict(split, logits="given", logits_vec=1, logits_cp=0))
    check(route(RAGGED, classes_given=1), **dict(split, logits="given", logits_vec=1, logits_cp=0, ragged=0))
    # rows that cannot be read with 16-byte loads: MUSK's K = 166, or a misaligned operand
    check(route(BATCH, K=166, C=1), **dict(split, logits="argmax", logits_vec=1, logits_cp=0, qmax_vec=1, attend_vec=1,
                                            finish="scalar"))
    check(route(BATCH, aligned=2), **dict(split, logits="argmax", logits_vec=1, logits_cp=0, qmax_vec=1, attend_vec=1))
    check(route(BATCH, vals_separate=1, Kv=166), **dict(split, logits="argmax", logits_vec=1, logits_cp=0, qmax_vec=1,
                                                         attend_vec=1, finish="scalar"))


def test_fp32_few_rows():
    # k_attend_hs with the critical row's query inside the launch: (ceil(1500 / 64) + C) * 1 workgroups <= 2 * CUs
    hs = dict(nw=1, r0=32, logits="stream", logits_cp=2, rowmax=0, qmax="inline", ragged=0, ragged_attend=0, image="split_cut",
              attend="hs", finish="vec4", finish_rows=64, pred=1)
    check(route(LONE), **hs)
    check(route(LONE, packed_split=1), **dict(hs, image="split_caller"))
    check(route(LONE, row_map=1, vals_separate=1, C=5), **hs)
    check(route(LONE, C=1), **dict(hs, logits_cp=1))
    check(route(dict(n_bags=3, total_rows=4000, max_rows=1500)), **hs)    # a ragged batch in the 32-row regime: no work lists
    # ... and with the k_qmax launch: too many workgroups to be resident at once, dsmil_agg_inline_query(0), given classes
    launch = dict(hs, qmax="launch", qmax_vec=4, qmax_threads=1024)
    check(route(FEW), **launch)
    check(route(dict(FEW, n_bags=6, total_rows=30000)), **dict(hs))       # (79 + 2) * 6 = 486 <= 512
    with knob("dsmil_agg_inline_query", 0):
        check(route(LONE), **launch)
    check(route(LONE, classes_given=1), **dict(launch, r0=128, logits="given", logits_vec=1, logits_cp=0))
    # the training step: no bag head, the logits launch carries the prologue job
    check(route(LONE, skip_pred=1, prologue_job=1, packed_split=1), **dict(hs, image="split_caller", prologue=1, pred=0))
    check(route(LONE, skip_pred=1), **dict(hs, prologue=0, pred=0))
    # no 16-byte loads: k_query_attend_split on 32-row tiles, register-staged
    small = dict(nw=1, r0=128, logits="argmax", logits_vec=1, qmax="launch", qmax_vec=1, qmax_threads=1024, image="split_cut",
                 attend="split", attend_nw=1, attend_vec=1, attend_np=6, finish="scalar", finish_rows=32, pred=1, prologue=0)
    check(route(LONE, K=166, C=1), **small)
    check(route(LONE, K=166, C=1, skip_pred=1, prologue_job=1), **dict(small, pred=0))
    check(route(LONE, aligned=6), **dict(small, finish="vec4"))


def test_bf16():
    res = dict(nw=4, r0=128, logits="stream", logits_cp=2, rowmax=0, qmax="launch", qmax_vec=4, qmax_threads=1024, ragged=0,
               ragged_attend=0, image="bf16", attend="bf16_res", finish="vec4", finish_rows=64, pred=1)
    check(route(BATCH, bf16=1), **res)
    check(route(BATCH, bf16=1, K=256, C=1, nonlinear=0), **dict(res, logits_cp=1))
    check(route(RAGGED, bf16=1), **dict(res, ragged=1, ragged_attend=1, tile_attend=64, tile_logits=128))
    check(route(BATCH, bf16=1, aligned=0), **dict(res, qmax_vec=1))    # (the bf16 rows themselves are checked by the entry point)
    # the co-resident set (k_logits_pipe, 4-wave k_qmax, lean k_finish): K = 512, C <= 2, when several streams are in use
    pipe = dict(res, r0=512, logits="pipe", qmax_threads=256, finish="lean")
    check(route(BATCH, bf16=1, several_streams=1), **pipe)
    check(route(RAGGED, bf16=1, several_streams=1), **dict(pipe, ragged=1, ragged_attend=1, tile_attend=64, tile_logits=512))
    check(route(BATCH, bf16=1, several_streams=1, K=256), **res)
    check(route(BATCH, bf16=1, several_streams=1, row_map=1), **res)
    check(route(BATCH, bf16=1, several_streams=1, classes_given=1), **dict(res, logits="given", logits_vec=1, logits_cp=0))
    with knob("dsmil_agg_logits_form", 2):
        check(route(BATCH, bf16=1), **pipe)
        check(route(BATCH, bf16=1, C=1), **dict(pipe, logits_cp=1))
    with knob("dsmil_agg_logits_form", 0):
        check(route(BATCH, bf16=1, several_streams=1), **res)
    # k_query_attend_bf16_dma: what the resident kernel is not instantiated for (K, C > 2, V != feats)
    dma = dict(res, attend="bf16_dma", finish_rows=128)
    check(route(BATCH, bf16=1, K=1024), **dma)
    check(route(BATCH, bf16=1, C=3), **dma)
    check(route(RAGGED, bf16=1, vals_separate=1), **dict(dma, ragged=1, ragged_attend=0))
    # ... k_logits_pipe does not ask for V == feats, the lean k_finish goes with the resident kernel only
    check(route(BATCH, bf16=1, vals_separate=1, several_streams=1), **dict(dma, r0=512, logits="pipe", qmax_threads=256))
    # the ring kernel: few rows
    ring = dict(res, nw=1, r0=32, attend="bf16_ring", attend_nw=1, finish_rows=32)
    check(route(LONE, bf16=1), **ring)
    check(route(LONE, bf16=1, several_streams=1), **ring)
    check(route(FEW, bf16=1, C=4, K=1024), **ring)


def test_shard_phases():
    # phase 1 (dsmil_agg_shard_argmax) ends behind k_qmax; phase 2 (dsmil_agg_shard_attend) starts there, against given rows
    check(route(LONG, phase=1), nw=4, r0=128, logits="stream", rowmax=0, qmax="shard1", qmax_vec=4, qmax_threads=1024,
          image="none", attend="none", finish="none", pred=0)
    check(route(LONE, phase=1), nw=1, r0=32, logits="stream", qmax="shard1", qmax_vec=4, attend="none", finish="none", pred=0)
    check(route(LONE, phase=1, K=166), nw=1, r0=128, logits="argmax", logits_vec=1, qmax="shard1", qmax_vec=1, attend="none")
    check(route(LONG, phase=2), nw=4, r0=128, logits="none", rowmax=0, qmax="shard2", qmax_vec=4, qmax_threads=1024, ragged=0,
          image="split_cut", attend="split", attend_nw=4, attend_vec=4, attend_np=6, finish="vec4", finish_rows=128, pred=0)
    check(route(LONE, phase=2), nw=1, r0=128, logits="none", qmax="shard2", qmax_vec=4, image="split_cut", attend="hs",
          finish="vec4", finish_rows=64, pred=0)
    check(route(LONE, phase=2, aligned=3), qmax="shard2", qmax_vec=1, attend="hs")
    check(route(LONE, phase=2, vals_separate=1, Kv=166), qmax="shard2", qmax_vec=4, attend="split", attend_nw=1, attend_vec=1,
          finish="scalar", finish_rows=32)


def test_query_needs_valid_sizes_and_leaves_the_stream_record_alone():
    L = nat.lib()
    r = nat.AggRoute()
    assert L.dsmil_agg_forward_route(None, ctypes.byref(r)) == nat.DSMIL_E_INVALID
    for bad in (dict(n_bags=0), dict(total_rows=0), dict(max_rows=0), dict(max_rows=2000), dict(K=0), dict(Kv=0), dict(C=0)):
        c = nat.AggCall(**dict(dict(LONE, K=512, Kv=512, C=2), **bad))
        assert L.dsmil_agg_forward_route(ctypes.byref(c), ctypes.byref(r)) == nat.DSMIL_E_INVALID, bad
    # dsmil_agg_logits_form(1): the answer follows several_streams as GIVEN; asking — however often, whatever was asked in
    # between — records nothing, so the same question keeps its answer
    assert L.dsmil_agg_logits_form(-1) == 1
    for _ in range(6):
        assert route(BATCH, bf16=1)["logits"] == "stream"
        assert route(BATCH, bf16=1, several_streams=1)["logits"] == "pipe"
    assert [route(BATCH, bf16=1)["logits"] for _ in range(8)] == ["stream"] * 8


# (n_bags, total_rows, K, Kv, C, dsmil_agg_tile_rows, dsmil_agg_workspace_bytes) as the library answered before the change
SIZES = [
    (1, 1, 512, 512, 2, 32, 5037312), (1, 1, 166, 166, 1, 32, 1101312), (1, 1, 1024, 1024, 2, 32, 9891072),
    (1, 1, 256, 256, 3, 32, 3668736), (1, 1, 512, 384, 2, 32, 3987712), (1, 1, 128, 128, 17, 32, 9402112),
    (1, 1500, 512, 512, 2, 32, 5043968), (1, 1500, 166, 166, 1, 32, 1107456), (1, 1500, 1024, 1024, 2, 32, 9897728),
    (1, 1500, 256, 256, 3, 32, 3676160), (1, 1500, 512, 384, 2, 32, 3994368), (1, 1500, 128, 128, 17, 32, 9417216),
    (1, 65407, 512, 512, 2, 32, 9541632), (1, 65407, 166, 166, 1, 32, 2072064), (1, 65407, 1024, 1024, 2, 32, 18573312),
    (1, 65407, 256, 256, 3, 32, 7162112), (1, 65407, 512, 384, 2, 32, 7447552), (1, 65407, 128, 128, 17, 32, 19131648),
    (1, 65408, 512, 512, 2, 128, 5347584), (1, 65408, 166, 166, 1, 128, 1386752), (1, 65408, 1024, 1024, 2, 128, 10201344),
    (1, 65408, 256, 256, 3, 128, 4004352), (1, 65408, 512, 384, 2, 128, 4297984), (1, 65408, 128, 128, 17, 128, 10114816),
    (1, 100000, 512, 512, 2, 128, 7728896), (1, 100000, 166, 166, 1, 128, 1900288), (1, 100000, 1024, 1024, 2, 128, 14790400),
    (1, 100000, 256, 256, 3, 128, 5851136), (1, 100000, 512, 384, 2, 128, 6127360), (1, 100000, 128, 128, 17, 128, 15258368),
    (8, 40000, 512, 512, 2, 32, 6198528), (8, 40000, 166, 166, 1, 32, 1437184), (8, 40000, 1024, 1024, 2, 32, 12010752),
    (8, 40000, 256, 256, 3, 32, 4614656), (8, 40000, 512, 384, 2, 32, 4909312), (8, 40000, 128, 128, 17, 32, 12130560),
    (64, 640000, 512, 512, 2, 128, 45636608), (64, 640000, 166, 166, 1, 128, 10089216), (64, 640000, 1024, 1024, 2, 128, 87518208),
    (64, 640000, 256, 256, 3, 128, 35757056), (64, 640000, 512, 384, 2, 128, 35330048), (64, 640000, 128, 128, 17, 128, 119675648),
    (64, 600000, 512, 512, 2, 128, 42855424), (64, 600000, 166, 166, 1, 128, 9488384), (64, 600000, 1024, 1024, 2, 128, 82177024),
    (64, 600000, 256, 256, 3, 128, 33570560), (64, 600000, 512, 384, 2, 128, 33188864), (64, 600000, 128, 128, 17, 128, 112255744),
    (511, 128, 512, 512, 2, 128, 7741952), (511, 128, 166, 166, 1, 128, 1722880), (511, 128, 1024, 1024, 2, 128, 14749952),
    (511, 128, 256, 256, 3, 128, 6132736), (511, 128, 512, 384, 2, 128, 6153728), (511, 128, 128, 128, 17, 128, 19672064),
    (512, 512, 512, 512, 2, 128, 7749120), (512, 512, 166, 166, 1, 128, 1725696), (512, 512, 1024, 1024, 2, 128, 14761472),
    (512, 512, 256, 256, 3, 128, 6139392), (512, 512, 512, 384, 2, 128, 6159872), (512, 512, 128, 128, 17, 128, 19696128),
    (300, 27136, 512, 512, 2, 128, 6779904), (300, 27136, 166, 166, 1, 128, 1596928), (300, 27136, 1024, 1024, 2, 128, 12867840),
    (300, 27136, 256, 256, 3, 128, 5359872), (300, 27136, 512, 384, 2, 128, 5424128), (300, 27136, 128, 128, 17, 128, 19865344),
    (300, 27264, 512, 512, 2, 128, 6780928), (300, 27264, 166, 166, 1, 128, 1597952), (300, 27264, 1024, 1024, 2, 128, 12868864),
    (300, 27264, 256, 256, 3, 128, 5360896), (300, 27264, 512, 384, 2, 128, 5425152), (300, 27264, 128, 128, 17, 128, 19866624),
]


def test_sizes_are_what_they_were():
    L = nat.lib()
    for n_bags, total, K, Kv, C, tile_rows, ws_bytes in SIZES:
        assert L.dsmil_agg_tile_rows(n_bags, total) == tile_rows, (n_bags, total)
        assert L.dsmil_agg_workspace_bytes(n_bags, total, K, Kv, C) == ws_bytes, (n_bags, total, K, Kv, C)
        assert route(dict(n_bags=n_bags, total_rows=total, max_rows=(total + n_bags - 1) // n_bags), K=K, Kv=Kv, C=C)["nw"] * 32 == tile_rows


def test_f2_image_question_matches_the_old_python_condition():
    """ops.agg_forward used to mirror the library's condition for building the k_attend_f2 / k_attend_f3 weight image; it now
    asks the route.  The old expression is the yardstick (default knobs, aligned operands, as ops passes them)."""
    L = nat.lib()
    split_is_not_none = L.dsmil_agg_mlp_form() != 0
    n = 0
    for n_bags, total, K, Kv, C, _, _ in SIZES:
        for same_vals in (True, False):
            for given in (False, True):
                for nonlinear in (0, 1):
                    for row_map in (0, 1):
                        if same_vals and Kv != K:
                            continue
                        old = (split_is_not_none and L.dsmil_agg_tile_rows(n_bags, total) == 128 and K % 128 == 0 and K <= 512
                               and same_vals and not given)
                        got = route(dict(n_bags=n_bags, total_rows=total, max_rows=(total + n_bags - 1) // n_bags), K=K, Kv=Kv,
                                    C=C, nonlinear=nonlinear, vals_separate=not same_vals, classes_given=given, row_map=row_map,
                                    packed_split=split_is_not_none)
                        assert (got["attend"] in ("f3", "f2")) == old, (n_bags, total, K, Kv, C, same_vals, given, nonlinear)
                        assert (got["image"] == "f2_cut") == old and got["rowmax"] == int(old)
                        n += old
    assert n > 50
