"""Host-side operators over the C-ABI (include/dsmil_hip.h) for CUDA(HIP) tensors.

PyTorch is plumbing here: it owns device memory and the stream; all arithmetic of the forward
hot path happens in libdsmil_hip.so.  Functions raise if handed CPU tensors — the CPU route of
the nn.Modules (config 0, MUSK1 plumbing) never comes through this file.
"""
import collections
import copy
import ctypes

import numpy as np
import torch

from . import _native

Q_DIM = 128

_ws_cache = {}
_off_cache = collections.OrderedDict()


class _LRU:
    """Tiny keyed cache for derived device buffers (packed / folded weights).  Keys carry the device and
    the (data_ptr, _version) of every source tensor; each entry also holds the sources themselves, so a
    freed tensor's address can never come back as a different model's weight while its entry lives.
    A handful of entries: tree mode alternates two embedders, DDP-less multi-device processes hold one
    model per device."""

    def __init__(self, cap=8):
        self.cap = cap
        self.d = collections.OrderedDict()

    def get(self, key):
        v = self.d.get(key)
        if v is not None:
            self.d.move_to_end(key)
        return v

    def put(self, key, value):
        self.d[key] = value
        self.d.move_to_end(key)
        while len(self.d) > self.cap:
            self.d.popitem(last=False)
        return value


def _tkey(t):
    return None if t is None else (t.data_ptr(), t._version)


def _stream(device):
    return ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)


_ws_last = [None]


def _workspace(device, nbytes):
    """Scratch for one native call, cached per (device, HIP stream): calls on different streams may run concurrently
    (StreamPool) and must not share partial buffers.  Allocated while that stream is current, so the caching
    allocator ties its lifetime to the stream's work."""
    key = (str(device), int(torch.cuda.current_stream(device).cuda_stream))
    buf = _ws_cache.get(key)
    if buf is None or buf.numel() < nbytes:
        if len(_ws_cache) >= 16:   # transient streams: forget the oldest entries (their memory returns to the allocator)
            for k in list(_ws_cache)[:8]:
                del _ws_cache[k]
        buf = torch.empty(int(nbytes * 1.25) + 4096, dtype=torch.uint8, device=device)
        _ws_cache[key] = buf
    _ws_last[0] = buf
    return buf


class _Ready:
    """Marks device data produced on one stream (a packed weight image) so that OTHER streams wait for it before use —
    an event wait enqueued on the consumer's stream, no host sync (the packing of a training step stays asynchronous)."""

    def __init__(self, dev):
        self.ev = None
        if torch.device(dev).type != "cuda":   # host data (the CPU module path folds BatchNorms too): nothing to wait for
            return
        self.sid = int(torch.cuda.current_stream(dev).cuda_stream)
        self.ev = torch.cuda.Event()
        self.ev.record(torch.cuda.current_stream(dev))

    def wait(self, dev, *buffers):
        """Make the current stream wait for the producer; `buffers` (the cached device tensors about to be read) are
        marked as in use on the current stream, so that an entry evicted from the cache while another stream still reads
        it is not handed back to the producing stream's allocator pool early."""
        if self.ev is None:
            return
        cur = torch.cuda.current_stream(dev)
        if int(cur.cuda_stream) != self.sid:
            cur.wait_event(self.ev)
            for b in buffers:
                if b is not None and b.is_cuda:
                    b.record_stream(cur)


class StreamPool:
    """Round-robin dispatch of INDEPENDENT native calls over n HIP streams of one device.

    The aggregator forward is a chain of kernels with complementary bounds — `k_logits_stream` streams the bag at
    HBM speed with idle matrix cores, `k_query_attend_split` is MFMA-bound at half the HBM rate — and a batch of bags
    cannot overlap them (the critical instance must be known before any score).  Two INDEPENDENT batches can: dealt to
    different streams, the logits pass of one runs under the attend kernel of the other (measured on 64 x 10 000 x 512
    bags: 73.4 k bags/s on one stream, 78.2 k on two, 80.0 k on three; round 6, bf16 bags: the persistent attend kernel
    leaves one 80-register slot per SIMD and the logits / q_max / combine kernels are cut to it — 190 k bags/s on one
    stream, 250-260 k on two or three, `dsmil_agg_logits_form`).  Each stream has its own workspace
    (`_workspace`); outputs are allocated on the stream that produces them; `join()` makes the caller's stream wait
    for everything submitted.

        pool = ops.StreamPool(3)
        outs = [pool.run(ops.agg_forward, feats_b, lengths_b, w) for (feats_b, lengths_b) in batches]
        pool.join()
    """

    def __init__(self, n=3, device=None):
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        self.streams = [torch.cuda.Stream(device=self.device) for _ in range(max(1, int(n)))]
        self._i = 0

    def next_stream(self):
        """The next stream of the round-robin: the one place that deals."""
        s = self.streams[self._i % len(self.streams)]
        self._i += 1
        return s

    def dealer(self):
        """A round-robin of its own over the same streams, from the first: for a caller whose deal must neither depend on nor
        move this pool's count, and that orders its streams itself (next_stream, no wait per call)."""
        d = copy.copy(self)
        d._i = 0
        return d

    def run(self, fn, *args, **kwargs):
        s = self.next_stream()
        s.wait_stream(torch.cuda.current_stream(self.device))   # inputs may have been produced on the caller's stream
        with torch.cuda.stream(s):
            return fn(*args, **kwargs)

    def join(self):
        cur = torch.cuda.current_stream(self.device)
        for s in self.streams:
            cur.wait_stream(s)


def offsets_tensor(lengths, device):
    """Device int64 [n_bags+1] prefix offsets for a tuple of bag lengths (cached: a repeated bag
    shape costs no H2D copy, keeping MILNet.forward free of host syncs)."""
    key = (str(device), tuple(int(n) for n in lengths))
    t = _off_cache.get(key)
    if t is None:
        off = np.zeros(len(key[1]) + 1, np.int64)
        np.cumsum(np.asarray(key[1], np.int64), out=off[1:])
        t = torch.from_numpy(off).to(device)
        _off_cache[key] = t
        if len(_off_cache) > 256:
            _off_cache.popitem(last=False)
    else:
        _off_cache.move_to_end(key)
    return t


def _cuda(t, name):
    if not t.is_cuda:
        raise RuntimeError(f"{name} must be a CUDA(HIP) tensor for the native path")
    return t


def _f32c(t, name):
    if t is None:
        return None
    _cuda(t, name)
    if t.dtype != torch.float32:
        raise RuntimeError(f"{name} must be float32 (got {t.dtype})")
    return t if t.is_contiguous() else t.contiguous()


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)


def fc_forward(feats, fc_w, fc_b):
    """FCLayer / IClassifier.fc on the GPU: dsmil.py:11,24."""
    feats = _f32c(feats, "feats"); fc_w = _f32c(fc_w, "fc_w"); fc_b = _f32c(fc_b, "fc_b")
    N, K = feats.shape
    C = fc_w.shape[0]
    out = torch.empty((N, C), dtype=torch.float32, device=feats.device)
    if N == 0:
        return out
    with torch.cuda.device(feats.device):
        rc = _native.lib().dsmil_fc_forward(_ptr(feats), N, K, C, _ptr(fc_w), _ptr(fc_b), _ptr(out),
                                            _stream(feats.device))
    _native.check(rc, "dsmil_fc_forward")
    return out


_bf16_cache = _LRU()
_split_cache = _LRU()
W_KEYS = ("fc_w", "fc_b", "q0_w", "q0_b", "q2_w", "q2_b", "fcc_w", "fcc_b")   # the field order of struct dsmil_agg_params


def _cached(cache, key, dev, sources, make):
    """The device buffers derived from one weight set, made once per ``key`` (the device and the (data_ptr, _version) of
    every source tensor).  ``make()`` allocates and fills them on the current stream and returns them as a tuple.  The entry
    is (buffers, sources, _Ready): it keeps ``sources`` alive, so that a freed parameter's address can never be mistaken
    for a new one with the same version count, and a hit on another stream waits for the producer (_Ready.wait)."""
    ent = cache.get(key)
    if ent is None:
        ent = cache.put(key, (make(), sources, _Ready(dev)))
    else:
        ent[2].wait(dev, *ent[0])
    return ent[0]


def _pack_image(dev, nbytes, entry, *args):
    """A new uint8 device buffer of ``nbytes`` filled by the library's pack call ``entry``(*args, buffer, stream)."""
    packed = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        rc = getattr(_native.lib(), entry)(*args, _ptr(packed), _stream(dev))
    _native.check(rc, entry)
    return packed


def _bf16_params(w, nonlinear, dev):
    """bf16 path: every weight/bias rounded to bf16 (what module.bfloat16() would hold), kept as
    fp32 tensors for the f32-accumulating stages + the packed bf16 MFMA operands.  Cached per
    parameter set (_cached)."""

    def make():
        r = [w[k].detach().to(torch.bfloat16).to(torch.float32).contiguous() if w.get(k) is not None else None
             for k in W_KEYS]
        q0_w, q2_w = r[2], r[4]
        K = q0_w.shape[1]
        return (_pack_image(dev, _native.lib().dsmil_agg_packed_bf16_bytes(K), "dsmil_agg_pack_bf16", _ptr(q0_w),
                            _ptr(q2_w if nonlinear else None), K), *r)
    key = (str(dev), bool(nonlinear)) + tuple(_tkey(w.get(k)) for k in W_KEYS)
    packed, *r = _cached(_bf16_cache, key, dev, [w.get(k) for k in W_KEYS], make)
    return dict(zip(W_KEYS, r)), packed


def _split_params(q0_w, q2_w, nonlinear, dev):
    """fp32 path, MFMA forms 6 / 9: the query weights cut into three bf16 planes in MFMA-fragment order
    (dsmil_agg_pack_split), prepared once per weight set; None for form 0 (f32 MFMA reads the weights as
    they are)."""
    L = _native.lib()
    if L.dsmil_agg_mlp_form() == 0:
        return None
    K, q2 = q0_w.shape[1], q2_w if nonlinear else None
    key = (str(dev), bool(nonlinear), _tkey(q0_w), _tkey(q2))

    def make():
        nbytes = L.dsmil_agg_packed_split_bytes(K, 1 if nonlinear else 0)
        return (_pack_image(dev, nbytes, "dsmil_agg_pack_split", _ptr(q0_w), _ptr(q2), K),)
    return _cached(_split_cache, key, dev, [q0_w, q2_w], make)[0]


def _f2_params(q0_w, q2_w, nonlinear, dev):
    """fp32 path, batches of bags (k_attend_f2, csrc/agg_f2.h): the query weights as two fp16 planes of their power-of-two
    scaled values in MFMA-fragment order (dsmil_agg_pack_f2), prepared once per weight set."""
    K, q2 = q0_w.shape[1], q2_w if nonlinear else None
    key = ("f2", str(dev), bool(nonlinear), _tkey(q0_w), _tkey(q2))

    def make():
        nbytes = _native.lib().dsmil_agg_packed_f2_bytes(K)
        return (_pack_image(dev, nbytes, "dsmil_agg_pack_f2", _ptr(q0_w), _ptr(q2), K),)
    return _cached(_split_cache, key, dev, [q0_w, q2_w], make)[0]


def _i64c(t, name):
    if t is None:
        return None
    if not t.is_cuda or t.dtype != torch.int64:
        raise RuntimeError(f"{name} must be an int64 CUDA(HIP) tensor")
    return t if t.is_contiguous() else t.contiguous()


def _agg_params(w, K, Kv, nonlinear):
    """struct dsmil_agg_params of the weight dict ``w``, the contiguous fp32 tensors it points into (in W_KEYS order; the
    caller holds them until its call is enqueued) and C."""
    keep = [_f32c(w.get(k), k) for k in W_KEYS]
    C = w["fcc_w"].shape[0]
    p = _native.AggParams(*[(t.data_ptr() if t is not None else 0) for t in keep], K, Kv, C, 1 if nonlinear else 0)
    return p, keep, C


def agg_forward(feats, lengths, w, classes_in=None, vals=None, nonlinear=True, offsets=None, row_map=None):
    """dsmil_agg_forward / dsmil_agg_forward_bf16 over a batch of bags stored back to back.

    feats [total,K] fp32 or bf16 CUDA; lengths: python ints (bag sizes); w: dict of CUDA tensors with
    keys fc_w fc_b q0_w q0_b q2_w q2_b fcc_w fcc_b (fc_* may be None when classes_in is given).
    A bf16 `feats` selects the bf16-storage path (BASELINE config 2): weights are rounded to bf16,
    accumulation stays f32, outputs are fp32.
    ``row_map`` (int64 [total], fp32 path): logical row i lives at physical row row_map[i] of feats / vals —
    train_tcga.py:78-83's `feats[random_indices]` without the gathered copy; `lengths` then count LOGICAL rows.
    Returns (classes [total,C], pred [n_bags,C], A [total,C], B [n_bags,C,Kv], idx int64 [n_bags,C]).
    """
    bf16 = feats.dtype == torch.bfloat16
    if not feats.is_cuda:
        raise RuntimeError("feats must be a CUDA(HIP) tensor for the native path")
    if bf16:
        feats = feats if feats.is_contiguous() else feats.contiguous()
    else:
        feats = _f32c(feats, "feats")
    dev = feats.device
    total, K = feats.shape
    row_map = _i64c(row_map, "row_map")
    if row_map is not None:
        if bf16:
            raise ValueError("row_map is implemented for the fp32 path")
        total = int(row_map.numel())
    lengths = [int(n) for n in lengths]
    if sum(lengths) != total:
        raise ValueError(f"bag lengths sum to {sum(lengths)} but feats has {total} rows")
    if any(n <= 0 for n in lengths):
        raise ValueError("every bag needs at least one instance (the reference's sort/index_select "
                         "at dsmil.py:52-53 fails on an empty bag too)")
    n_bags = len(lengths)
    if vals is None:
        vals = feats
    elif bf16:
        vals = vals.to(torch.bfloat16).contiguous()
    else:
        vals = _f32c(vals, "vals")
    Kv = vals.shape[1]
    packed = None
    if bf16:
        w, packed = _bf16_params(w, nonlinear, dev)
    p, keep, C = _agg_params(w, K, Kv, nonlinear)
    if w["fcc_w"].shape[2] != Kv:
        raise ValueError(f"fcc kernel_size {w['fcc_w'].shape[2]} != value width {Kv}")
    if classes_in is not None:
        classes_in = _f32c(classes_in.float(), "classes_in")
        if tuple(classes_in.shape) != (total, C):
            raise ValueError(f"c must be [{total},{C}], got {tuple(classes_in.shape)}")
    off = offsets if offsets is not None else offsets_tensor(lengths, dev)
    classes = classes_in if classes_in is not None else torch.empty((total, C), dtype=torch.float32, device=dev)
    A = torch.empty((total, C), dtype=torch.float32, device=dev)
    B = torch.empty((n_bags, C, Kv), dtype=torch.float32, device=dev)
    pred = torch.empty((n_bags, C), dtype=torch.float32, device=dev)
    idx = torch.empty((n_bags, C), dtype=torch.int64, device=dev)
    L = _native.lib()
    nbytes = L.dsmil_agg_workspace_bytes(n_bags, total, K, Kv, C)
    ws = _workspace(dev, nbytes)
    with torch.cuda.device(dev):
        if bf16:
            rc = L.dsmil_agg_forward_bf16(_ptr(feats), _ptr(vals), _ptr(off), n_bags, total, max(lengths),
                                          ctypes.byref(p), _ptr(packed), _ptr(classes_in),
                                          _ptr(classes if classes_in is None else None),
                                          _ptr(A), _ptr(B), _ptr(pred), _ptr(idx), _ptr(ws), ws.numel(),
                                          _stream(dev))
        else:
            split = _split_params(keep[2], keep[4], nonlinear, dev)
            # the route of this call (the library's one decision): k_attend_f3 / k_attend_f2 read their own weight image
            f2 = None
            ptrs = [feats, vals, keep[0], keep[2], keep[4] if nonlinear else None]
            route = _native.forward_route(
                total_rows=total, max_rows=max(lengths), n_bags=n_bags, K=K, Kv=Kv, C=C, nonlinear=1 if nonlinear else 0,
                aligned=7 if all(t is None or t.data_ptr() % 16 == 0 for t in ptrs) else 0, classes_given=classes_in is not None,
                vals_separate=vals is not feats, row_map=row_map is not None, packed_split=split is not None)
            if _native.ATTEND[route.attend] in ("f3", "f2"):
                f2 = _f2_params(keep[2], keep[4], nonlinear, dev)
            opts = _native.AggOpts(split.data_ptr() if split is not None else 0,
                                   row_map.data_ptr() if row_map is not None else 0,
                                   f2.data_ptr() if f2 is not None else 0)
            rc = L.dsmil_agg_forward_ex(_ptr(feats), _ptr(vals), _ptr(off), n_bags, total, max(lengths),
                                        ctypes.byref(p), ctypes.byref(opts), _ptr(classes_in),
                                        _ptr(classes if classes_in is None else None),
                                        _ptr(A), _ptr(B), _ptr(pred), _ptr(idx), _ptr(ws), ws.numel(),
                                        _stream(dev))
    _native.check(rc, "dsmil_agg_forward_bf16" if bf16 else "dsmil_agg_forward_ex")
    del keep
    return classes, pred, A, B, idx


def _value_params(v_w, dev):
    """BClassifier.v's weight [Kv, K] as two fp16 planes of its power-of-two scaled values in MFMA-fragment order
    (dsmil_value_pack, csrc/agg_value.h), prepared once per weight set (cached like _f2_params)."""
    Kv, K = v_w.shape

    def make():
        nbytes = _native.lib().dsmil_value_packed_bytes(K, Kv)
        return (_pack_image(dev, nbytes, "dsmil_value_pack", _ptr(v_w), K, Kv),)
    return _cached(_split_cache, ("value", str(dev), _tkey(v_w)), dev, [v_w], make)[0]


def _value_params_b16(v_w, v_b, dev):
    """bf16 rows: BClassifier.v's weight rounded to bf16 in MFMA-fragment order (dsmil_value_pack_bf16, csrc/agg_value.h), the
    fp32 weight the entry also takes and the bias rounded to bf16 and kept as fp32 (what module.bfloat16() would hold, as
    _bf16_params does for the aggregator's), prepared once per weight set.  v_w / v_b: fp32 masters or bf16 parameters."""
    Kv, K = v_w.shape

    def make():
        w32 = v_w.detach().to(torch.float32).contiguous()
        b32 = v_b.detach().to(torch.bfloat16).to(torch.float32).contiguous()
        nbytes = _native.lib().dsmil_value_packed_bf16_bytes(K, Kv)
        return (_pack_image(dev, nbytes, "dsmil_value_pack_bf16", _ptr(w32), K, Kv), w32, b32)
    return _cached(_split_cache, ("value_b16", str(dev), _tkey(v_w), _tkey(v_b)), dev, [v_w, v_b], make)


def value_proj(feats, v_w, v_b, row_map=None):
    """dsmil_value_forward: V = ReLU(feats @ v_w^T + v_b), the Linear + ReLU of BClassifier.v (dsmil.py:35-39,48), in ONE
    native launch (fp32 in, fp32 out; the weight planes are cut once per weight set).  feats [rows, K] fp32 CUDA, v_w [Kv, K],
    v_b [Kv]; ``row_map`` (int64 [n]): logical row i is physical row row_map[i] of feats.  Returns V [n, Kv] in logical order.
    bf16 ``feats`` select dsmil_value_forward_bf16 (the bf16-storage path: v_w and v_b — fp32 masters or bf16 parameters —
    are rounded to bf16, fp32 accumulation, one bf16 MFMA product per MAC): bf16 V [rows, Kv], no row map (its
    parameter gradients: value_proj_backward on the same bf16 rows)."""
    b16 = feats.dtype == torch.bfloat16
    if b16:   # v_w, v_b stay as they are: _value_params_b16 rounds them once per weight set, keyed by their own addresses
        if row_map is not None:
            raise ValueError("row_map is implemented for the fp32 path")
        feats = _cuda(feats, "feats").contiguous(); _cuda(v_w, "v_w"); _cuda(v_b, "v_b")
    else:
        feats = _f32c(feats, "feats"); v_w = _f32c(v_w, "v_w"); v_b = _f32c(v_b, "v_b")
    dev = feats.device
    rows, K = feats.shape
    Kv = v_w.shape[0]
    if v_w.shape[1] != K or v_b.numel() != Kv:
        raise ValueError(f"v_w must be [Kv,{K}] and v_b [Kv], got {tuple(v_w.shape)} / {tuple(v_b.shape)}")
    row_map = _i64c(row_map, "row_map")
    n = int(row_map.numel()) if row_map is not None else rows
    V = torch.empty((n, Kv), dtype=feats.dtype, device=dev)
    if n == 0:
        return V
    L = _native.lib()
    if b16:
        packed, w32, b32 = _value_params_b16(v_w, v_b, dev)
        entry, call = "dsmil_value_forward_bf16", lambda: L.dsmil_value_forward_bf16(
            _ptr(feats), n, K, Kv, _ptr(w32), _ptr(b32), _ptr(packed), _ptr(V), None, 0, _stream(dev))
    else:
        packed = _value_params(v_w, dev)
        entry, call = "dsmil_value_forward", lambda: L.dsmil_value_forward(
            _ptr(feats), n, K, Kv, _ptr(v_w), _ptr(v_b), _ptr(packed), _ptr(row_map), _ptr(V), None, 0, _stream(dev))
    with torch.cuda.device(dev):
        rc = call()
    _native.check(rc, entry)
    return V


def value_proj_backward(feats, V, g_vals, row_map=None):
    """dsmil_value_backward: the PARAMETER gradients of BClassifier.v's Linear behind g_vals (what agg_backward returns as
    ``vals``):  gZ = g_vals * (V > 0),  g_v_w [Kv, K] = gZ^T feats,  g_v_b [Kv] = colsum gZ — deterministic (fixed-order
    sums).  The gradient of the input rows (gZ v_w) is value_proj_backward_rows.  Returns (g_v_w, g_v_b).
    bf16 ``feats`` select dsmil_value_backward_bf16 (the bf16-storage path): V must then be the bf16 V of ``value_proj`` and
    g_vals fp32 (the bf16 aggregator backward's, unrounded); the operands are read as they are stored — no fp32 copy of
    either — and the results are fp32; no row map."""
    b16 = feats.dtype == torch.bfloat16
    if b16:
        if row_map is not None:
            raise ValueError("row_map is implemented for the fp32 path")
        _cuda(feats, "feats"); _cuda(V, "V"); _cuda(g_vals, "g_vals")
        if V.dtype != torch.bfloat16 or g_vals.dtype != torch.float32:
            raise ValueError(f"bf16 rows take a bf16 V and fp32 g_vals, got {V.dtype} / {g_vals.dtype}")
        feats, V, g_vals = feats.contiguous(), V.contiguous(), g_vals.contiguous()
    else:
        feats = _f32c(feats, "feats"); V = _f32c(V, "V"); g_vals = _f32c(g_vals, "g_vals")
    dev = feats.device
    row_map = _i64c(row_map, "row_map")
    n = int(row_map.numel()) if row_map is not None else feats.shape[0]
    if feats.dim() != 2 or V.dim() != 2 or V.shape[0] != n or g_vals.shape != V.shape:
        raise ValueError(f"V / g_vals must be [{n},Kv], got {tuple(V.shape)} / {tuple(g_vals.shape)}")
    K, Kv = feats.shape[1], V.shape[1]
    g_w = torch.empty((Kv, K), dtype=torch.float32, device=dev)
    g_b = torch.empty((Kv,), dtype=torch.float32, device=dev)
    if n == 0:
        return g_w.zero_(), g_b.zero_()
    L = _native.lib()
    if b16:
        entry, ws = "dsmil_value_backward_bf16", _workspace(dev, L.dsmil_value_backward_bf16_workspace_bytes(n, K, Kv))
        call = lambda: L.dsmil_value_backward_bf16(_ptr(feats), _ptr(V), _ptr(g_vals), n, K, Kv, _ptr(g_w), _ptr(g_b), _ptr(ws),
                                                   ws.numel(), _stream(dev))
    else:
        entry, ws = "dsmil_value_backward", _workspace(dev, L.dsmil_value_workspace_bytes(n, K, Kv))
        call = lambda: L.dsmil_value_backward(_ptr(feats), _ptr(V), _ptr(g_vals), n, K, Kv, _ptr(row_map), _ptr(g_w), _ptr(g_b),
                                              _ptr(ws), ws.numel(), _stream(dev))
    with torch.cuda.device(dev):
        rc = call()
    _native.check(rc, entry)
    return g_w, g_b


def value_proj_backward_rows(V, g_vals, v_w, out=None, accumulate=False):
    """dsmil_value_backward_rows: the INPUT-row gradient of BClassifier.v's Linear + ReLU behind g_vals,
    g_x [rows, K] = (g_vals * (V > 0)) @ v_w, in one native launch (k_value_gx: mask applied while the operand is staged,
    bf16 MFMA over exact three-plane cuts, deterministic).  V, g_vals [rows, Kv] fp32 CUDA, v_w [Kv, K].  ``out``: an
    fp32 [rows, K] buffer to write — or, with ``accumulate``, to add to (the aggregator's own g_feats: one buffer, no add
    pass); None allocates.  Returns out."""
    V = _f32c(V, "V"); g_vals = _f32c(g_vals, "g_vals"); v_w = _f32c(v_w, "v_w")
    dev = V.device
    n, Kv = V.shape
    K = v_w.shape[1]
    if tuple(g_vals.shape) != (n, Kv) or v_w.shape[0] != Kv:
        raise ValueError(f"g_vals must be [{n},{Kv}] and v_w [{Kv},K], got {tuple(g_vals.shape)} / {tuple(v_w.shape)}")
    if out is None:
        if accumulate:
            raise ValueError("accumulate needs the buffer to add to (out)")
        out = torch.empty((n, K), dtype=torch.float32, device=dev)
    elif (tuple(out.shape) != (n, K) or out.dtype != torch.float32 or not out.is_contiguous() or out.device != dev):
        raise ValueError(f"out must be a contiguous fp32 [{n},{K}] tensor on {dev}")
    if n == 0:
        return out
    with torch.cuda.device(dev):
        rc = _native.lib().dsmil_value_backward_rows(None, _ptr(V), _ptr(g_vals), n, K, Kv, _ptr(v_w), None,
                                                     1 if accumulate else 0, _ptr(out), None, 0, _stream(dev))
    _native.check(rc, "dsmil_value_backward_rows")
    return out


class GraphedAggForward:
    """MILNet.forward of ONE bag shape captured into a hipGraph and replayed (the library enqueues on the
    caller's stream, allocates nothing and never synchronises, so the whole 5-launch forward is capturable).  A single
    10 000-row bag is launch-bound (5 dependent launches for ~30 us of device work); replay issues them with one call.

        g = GraphedAggForward(w, n_rows, K)          # captures once (weights are read from `w`'s tensors in place)
        classes, pred, A, B, idx = g(feats)          # copies feats into the static input, replays, returns the
                                                     # static output tensors (valid until the next call)
    ``dtype=torch.bfloat16`` captures the bf16-storage path; with ``v_w`` / ``v_b`` the value projection of either dtype is
    one more launch of the same capture.  Inference only: the capture holds the addresses of the weights and of their packed plane cuts, so the weights
    must stay as they are — build a new object after an optimizer step or a load_state_dict."""

    def __init__(self, w, n_rows, K, nonlinear=True, device=None, dtype=torch.float32, v_w=None, v_b=None):
        dev = torch.device(device) if device is not None else w["q0_w"].device
        self.w, self.n, self.nonlinear, self.dev = w, int(n_rows), nonlinear, dev

        def fwd():   # with v_w / v_b (BClassifier(passing_v=True)): the projection launch is captured with the rest (either dtype)
            vals = self._vals = value_proj(self.x, v_w, v_b) if v_w is not None else None   # (V lives as long as the graph)
            return agg_forward(self.x, [self.n], w, vals=vals, nonlinear=nonlinear, offsets=self.offsets)
        self.x = torch.zeros((self.n, K), dtype=dtype, device=dev)
        self.offsets = offsets_tensor([self.n], dev)
        side = torch.cuda.Stream(device=dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side):   # warm-up outside capture: workspace, packed weights, function attributes
            for _ in range(2):
                fwd()
        torch.cuda.current_stream(dev).wait_stream(side)
        torch.cuda.synchronize(dev)
        # the captured launches read these buffers by address: keep them alive as long as the graph
        self._keep = [_split_params(_f32c(w["q0_w"], "q0_w"), _f32c(w.get("q2_w"), "q2_w"), nonlinear, dev)
                      if dtype == torch.float32 else _bf16_params(w, nonlinear, dev)]
        if v_w is not None:
            self._keep.append(_value_params(_f32c(v_w, "v_w"), dev) if dtype == torch.float32
                              else _value_params_b16(v_w, v_b, dev))
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph):
            self.out = fwd()
        self._keep.append(_ws_last[0])   # the workspace of the capture stream

    def __call__(self, feats):
        if tuple(feats.shape) != tuple(self.x.shape):   # copy_ would broadcast a wrong-sized bag silently
            raise ValueError(f"captured for a bag of shape {tuple(self.x.shape)}, got {tuple(feats.shape)}")
        self.x.copy_(feats)
        self.graph.replay()
        return self.out   # the STATIC output tensors of the capture: valid until the next call (clone to keep)


def agg_shard_argmax(feats, w, nonlinear=True):
    """dsmil_agg_shard_argmax: one rank's row range of an instance-sharded bag.
    Returns (classes [rows,C], best_val [C], best_idx [C] shard-local)."""
    feats = _f32c(feats, "feats")
    dev = feats.device
    rows, K = feats.shape
    p, keep, C = _agg_params(w, K, w["fcc_w"].shape[2], nonlinear)
    classes = torch.empty((rows, C), dtype=torch.float32, device=dev)
    best_val = torch.empty((C,), dtype=torch.float32, device=dev)
    best_idx = torch.empty((C,), dtype=torch.int64, device=dev)
    L = _native.lib()
    ws = _workspace(dev, L.dsmil_agg_workspace_bytes(1, rows, K, w["fcc_w"].shape[2], C))
    with torch.cuda.device(dev):
        rc = L.dsmil_agg_shard_argmax(_ptr(feats), rows, ctypes.byref(p), _ptr(classes), _ptr(best_val),
                                      _ptr(best_idx), _ptr(ws), ws.numel(), _stream(dev))
    _native.check(rc, "dsmil_agg_shard_argmax")
    del keep
    return classes, best_val, best_idx


def agg_shard_attend(feats, w, crit_rows, vals=None, nonlinear=True):
    """dsmil_agg_shard_attend: attention of this shard's rows against the bag-wide critical rows.
    Returns (A_unnorm [rows,C] = exp(s - m_shard), ml [C,2] = (m_shard, l_shard), B_unnorm [C,Kv])."""
    feats = _f32c(feats, "feats")
    dev = feats.device
    rows, K = feats.shape
    vals = feats if vals is None else _f32c(vals, "vals")
    Kv = vals.shape[1]
    p, keep, C = _agg_params(w, K, Kv, nonlinear)
    crit_rows = _f32c(crit_rows, "crit_rows")
    if tuple(crit_rows.shape) != (C, K):
        raise ValueError(f"crit_rows must be [{C},{K}], got {tuple(crit_rows.shape)}")
    A = torch.empty((rows, C), dtype=torch.float32, device=dev)
    ml = torch.empty((C, 2), dtype=torch.float32, device=dev)
    B = torch.empty((C, Kv), dtype=torch.float32, device=dev)
    L = _native.lib()
    ws = _workspace(dev, L.dsmil_agg_workspace_bytes(1, rows, K, Kv, C))
    with torch.cuda.device(dev):
        rc = L.dsmil_agg_shard_attend(_ptr(feats), _ptr(vals), rows, ctypes.byref(p), _ptr(crit_rows), _ptr(A),
                                      _ptr(ml), _ptr(B), _ptr(ws), ws.numel(), _stream(dev))
    _native.check(rc, "dsmil_agg_shard_attend")
    del keep
    return A, ml, B


_bce_cache = _LRU()


def bce_class_weights(pos_weight, weight, C, dev):
    """The class-weight tensors of a BCEWithLogitsLoss (each None, or 1 or ``C`` elements on any device in any float type —
    train_mil.py:172 builds a 0-dim one) as what the ``_w`` entries read: contiguous fp32 [C] tensors on ``dev`` (None stays
    None).  Made once per version of the criterion's tensors (_cached)."""
    if pos_weight is None and weight is None:
        return None, None

    def make():
        return tuple(None if t is None else t.detach().to(device=dev, dtype=torch.float32).reshape(-1).expand(C).contiguous()
                     for t in (pos_weight, weight))
    key = (str(dev), int(C), _tkey(pos_weight), _tkey(weight))
    return _cached(_bce_cache, key, dev, [pos_weight, weight], make)


def _bce_weights(pos_weight, weight, C, dev):
    """struct dsmil_bce_weights over the two class-weight vectors of BCEWithLogitsLoss (train_mil.py:52-55), each None or
    [C] — or None when both are None (the caller then takes the unweighted entry).  Returns (struct, the tensors it points
    into: hold them until the call is enqueued)."""
    if pos_weight is None and weight is None:
        return None, ()
    keep = []
    for name, t in (("pos_weight", pos_weight), ("weight", weight)):
        if t is not None:
            t = _f32c(t.reshape(-1), name)
            if t.device != dev or t.numel() != C:
                raise ValueError(f"{name} must hold {C} elements on {dev} (got {t.numel()} on {t.device})")
        keep.append(t)
    return _native.BceWeights(*[(t.data_ptr() if t is not None else 0) for t in keep]), keep


def agg_loss_head(classes, pred, idx, label, pos_weight=None, weight=None):
    """dsmil_agg_loss_head: the training objective of one bag (train_tcga.py:67-71) and its logit gradients in one
    launch.  Returns (loss [] , max_pred [C], g_pred [C], g_max [C]).  ``pos_weight`` / ``weight`` ([C] fp32 each, or None):
    the class weights of BCEWithLogitsLoss(weight, pos_weight) (train_mil.py:52-55) — dsmil_agg_loss_head_w."""
    classes = _f32c(classes, "classes"); pred = _f32c(pred.reshape(-1), "pred")
    label = _f32c(label.reshape(-1).to(torch.float32), "label")
    idx = _i64c(idx.reshape(-1), "idx")
    C = classes.shape[1]
    dev = classes.device
    out = torch.empty((1 + 3 * C,), dtype=torch.float32, device=dev)
    loss, max_pred, g_pred, g_max = out[0:1], out[1:1 + C], out[1 + C:1 + 2 * C], out[1 + 2 * C:]
    bw, keep = _bce_weights(pos_weight, weight, C, dev)
    with torch.cuda.device(dev):
        if bw is None:
            entry = "dsmil_agg_loss_head"
            rc = _native.lib().dsmil_agg_loss_head(_ptr(classes), _ptr(pred), _ptr(idx), _ptr(label), C, _ptr(loss),
                                                   _ptr(max_pred), _ptr(g_pred), _ptr(g_max), _stream(dev))
        else:
            entry = "dsmil_agg_loss_head_w"
            rc = _native.lib().dsmil_agg_loss_head_w(_ptr(classes), _ptr(pred), _ptr(idx), _ptr(label), C, _ptr(loss),
                                                     _ptr(max_pred), _ptr(g_pred), _ptr(g_max), ctypes.byref(bw), _stream(dev))
    _native.check(rc, entry)
    del keep
    return loss.reshape(()), max_pred, g_pred, g_max


def _agg_backward(lengths, offsets, feats, w, A, B, idx, g_pred, g_classes, g_A, g_B, vals, nonlinear, want_g_vals, g_max,
                  row_map, want_g_feats):
    """The body of agg_backward (``lengths`` None: ONE bag, dsmil_agg_backward_ex, or dsmil_agg_backward_rows for the input
    rows' gradient) and of agg_backward_bags (a batch: dsmil_agg_backward_bags).  The entries launch different kernels.
    bf16-stored rows take dsmil_agg_backward_bags_bf16 (a lone bag as a batch of one) with the bf16-rounded weight set of
    the forward (_bf16_params: the same cache entry): the gradient of what agg_forward computed on those rows, in fp32."""
    bf16 = feats.dtype == torch.bfloat16
    if bf16:
        if row_map is not None:
            raise ValueError("row_map is implemented for the fp32 path")
        if want_g_feats:
            raise ValueError("the gradient of the input rows is implemented for the fp32 path")
        if not feats.is_cuda:
            raise RuntimeError("feats must be a CUDA(HIP) tensor for the native path")
        feats = feats if feats.is_contiguous() else feats.contiguous()
        w = _bf16_params(w, nonlinear, feats.device)[0]
        if lengths is None:
            lengths = [feats.shape[0]]
    else:
        feats = _f32c(feats, "feats")
    dev = feats.device
    N, K = feats.shape
    row_map = _i64c(row_map, "row_map")
    if row_map is not None:
        N = int(row_map.numel())
    if vals is None:
        vals = feats
    else:
        vals = vals.to(torch.bfloat16).contiguous() if bf16 else _f32c(vals, "vals")
    Kv = vals.shape[1]
    p, keep, C = _agg_params(w, K, Kv, nonlinear)
    A = _f32c(A, "A"); B = _f32c(B, "B")
    g_classes = _f32c(g_classes, "g_classes"); g_A = _f32c(g_A, "g_A"); g_B = _f32c(g_B, "g_B")
    L = _native.lib()
    if lengths is None:
        entry = "dsmil_agg_backward_rows" if want_g_feats else "dsmil_agg_backward_ex"
        extent, per_bag = (N,), (-1,)
        idx = idx.contiguous()
        nbytes = L.dsmil_agg_backward_workspace_bytes(N, K, Kv, C)
    else:
        entry = "dsmil_agg_backward_bags_bf16" if bf16 else "dsmil_agg_backward_bags"
        lengths = [int(n) for n in lengths]
        if sum(lengths) != N or any(n <= 0 for n in lengths):
            raise ValueError(f"bag lengths must be positive and sum to {N}")
        off = offsets if offsets is not None else offsets_tensor(lengths, dev)
        extent, per_bag = (_ptr(off), len(lengths), N, max(lengths)), (len(lengths), C)
        idx = _i64c(idx.reshape(per_bag), "idx")
        nbytes = getattr(L, entry + "_workspace_bytes")(len(lengths), N, K, Kv, C)
    g_pred = _f32c(g_pred.reshape(per_bag), "g_pred")
    g_max = _f32c(g_max.reshape(per_bag), "g_max") if g_max is not None else None
    new = lambda *shape: torch.empty(shape, dtype=torch.float32, device=dev)
    out = {"q0_w": new(Q_DIM, K), "q0_b": new(Q_DIM), "fcc_w": new(C, C, Kv), "fcc_b": new(C)}
    if nonlinear:
        out["q2_w"], out["q2_b"] = new(Q_DIM, Q_DIM), new(Q_DIM)
    if g_classes is not None or g_max is not None:
        out["fc_w"], out["fc_b"] = new(C, K), new(C)
    g = _native.AggGrads(*[(out[k].data_ptr() if k in out else 0) for k in W_KEYS])
    g_vals = new(N, Kv) if want_g_vals else None
    g_feats = new(N, K) if want_g_feats else None
    ws = _workspace(dev, nbytes)
    # (the bf16 entry has neither a row map nor a row-gradient argument; dsmil_agg_backward_ex no row-gradient argument)
    rmap = () if bf16 else (_ptr(row_map),)
    tail = () if bf16 or entry == "dsmil_agg_backward_ex" else (_ptr(g_feats),)
    with torch.cuda.device(dev):
        rc = getattr(L, entry)(_ptr(feats), _ptr(vals), *extent, ctypes.byref(p), _ptr(A), _ptr(B), _ptr(idx), _ptr(g_classes),
                               _ptr(g_max), _ptr(g_pred), _ptr(g_A), _ptr(g_B), ctypes.byref(g), _ptr(g_vals), *rmap,
                               _ptr(ws), ws.numel(), _stream(dev), *tail)
    _native.check(rc, entry)
    del keep
    if want_g_feats:
        out["feats"] = g_feats
    if want_g_vals:
        out["vals"] = g_vals
    return out


def agg_backward(feats, w, A, B, idx, g_pred, g_classes=None, g_A=None, g_B=None, vals=None, nonlinear=True,
                 want_g_vals=False, g_max=None, row_map=None, want_g_feats=False):
    """dsmil_agg_backward: parameter gradients of FCLayer + BClassifier for ONE bag (what autograd
    derives for train_tcga.py:67-72).  feats [N,K] fp32 CUDA (or bf16: dsmil_agg_backward_bags_bf16 on a batch of one, the
    gradient at the bf16 rows and the bf16-rounded weights, fp32 results; no row_map, no want_g_feats), w as in agg_forward, A [N,C], B [1,C,Kv],
    idx [1,C] = the forward's outputs; g_* = upstream gradients (None = zero).  Returns a dict with the
    gradient of every key of ``w`` (fc_* only when g_classes or g_max is given, q2_* only when nonlinear) and
    ``vals`` (when want_g_vals).  ``g_max`` [C]: the sparse gradient of max_n classes[n,:] (the training objective's
    instance stream); ``row_map``: see agg_forward (N = its length).  ``want_g_feats``: also return ``feats``, the
    gradient of the input rows [N,K] in LOGICAL row order (dsmil_agg_backward_rows, one more launch: k_bwd_gx); with
    caller-supplied ``vals`` it leaves out the value stream's share (value_proj_backward_rows adds that).  A call without
    it is dsmil_agg_backward_ex as before."""
    return _agg_backward(None, None, feats, w, A, B, idx, g_pred, g_classes, g_A, g_B, vals, nonlinear, want_g_vals, g_max,
                         row_map, want_g_feats)


def agg_loss_head_bags(classes, lengths, pred, idx, labels, offsets=None, pos_weight=None, weight=None):
    """dsmil_agg_loss_head_bags: the objective of ``agg_loss_head`` for every bag of a batch stored back to back, one
    launch.  classes [total,C], pred / idx / labels [n_bags,C] (the batched forward's outputs; labels 0/1).  Returns
    (loss [n_bags], max_pred [n_bags,C], g_pred [n_bags,C], g_max [n_bags,C]) — the gradients of each bag's OWN loss.
    ``pos_weight`` / ``weight`` as in ``agg_loss_head``: dsmil_agg_loss_head_bags_w."""
    classes = _f32c(classes, "classes")
    n, C = len(lengths), classes.shape[1]
    pred = _f32c(pred.reshape(n, C), "pred")
    labels = _f32c(labels.reshape(n, C).to(torch.float32), "labels")
    idx = _i64c(idx.reshape(n, C), "idx")
    dev = classes.device
    off = offsets if offsets is not None else offsets_tensor(lengths, dev)
    loss = torch.empty((n,), dtype=torch.float32, device=dev)
    max_pred, g_pred, g_max = (torch.empty((n, C), dtype=torch.float32, device=dev) for _ in range(3))
    bw, keep = _bce_weights(pos_weight, weight, C, dev)
    with torch.cuda.device(dev):
        if bw is None:
            entry = "dsmil_agg_loss_head_bags"
            rc = _native.lib().dsmil_agg_loss_head_bags(_ptr(classes), _ptr(off), _ptr(pred), _ptr(idx), _ptr(labels), n, C,
                                                        _ptr(loss), _ptr(max_pred), _ptr(g_pred), _ptr(g_max), _stream(dev))
        else:
            entry = "dsmil_agg_loss_head_bags_w"
            rc = _native.lib().dsmil_agg_loss_head_bags_w(_ptr(classes), _ptr(off), _ptr(pred), _ptr(idx), _ptr(labels), n, C,
                                                          _ptr(loss), _ptr(max_pred), _ptr(g_pred), _ptr(g_max),
                                                          ctypes.byref(bw), _stream(dev))
    _native.check(rc, entry)
    del keep
    return loss, max_pred, g_pred, g_max


def agg_backward_bags(feats, lengths, w, A, B, idx, g_pred, g_classes=None, g_A=None, g_B=None, vals=None, nonlinear=True,
                      want_g_vals=False, g_max=None, row_map=None, want_g_feats=False, offsets=None):
    """dsmil_agg_backward_bags: the backward of ``agg_forward`` over a BATCH of bags stored back to back (minibatch
    training: one summed gradient over the bags).  ``lengths``: the bags' LOGICAL row counts; A [total,C], B [n,C,Kv],
    idx [n,C] = the batched forward's outputs; g_pred [n,C], g_max [n,C] or None, g_classes / g_A [total,C], g_B [n,C,Kv]
    (None = zero).  Returns the dict of ``agg_backward``: every parameter gradient summed over the bags, ``vals`` /
    ``feats`` (on request) laid end to end in logical row order.  bf16 ``feats``: dsmil_agg_backward_bags_bf16 (see
    ``agg_backward``)."""
    return _agg_backward(lengths, offsets, feats, w, A, B, idx, g_pred, g_classes, g_A, g_B, vals, nonlinear, want_g_vals,
                         g_max, row_map, want_g_feats)


def _step_operands(what, params, exp_avg, exp_avg_sq, K, C, nonlinear, step, lr, betas, eps, weight_decay):
    """struct dsmil_agg_params over the eight ``params`` and struct dsmil_adam_state over their moments for the one-call
    training steps.  Returns (params struct, state struct, the pointer arrays the state points into: hold them until the
    call is enqueued)."""
    for t in list(params) + list(exp_avg) + list(exp_avg_sq):
        if t is not None and not (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()):
            raise RuntimeError(f"{what}: parameters and Adam moments must be contiguous fp32 CUDA tensors")
    ptr = lambda t: (t.data_ptr() if t is not None else 0)
    p = _native.AggParams(*[ptr(t) for t in params], K, K, C, 1 if nonlinear else 0)
    arr = ctypes.c_void_p * 8
    m_arr, v_arr = arr(*[ptr(t) for t in exp_avg]), arr(*[ptr(t) for t in exp_avg_sq])
    st = _native.AdamState(ctypes.cast(m_arr, ctypes.POINTER(ctypes.c_void_p)), ctypes.cast(v_arr, ctypes.POINTER(ctypes.c_void_p)),
                           int(step), float(lr), float(betas[0]), float(betas[1]), float(eps), float(weight_decay))
    return p, st, (m_arr, v_arr)


def agg_train_step(feats, label, params, exp_avg, exp_avg_sq, step, lr, betas, eps, weight_decay, nonlinear=True,
                   row_map=None, loss_out=None):
    """dsmil_agg_train_step: one train_tcga.py:60-75 step (forward, 0.5 BCE(bag) + 0.5 BCE(max instance), backward,
    Adam) as ONE native call.  ``params`` / ``exp_avg`` / ``exp_avg_sq``: the eight tensors in the order fc_w, fc_b, q0_w,
    q0_b, q2_w, q2_b, fcc_w, fcc_b (None for q2_* of a linear query) — parameters and moments are updated IN PLACE.
    ``step`` = 1-based index of this update.  Returns the loss as a 1-element device tensor (no host sync)."""
    feats = _f32c(feats, "feats")
    dev = feats.device
    rows, K = feats.shape
    row_map = _i64c(row_map, "row_map")
    N = int(row_map.numel()) if row_map is not None else rows
    label = _f32c(label.reshape(-1).to(torch.float32), "label")
    C = int(label.numel())
    p, st, keep = _step_operands("agg_train_step", params, exp_avg, exp_avg_sq, K, C, nonlinear, step, lr, betas, eps, weight_decay)
    loss = loss_out if loss_out is not None else torch.empty((1,), dtype=torch.float32, device=dev)
    L = _native.lib()
    ws = _workspace(dev, L.dsmil_agg_train_step_workspace_bytes(N, K, C, 1 if nonlinear else 0))
    with torch.cuda.device(dev):
        rc = L.dsmil_agg_train_step(_ptr(feats), N, _ptr(row_map), _ptr(label), ctypes.byref(p), ctypes.byref(st), _ptr(loss),
                                    _ptr(ws), ws.numel(), _stream(dev))
    _native.check(rc, "dsmil_agg_train_step")
    del keep
    return loss


def agg_train_step_bags(feats, lengths, labels, params, exp_avg, exp_avg_sq, step, lr, betas, eps, weight_decay,
                        nonlinear=True, row_map=None, offsets=None, pos_weight=None, weight=None):
    """dsmil_agg_train_step_bags / dsmil_agg_train_step_bags_bf16 (by ``feats.dtype``): ONE optimiser step on a batch of
    bags stored back to back as ONE native call — batched forward, the mean over the bags of ``agg_train_step``'s objective,
    batched backward, Adam.  ``lengths``: the bags' LOGICAL row counts; labels [n_bags, C]; ``params`` / ``exp_avg`` /
    ``exp_avg_sq`` / ``step`` as in ``agg_train_step`` (updated IN PLACE).  ``row_map``: int64 [sum(lengths)] as in
    ``agg_forward``; the bf16 entry has none, so bf16 rows are gathered by one index_select in front of the call (as
    MILNet.batch_loss does).  ``pos_weight`` / ``weight`` as in ``agg_loss_head``: the ``_w`` form of the same entry (same
    launches, same workspace).  Returns (loss [1], loss_each [n_bags]) as device tensors (no host sync)."""
    bf16 = feats.dtype == torch.bfloat16
    if not feats.is_cuda:
        raise RuntimeError("feats must be a CUDA(HIP) tensor for the native path")
    row_map = _i64c(row_map, "row_map")
    if bf16:
        if row_map is not None:
            feats, row_map = feats.index_select(0, row_map), None
        feats = feats if feats.is_contiguous() else feats.contiguous()
    else:
        feats = _f32c(feats, "feats")
    dev = feats.device
    rows, K = feats.shape
    total = int(row_map.numel()) if row_map is not None else rows
    lengths = [int(n) for n in lengths]
    n = len(lengths)
    if n < 1 or sum(lengths) != total or any(m <= 0 for m in lengths):
        raise ValueError(f"bag lengths must be positive and sum to {total}")
    labels = _f32c(labels.reshape(n, -1).to(torch.float32), "labels")
    C = int(labels.shape[1])
    p, st, keep = _step_operands("agg_train_step_bags", params, exp_avg, exp_avg_sq, K, C, nonlinear, step, lr, betas, eps,
                                 weight_decay)
    off = offsets if offsets is not None else offsets_tensor(lengths, dev)
    out = torch.empty((1 + n,), dtype=torch.float32, device=dev)
    loss, each = out[0:1], out[1:]
    L = _native.lib()
    entry = "dsmil_agg_train_step_bags_bf16" if bf16 else "dsmil_agg_train_step_bags"
    ws = _workspace(dev, getattr(L, entry + "_workspace_bytes")(n, total, K, C, 1 if nonlinear else 0))
    rmap = () if bf16 else (_ptr(row_map),)
    bw, keep_w = _bce_weights(pos_weight, weight, C, dev)
    tail = ()
    if bw is not None:
        entry, tail = entry + "_w", (ctypes.byref(bw),)
    with torch.cuda.device(dev):
        rc = getattr(L, entry)(_ptr(feats), _ptr(off), n, total, max(lengths), *rmap, _ptr(labels), ctypes.byref(p),
                               ctypes.byref(st), _ptr(each), _ptr(loss), _ptr(ws), ws.numel(), *tail, _stream(dev))
    _native.check(rc, entry)
    del keep, keep_w
    return loss, each


def adam_step(params, grads, exp_avg, exp_avg_sq, step, lr, betas, eps, weight_decay):
    """dsmil_adam_step: torch.optim.Adam's update (amsgrad = maximize = False) of up to 8 tensors in one launch, in place."""
    n = len(params)
    arr = ctypes.c_void_p * n
    cast = lambda ts: ctypes.cast(arr(*[t.data_ptr() for t in ts]), ctypes.POINTER(ctypes.c_void_p))
    numel = (ctypes.c_int64 * n)(*[int(t.numel()) for t in params])
    dev = params[0].device
    with torch.cuda.device(dev):
        rc = _native.lib().dsmil_adam_step(n, cast(params), cast(grads), cast(exp_avg), cast(exp_avg_sq), numel, int(step),
                                           float(lr), float(betas[0]), float(betas[1]), float(eps), float(weight_decay), _stream(dev))
    _native.check(rc, "dsmil_adam_step")


# ---------------------------------------------------------------------------------------------
# patch embedder (ResNet-18 + InstanceNorm) — compute_feats.py:146-170,211 / dsmil.py:21-25
# ---------------------------------------------------------------------------------------------
_pack_cache = _LRU()


def resnet_conv_shapes(depth):
    """Shapes of the bias-free convs of a torchvision ResNet in state_dict order (mirror of make_arch in
    csrc/resnet_fwd.hip): BasicBlock depth 18 -> 20 tensors, 34 -> 36; Bottleneck depth 50 -> 53, 101 -> 104."""
    nblk = {18: (2, 2, 2, 2), 34: (3, 4, 6, 3), 50: (3, 4, 6, 3), 101: (3, 4, 23, 3)}[depth]
    shapes = [(64, 3, 7, 7)]
    cin = 64
    for l, n in enumerate(nblk):
        c = 64 << l
        for b in range(n):
            if depth >= 50:
                shapes += [(c, cin, 1, 1), (c, c, 3, 3), (4 * c, c, 1, 1)]
                if b == 0:
                    shapes.append((4 * c, cin, 1, 1))
                cin = 4 * c
            else:
                shapes += [(c, cin, 3, 3), (c, c, 3, 3)]
                if l > 0 and b == 0:
                    shapes.append((c, cin, 1, 1))
                cin = c
    return shapes


RESNET18_SHAPES = resnet_conv_shapes(18)
RESNET_DEPTHS = (18, 34, 50, 101)


def resnet_depth_of(convs):
    """18 / 34 / 50 / 101 when the conv list has exactly that architecture's shapes and order, else None."""
    for depth in RESNET_DEPTHS:
        sh = resnet_conv_shapes(depth)
        if len(convs) == len(sh) and all(tuple(w.shape) == t for w, t in zip(convs, sh)):
            return depth
    return None


RESNET_MAX_ABS_WEIGHT = 100.0   # < 65504 / (2^8 * 2.25): see _packed_resnet_weights


def _packed_resnet_weights(convs, depth=18, precision=0):
    """Device buffer with the non-stem conv weights re-laid-out for the kernels (dsmil_resnet_pack:
    Winograd-transformed or [tap][Cout][Cin]).  Cached per weight set; rebuilt when any tensor was
    modified in place (``_version``), re-assigned or moved (``data_ptr``) — _cached."""
    dev = convs[0].device
    key = (str(dev), depth, int(precision)) + tuple(_tkey(w) for w in convs)
    keep = []   # the contiguous fp32 weights the pack call reads: the entry holds them next to the source tensors

    def make():
        L = _native.lib()
        nbytes = L.dsmil_resnet_packed_bytes_ex(depth, int(precision))
        if nbytes == 0:
            raise ValueError(f"precision {precision} is not implemented for a depth-{depth} trunk "
                             "(the bf16-activation trunk: ResNet-18 / 34 with InstanceNorm)")
        buf = torch.empty((nbytes + 3) // 4, dtype=torch.float32, device=dev)
        keep.extend(_f32c(w.detach(), "conv weight") for w in convs)
        # The conv operands are cut into fp16 planes of the 2^8-scaled weights (csrc/resnet_fwd.hip, EMB_WSHIFT); a Winograd
        # weight transform grows a 3x3 kernel by at most 2.25x, so |w| must stay below 65504 / (256 * 2.25) = 113.7 or a plane
        # overflows to inf.  Checked ONCE per weight set (this function is cached on the weights' versions): one host read.
        wmax = float(torch.stack([w.abs().amax() for w in keep]).amax())
        if not wmax < RESNET_MAX_ABS_WEIGHT:   # (also catches NaN)
            raise ValueError(f"conv weight magnitude {wmax:g} is outside the native embedder's range (|w| < {RESNET_MAX_ABS_WEIGHT:g}: "
                             "its operands are fp16 planes of the 2^8-scaled weights)")
        arr = (ctypes.c_void_p * len(keep))(*[t.data_ptr() for t in keep])
        with torch.cuda.device(dev):
            rc = L.dsmil_resnet_pack_ex(depth, arr, _ptr(buf), int(precision), _stream(dev))
        _native.check(rc, "dsmil_resnet_pack_ex")
        return (buf,)
    return _cached(_pack_cache, key, dev, (keep, list(convs)), make)[0]


_bn_cache = _LRU()
_bn_checked = _LRU()
_f16_trunk_ok = _LRU()     # weight set -> its fp16-activation trunk produced finite features (checked once)


def _folded_bn(norms, dev):
    """Fold the trunk's eval-mode BatchNorm2d modules into y = (x - m) * r, concatenated in conv order (cached on the
    parameter / buffer versions)."""
    key = (str(dev),) + tuple((id(n), _tkey(n.running_mean), _tkey(n.running_var), _tkey(n.weight), _tkey(n.bias), n.eps)
                              for n in norms)

    def make():
        ms, rs = [], []
        for n in norms:
            var = n.running_var.detach().to(dev, torch.float64)
            mean = n.running_mean.detach().to(dev, torch.float64)
            w = n.weight.detach().to(dev, torch.float64) if n.weight is not None else torch.ones_like(var)
            b = n.bias.detach().to(dev, torch.float64) if n.bias is not None else torch.zeros_like(var)
            r = w / torch.sqrt(var + n.eps)
            if bool((r == 0).any()):
                raise NotImplementedError("a BatchNorm channel with weight 0 cannot be folded into (x - m) * r")
            ms.append(mean - b / r)
            rs.append(r)
        return torch.cat(ms).to(torch.float32).contiguous(), torch.cat(rs).to(torch.float32).contiguous()
    return _cached(_bn_cache, key, dev, list(norms), make)   # (m, r); the modules stay alive: their ids stay unique


def resnet18in_forward(x, convs, fc_w=None, fc_b=None, bn_norms=None, precision="fp32"):
    """x: [B,3,H,W] fp32 CUDA in [0,1] (what VF.to_tensor yields), OR decoded images as uint8
    [B,H,W,3] CUDA (the /255 + HWC->CHW of to_tensor is then fused into the stem, bit-identically);
    convs: the trunk's conv weights in torchvision state_dict order (20 for ResNet-18, 36 for ResNet-34, 53 for
    ResNet-50, 104 for ResNet-101).
    ``bn_norms``: the eval-mode BatchNorm2d modules of a `--norm_layer batch` trunk, in the same order;
    None = InstanceNorm.  One native launch sequence (dsmil_resnet_forward_ex).
    ``precision``: "fp32" (default: fp32-class, the parity path); "half" (OPT-IN reduced precision, <= 5e-3 feature error, not
    the 1e-4 bar): fp16 ACTIVATIONS behind the stem, one fp16 MFMA product per MAC, f32 accumulation and InstanceNorm statistics
    (round 6, csrc/resnet_b16.h: ResNet-18 / 34 InstanceNorm trunks, ~2.6e-3, 2x the fp32 path) — and where that trunk does not
    apply (frozen BatchNorm, Bottleneck trunks, patches under 64 x 64 or wider than ~1000 pixels, weights whose conv sums leave
    fp16's range) the older form: fp32 activations, every conv operand rounded to one fp16 plane (~2.6e-3, 1.2x); "bf16"
    (OPT-IN): the same trunk on bf16 activations — fp32's range, 8 significant bits: ~2e-2 feature error; include/dsmil_hip.h.
    Returns (feats [B,512 | 2048], classes [B,C] or None)."""
    if precision not in ("fp32", "half", "bf16"):
        raise ValueError("precision must be 'fp32', 'half' or 'bf16'")
    prec = {"fp32": 0, "half": 1, "bf16": 2}[precision]
    if prec == 2 and bn_norms is not None:
        raise ValueError("precision 'bf16' is implemented for InstanceNorm trunks")
    u8 = x.dtype == torch.uint8
    if u8:
        if not x.is_cuda:
            raise RuntimeError("x must be a CUDA(HIP) tensor for the native path")
        if x.dim() != 4 or x.shape[3] != 3:
            raise ValueError(f"uint8 patches must be NHWC [B,H,W,3], got {tuple(x.shape)}")
        x = x if x.is_contiguous() else x.contiguous()
        B, H, W, _ = x.shape
    else:
        x = _f32c(x, "x")
        if x.dim() != 4 or x.shape[1] != 3:
            raise ValueError(f"expected [B,3,H,W] patches, got {tuple(x.shape)}")
        B, _, H, W = x.shape
    depth = resnet_depth_of(convs)
    if depth is None:
        raise ValueError("conv weights do not have the ResNet-18 / 34 / 50 / 101 shapes and order")
    dev = x.device
    L = _native.lib()
    feats = torch.empty((B, L.dsmil_resnet_feature_dim(depth)), dtype=torch.float32, device=dev)
    if B == 0:
        return feats, (torch.empty((0, fc_w.shape[0]), device=dev) if fc_w is not None else None)
    fc_w = _f32c(fc_w.detach(), "fc_w") if fc_w is not None else None
    fc_b = _f32c(fc_b.detach(), "fc_b") if fc_b is not None else None
    C = fc_w.shape[0] if fc_w is not None else 0
    classes = torch.empty((B, C), dtype=torch.float32, device=dev) if fc_w is not None else None
    conv1 = _f32c(convs[0].detach(), "conv1.weight")
    nbytes = L.dsmil_resnet_workspace_bytes(depth, B, H, W)
    if nbytes == 0:
        raise ValueError(f"unsupported patch size {H}x{W}")
    ws = _workspace(dev, nbytes)
    bn_m = bn_r = None
    if bn_norms is not None:
        bn_m, bn_r = _folded_bn(bn_norms, dev)
        if bn_m.numel() != L.dsmil_resnet_norm_channels(depth):
            raise ValueError("BatchNorm channel counts do not match the trunk")

    def run(p):
        packed = _packed_resnet_weights(convs, depth, p)
        with torch.cuda.device(dev):
            return packed, L.dsmil_resnet_forward_ex(depth, _ptr(x), 1 if u8 else 0, B, H, W, _ptr(conv1), _ptr(packed), _ptr(bn_m),
                                                     _ptr(bn_r), _ptr(fc_w), _ptr(fc_b), C, _ptr(feats), _ptr(classes), _ptr(ws),
                                                     ws.numel(), p, _stream(dev))

    rc = None
    if prec == 1 and bn_norms is None and L.dsmil_resnet_packed_bytes_ex(depth, 3) != 0:
        # "half": the fp16-ACTIVATION trunk (precision 3) where it applies ...
        wkey = ("f16act",) + tuple(_tkey(w) for w in convs)
        ent = _f16_trunk_ok.get(wkey)              # (ok, the weights: an entry keeps its sources alive, so a freed tensor's address
        state = None if ent is None else ent[0]    # cannot come back as another model's)  None: not tried, True / False: checked once
        if state is not False:
            packed, rc = run(3)
            if rc == _native.DSMIL_E_UNSUPPORTED:  # (patch size outside the trunk's range)
                rc = None
            elif rc == 0 and state is None:
                # fp16 activations: the conv sums of THIS weight set must stay inside +-65504 — checked on its first forward
                # (one host read per weight set); a set that leaves the range keeps the one-plane form below
                ok = bool(torch.isfinite(feats).all())
                _f16_trunk_ok.put(wkey, (ok, list(convs)))
                if not ok:
                    rc = None
    if rc is None:   # ... else (and for every other precision) the form the caller named
        packed, rc = run(prec)
    _native.check(rc, "dsmil_resnet_forward_ex")
    if bn_norms is not None:
        # A frozen-BatchNorm trunk has no bound on its activations (InstanceNorm output is bounded by sqrt(H W)); an activation
        # past fp16's 65504 would turn into inf / NaN features.  The FIRST forward of every folded-BatchNorm set is checked
        # (one host read per weight set, none afterwards).
        key = ("bn_finite", bn_m.data_ptr(), bn_m._version, packed.data_ptr())
        if _bn_checked.get(key) is None:
            if not bool(torch.isfinite(feats).all()):
                raise FloatingPointError("the frozen-BatchNorm trunk produced non-finite features: an activation left the fp16 "
                                         "operand range of the native conv kernels (|a| < 65504)")
            _bn_checked.put(key, True)
    return feats, classes


# ---- the ctypes glue the embedder's stage, conv-backward and norm-backward wrappers below share ----
_REFUSALS = {"dsmil_trunk16": "shape outside what the 16-bit trunk's kernels implement",       # by the entry family's prefix
             "dsmil_trunk32": "shape or precision outside what the fp32-class trunk's kernels implement",
             "dsmil_conv_bwd": "shape outside what the conv backward kernels implement",
             "dsmil_norm_bwd": "shape outside what the norm backward kernels implement",
             "dsmil_stem_pool_bwd": "shape outside what the stem's norm / pool backward kernels implement"}


def _refused(rc, what):
    """Raises for a non-zero rc of entry ``what``: NotImplementedError for DSMIL_E_UNSUPPORTED, else as _native.check."""
    if rc == _native.DSMIL_E_UNSUPPORTED:
        raise NotImplementedError(f"{what}: {next(v for k, v in _REFUSALS.items() if what.startswith(k))}")
    _native.check(rc, what)


def _scratch(dev, need, ws=None):
    """A workspace of ``need`` bytes: a fresh one (256 bytes at least), or the caller's ``ws`` once seen to be large enough."""
    if ws is None:
        return torch.empty(max(int(need), 256), dtype=torch.uint8, device=dev)
    if not ws.is_cuda or ws.dtype != torch.uint8 or not ws.is_contiguous() or ws.numel() < need:
        raise RuntimeError(f"ws must be a contiguous uint8 CUDA(HIP) tensor of at least {need} bytes")
    return ws


def _plan(entry, fields, *args, what=None):
    """The 16 int32 plan entry ``entry`` writes behind ``args``, as a dict of ``fields``; a refusal raises as ``what``'s."""
    out = (ctypes.c_int32 * 16)()
    _refused(getattr(_native.lib(), entry)(*args, out), what or entry)
    return dict(zip(fields, list(out)))


def _size_or_reason(need, plan_entry, what, *args):
    """``need`` as a size query answered it — or, where it answered 0, the refusal of the plan entry that knows why."""
    if need == 0:
        _plan(plan_entry, (), *args, what=what)
    return need


def _conv_out(H, W, ks, stride, pad):      # (emb::outdim, csrc/emb_host.h)
    return (H + 2 * pad - ks) // stride + 1, (W + 2 * pad - ks) // stride + 1


# ---------------------------------------------------------------------------------------------
# the stages of the 16-bit activation trunk ALONE (csrc/resnet_b16.h behind dsmil_trunk16_*): FOR TESTS — no product path
# calls these.  16-bit maps are int16 tensors [positions(B,H,W), C] holding the raw bf16 / fp16 bits in the shared-border
# layout (include/dsmil_hip.h); uint16 tensors are taken as well.  A shape the kernels do not take raises NotImplementedError
# (DSMIL_E_UNSUPPORTED), every other refusal RuntimeError; nothing is launched in either case.
# ---------------------------------------------------------------------------------------------
TRUNK16_KINDS = {"bf16": 1, "fp16": 2}


def _t16_buf(t, name):
    if not t.is_cuda or t.dtype not in (torch.int16, torch.uint16) or not t.is_contiguous():
        raise RuntimeError(f"{name} must be a contiguous int16 / uint16 CUDA(HIP) tensor")
    return t


def trunk16_positions(B, H, W):
    """Positions of a [B,H,W] map in the shared-border layout: B (H+1) (W+1) + (W+1)."""
    return int(_native.lib().dsmil_trunk16_positions(B, H, W))


def trunk16_layout(x_nhwc, kind, borders_only=False):
    """k_b16_pad: fp32 NHWC [B,H,W,C] -> the 16-bit shared-border buffer; ``borders_only``: a buffer of bytes 0x3C of that
    shape with only k_b16_borders run on it (x supplies the shape and the device)."""
    x = _f32c(x_nhwc, "x_nhwc")
    B, H, W, C = x.shape
    out = torch.empty((trunk16_positions(B, H, W), C), dtype=torch.int16, device=x.device)
    with torch.cuda.device(x.device):
        rc = _native.lib().dsmil_trunk16_layout(_ptr(x), _ptr(out), B, H, W, C, TRUNK16_KINDS[kind], 1 if borders_only else 0,
                                                _stream(x.device))
    _refused(rc, "dsmil_trunk16_layout")
    return out


def trunk16_conv(buf, w, B, Hi, Wi, stride, pad, kind):
    """k_pack_b16 + b16::run_conv: buf [positions(B,Hi,Wi), Cin], w fp32 OIHW -> (out [positions(B,Ho,Wo), Cout], Ho, Wo)."""
    buf, w = _t16_buf(buf, "buf"), _f32c(w, "w")
    Cout, Cin, ks, _ = w.shape
    if tuple(buf.shape) != (trunk16_positions(B, Hi, Wi), Cin):
        raise ValueError(f"buf {tuple(buf.shape)} is not a [{B},{Hi},{Wi},{Cin}] map in the shared-border layout")
    Ho, Wo = _conv_out(Hi, Wi, ks, stride, pad)
    L = _native.lib()
    ws = _scratch(buf.device, L.dsmil_trunk16_conv_workspace_bytes(Cin, Cout, ks))
    out = torch.empty((max(trunk16_positions(B, Ho, Wo), 1), Cout), dtype=torch.int16, device=buf.device)
    with torch.cuda.device(buf.device):
        rc = L.dsmil_trunk16_conv(_ptr(buf), _ptr(w), _ptr(out), B, Hi, Wi, Cin, Cout, ks, stride, pad, TRUNK16_KINDS[kind],
                                  _ptr(ws), ws.numel(), _stream(buf.device))
    _refused(rc, "dsmil_trunk16_conv")
    return out, Ho, Wo


def trunk16_norm(buf, B, H, W, kind, idn=None, relu=True, out=None):
    """run_stats + run_apply: [relu]((x - mean) rstd [+ idn]) per (image, channel).  ``out``: the buffer to write (``buf``
    itself for the trunk's in-place form); default a new one whose closing row — which the kernel does not write — is zero."""
    buf = _t16_buf(buf, "buf")
    C = buf.shape[1]
    if tuple(buf.shape) != (trunk16_positions(B, H, W), C):
        raise ValueError(f"buf {tuple(buf.shape)} is not a [{B},{H},{W},{C}] map in the shared-border layout")
    for t, name in ((idn, "idn"), (out, "out")):
        if t is not None and (_t16_buf(t, name).shape != buf.shape):
            raise ValueError(f"{name} must have buf's shape")
    y = torch.zeros_like(buf) if out is None else out
    L = _native.lib()
    ws = _scratch(buf.device, L.dsmil_trunk16_norm_workspace_bytes(B, C))
    with torch.cuda.device(buf.device):
        rc = L.dsmil_trunk16_norm(_ptr(buf), _ptr(idn), _ptr(y), B, H, W, C, 1 if relu else 0, TRUNK16_KINDS[kind], _ptr(ws),
                                  ws.numel(), _stream(buf.device))
    _refused(rc, "dsmil_trunk16_norm")
    return y


def trunk16_pool(buf, idn, B, H, W, kind):
    """run_stats + k_pool_b16: fp32 [B,C] = mean over pixels of relu((x - mean) rstd + idn)."""
    buf, idn = _t16_buf(buf, "buf"), _t16_buf(idn, "idn")
    C = buf.shape[1]
    if tuple(buf.shape) != (trunk16_positions(B, H, W), C) or idn.shape != buf.shape:
        raise ValueError(f"buf / idn are not [{B},{H},{W},{C}] maps in the shared-border layout")
    L = _native.lib()
    ws = _scratch(buf.device, L.dsmil_trunk16_norm_workspace_bytes(B, C))
    feats = torch.empty((B, C), dtype=torch.float32, device=buf.device)
    with torch.cuda.device(buf.device):
        rc = L.dsmil_trunk16_pool(_ptr(buf), _ptr(idn), _ptr(feats), B, H, W, C, TRUNK16_KINDS[kind], _ptr(ws), ws.numel(),
                                  _stream(buf.device))
    _refused(rc, "dsmil_trunk16_pool")
    return feats


def trunk16_forward(x_nhwc, convs, kind):
    """pack_all + b16::trunk: fp32 NHWC [B,Hp,Wp,64] (what the stem hands over) and the trunk's conv weights in state_dict
    order (the stem's first: it is not read) -> fp32 features [B,512]."""
    x = _f32c(x_nhwc, "x_nhwc")
    B, Hp, Wp, C = x.shape
    depth = resnet_depth_of(convs)
    if C != 64 or depth not in (18, 34):
        raise ValueError("the 16-bit trunk takes a 64-channel map and the conv weights of a ResNet-18 / 34")
    L = _native.lib()
    keep = [_f32c(w.detach(), "conv weight") for w in convs]
    arr = (ctypes.c_void_p * len(keep))(*[t.data_ptr() for t in keep])
    ws = _scratch(x.device, L.dsmil_trunk16_workspace_bytes(depth, B, Hp, Wp))
    feats = torch.empty((B, L.dsmil_resnet_feature_dim(depth)), dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        rc = L.dsmil_trunk16_forward(depth, _ptr(x), B, Hp, Wp, arr, _ptr(feats), TRUNK16_KINDS[kind], _ptr(ws), ws.numel(),
                                     _stream(x.device))
    _refused(rc, "dsmil_trunk16_forward")
    return feats


# ---------------------------------------------------------------------------------------------
# the stages of the fp32-class trunk ALONE (csrc/resnet_fwd.hip, csrc/wino_w1.h behind dsmil_trunk32_*).  The TRAINING forward is
# composed from them (simclr.NativeConv2d: trunk32_conv; NativeBasicBlock: trunk32_conv, trunk32_tail; both ask
# trunk32_conv_supported); trunk32_conv_plan and trunk32_stem serve tests and tools only.  Maps are fp32 NHWC tensors,
# statistics fp32 [B,C].  precision "fp32" = the product form (two fp16 planes,
# three products), "half" = one fp16 plane.  A shape the kernels do not take raises NotImplementedError (DSMIL_E_UNSUPPORTED),
# every other refusal RuntimeError; nothing is launched in either case.
# ---------------------------------------------------------------------------------------------
TRUNK32_PRECISIONS = {"fp32": 0, "half": 1}
TRUNK32_KERNELS = {0: "w1", 1: "unit", 2: "s6", 3: "other"}
TRUNK32_TAILS = {"identity": 0, "down": 1, "pool": 2}
_T32_PLAN_FIELDS = ("kernel", "tile", "IB", "TYB", "TXB", "nby", "nbx", "Ho", "Wo", "nslots", "grid_x", "grid_y", "block", "products")


def trunk32_conv_plan(Cin, Cout, ks, stride, pad, B, H, W, norm=False, precision="fp32"):
    """What plan_conv decides for this conv on B maps of H x W (no device needed): a dict of ``kernel`` ("w1", "unit", "s6"),
    ``tile`` (direct: 42 / 22 / 24), the Winograd unit ``IB, TYB, TXB, nby, nbx``, ``Ho, Wo, nslots``, ``grid_x, grid_y, block``
    and ``products`` (plane products per MAC)."""
    d = _plan("dsmil_trunk32_conv_plan", _T32_PLAN_FIELDS, Cin, Cout, ks, stride, pad, B, H, W, 1 if norm else 0, TRUNK32_PRECISIONS[precision])
    d["kernel"] = TRUNK32_KERNELS[d["kernel"]]
    return d


def trunk32_conv_supported(Cin, Cout, ks, stride, pad, B, H, W, precision="fp32"):
    """True where dsmil_trunk32_conv takes the shape.  No device."""
    return _native.lib().dsmil_trunk32_conv_workspace_bytes(Cin, Cout, ks, stride, pad, B, H, W, TRUNK32_PRECISIONS[precision]) > 0


def trunk32_conv(x_nhwc, w, stride, pad, in_stats=None, frozen=None, precision="fp32"):
    """pack + run_conv: x fp32 NHWC [B,H,W,Cin], w fp32 OIHW -> (raw y [B,Ho,Wo,Cout], mean [B,Cout], rstd [B,Cout]).
    ``in_stats`` = (mean, rstd) [B,Cin]: x is raw and is staged as relu((x - mean) rstd); ``frozen`` = (m, r) [Cout]: the
    statistics are these per-channel values."""
    x, w = _f32c(x_nhwc, "x_nhwc"), _f32c(w, "w")
    B, H, W, Cin = x.shape
    Cout, Cin_w, ks, _ = w.shape
    if Cin_w != Cin:
        raise ValueError(f"w takes {Cin_w} input channels, x has {Cin}")
    im, ir = (_f32c(t, "in_stats") for t in in_stats) if in_stats is not None else (None, None)
    bm, br = (_f32c(t, "frozen") for t in frozen) if frozen is not None else (None, None)
    p = TRUNK32_PRECISIONS[precision]
    Ho, Wo = _conv_out(H, W, ks, stride, pad)
    L = _native.lib()
    ws = _scratch(x.device, L.dsmil_trunk32_conv_workspace_bytes(Cin, Cout, ks, stride, pad, B, H, W, p))
    y = torch.empty((B, max(Ho, 0), max(Wo, 0), Cout), dtype=torch.float32, device=x.device)
    mean = torch.empty((B, Cout), dtype=torch.float32, device=x.device)
    rstd = torch.empty_like(mean)
    with torch.cuda.device(x.device):
        rc = L.dsmil_trunk32_conv(_ptr(x), _ptr(w), _ptr(im), _ptr(ir), _ptr(bm), _ptr(br), _ptr(y), _ptr(mean), _ptr(rstd), B, H, W,
                                  Cin, Cout, ks, stride, pad, p, _ptr(ws), ws.numel(), _stream(x.device))
    _refused(rc, "dsmil_trunk32_conv")
    return y, mean, rstd


def trunk32_stem(x, conv1_w, frozen=None, precision="fp32"):
    """pack + stem + statistics + pool: x fp32 NCHW [B,3,H,W] or uint8 NHWC [B,H,W,3] -> (pooled fp32 NHWC [B,Hp,Wp,64],
    mean [B,64], rstd [B,64]).  ``frozen`` = (m, r) [64]: the frozen-statistics route (raw map + k_norm_relu_maxpool)."""
    if not x.is_cuda or not x.is_contiguous() or x.dtype not in (torch.float32, torch.uint8):
        raise RuntimeError("x must be a contiguous float32 NCHW or uint8 NHWC CUDA(HIP) tensor")
    u8 = x.dtype == torch.uint8
    B, H, W = (x.shape[0], x.shape[1], x.shape[2]) if u8 else (x.shape[0], x.shape[2], x.shape[3])
    if (x.shape[3] if u8 else x.shape[1]) != 3:
        raise ValueError("the stem takes three input channels")
    w = _f32c(conv1_w, "conv1_w")
    if tuple(w.shape) != (64, 3, 7, 7):
        raise ValueError("conv1_w must be [64,3,7,7]")
    bm, br = (_f32c(t, "frozen") for t in frozen) if frozen is not None else (None, None)
    Hp, Wp = _conv_out(*_conv_out(H, W, 7, 2, 3), 3, 2, 1)
    L = _native.lib()
    ws = _scratch(x.device, L.dsmil_trunk32_stem_workspace_bytes(B, H, W))
    pooled = torch.empty((B, Hp, Wp, 64), dtype=torch.float32, device=x.device)
    mean = torch.empty((B, 64), dtype=torch.float32, device=x.device)
    rstd = torch.empty_like(mean)
    with torch.cuda.device(x.device):
        rc = L.dsmil_trunk32_stem(_ptr(x), 1 if u8 else 0, _ptr(w), _ptr(bm), _ptr(br), _ptr(pooled), _ptr(mean), _ptr(rstd), B, H, W,
                                  TRUNK32_PRECISIONS[precision], _ptr(ws), ws.numel(), _stream(x.device))
    _refused(rc, "dsmil_trunk32_stem")
    return pooled, mean, rstd


def trunk32_tail(kind, y2, stats, idn, down_stats=None):
    """The pass that closes a block, y2 / idn fp32 [B,...,C], stats = (mean, rstd) [B,C]: "identity" relu(IN(y2) + idn),
    "down" relu(IN(y2) + IN(idn)) with ``down_stats`` of the raw downsample branch idn, "pool" the pixel mean of "identity"
    -> [B,C]."""
    y2, idn = _f32c(y2, "y2"), _f32c(idn, "idn")
    if idn.shape != y2.shape:
        raise ValueError("idn must have y2's shape")
    B, C = y2.shape[0], y2.shape[-1]
    HW = y2.numel() // (B * C)
    m2, r2 = (_f32c(t, "stats") for t in stats)
    md, rd = (_f32c(t, "down_stats") for t in down_stats) if down_stats is not None else (None, None)
    out = torch.empty((B, C) if kind == "pool" else y2.shape, dtype=torch.float32, device=y2.device)
    with torch.cuda.device(y2.device):
        rc = _native.lib().dsmil_trunk32_tail(TRUNK32_TAILS[kind], _ptr(y2), _ptr(m2), _ptr(r2), _ptr(idn), _ptr(md), _ptr(rd), _ptr(out),
                                              B, HW, C, 0, _stream(y2.device))
    _refused(rc, "dsmil_trunk32_tail")
    return out


# ---------------------------------------------------------------------------------------------
# conv backward for training the embedder (csrc/conv_bwd.hip behind dsmil_conv_bwd_*): the weight and the data gradient of one
# conv in the fp32-class trunk's layout and arithmetic (fp32 NHWC maps, fp32 OIHW weights, two fp16 planes, three products).
# A shape the kernels do not take raises NotImplementedError (DSMIL_E_UNSUPPORTED), every other refusal RuntimeError; nothing
# is launched in either case.
# ---------------------------------------------------------------------------------------------
CONV_BWD_WHICH = {"weight": 0, "data": 1}
_CONV_BWD_PLAN_FIELDS = ("which", "Ho", "Wo", "out_rows", "out_cols", "grid_x", "grid_y", "grid_z", "block", "chunk", "n_partials",
                         "run_len", "cols_pad")


def conv_backward_plan(Cin, Cout, ks, stride, pad, B, H, W, which="weight"):
    """What the host decides for this gradient (no device needed): a dict of ``Ho, Wo`` (the map of dy), ``out_rows, out_cols``
    (the output GEMM), ``grid_x, grid_y, grid_z, block``, and for the weight gradient ``chunk`` (positions per chunk),
    ``n_partials`` (partials a dw element is summed from), ``run_len`` (the longest run of positions one accumulator sums)
    and ``cols_pad``.  For the data gradient ``run_len`` = Cout ks^2 and ``n_partials`` = 1."""
    d = _plan("dsmil_conv_bwd_plan", _CONV_BWD_PLAN_FIELDS, Cin, Cout, ks, stride, pad, B, H, W, CONV_BWD_WHICH[which])
    d["which"] = which
    return d


def conv_backward_weight(x_nhwc, dy_nhwc, ks, stride, pad, in_stats=None, ws=None):
    """dsmil_conv_bwd_weight: x fp32 NHWC [B,H,W,Cin], dy fp32 NHWC [B,Ho,Wo,Cout] -> dw fp32 OIHW [Cout,Cin,ks,ks].
    ``in_stats`` = (mean, rstd) [B,Cin]: x is a raw conv output and the gradient is taken against relu((x - mean) rstd), the
    operand trunk32_conv stages.  ``ws``: a caller's workspace (uint8, any contents); default a fresh one.  No host sync."""
    x, dy = _f32c(x_nhwc, "x_nhwc"), _f32c(dy_nhwc, "dy_nhwc")
    B, H, W, Cin = x.shape
    Cout = dy.shape[3]
    Ho, Wo = _conv_out(H, W, ks, stride, pad)
    if tuple(dy.shape) != (B, Ho, Wo, Cout):
        raise ValueError(f"dy is {tuple(dy.shape)}, this conv of x gives {(B, Ho, Wo, 'Cout')}")
    im, ir = (_f32c(t, "in_stats") for t in in_stats) if in_stats is not None else (None, None)
    L = _native.lib()
    shape = (Cin, Cout, ks, stride, pad, B, H, W, 0)
    need = _size_or_reason(L.dsmil_conv_bwd_workspace_bytes(*shape), "dsmil_conv_bwd_plan", "dsmil_conv_bwd_weight", *shape)
    ws = _scratch(x.device, need, ws)
    dw = torch.empty((Cout, Cin, ks, ks), dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        rc = L.dsmil_conv_bwd_weight(_ptr(x), _ptr(im), _ptr(ir), _ptr(dy), _ptr(dw), B, H, W, Cin, Cout, ks, stride, pad, _ptr(ws),
                                     ws.numel(), _stream(x.device))
    _refused(rc, "dsmil_conv_bwd_weight")
    return dw


def conv_backward_data(dy_nhwc, w, H, W, stride, pad, ws=None):
    """dsmil_conv_bwd_data: dy fp32 NHWC [B,Ho,Wo,Cout], w fp32 OIHW [Cout,Cin,ks,ks] -> dx fp32 NHWC [B,H,W,Cin] for the H x W
    input the conv read.  An input pixel no output reads gets an exact 0.  No host sync."""
    dy, w = _f32c(dy_nhwc, "dy_nhwc"), _f32c(w, "w")
    B, Ho, Wo, Cout = dy.shape
    Cout_w, Cin, ks, _ = w.shape
    if Cout_w != Cout:
        raise ValueError(f"w gives {Cout_w} output channels, dy has {Cout}")
    if (Ho, Wo) != _conv_out(H, W, ks, stride, pad):
        raise ValueError(f"dy is {Ho} x {Wo}, this conv of a {H} x {W} input gives another map")
    L = _native.lib()
    shape = (Cin, Cout, ks, stride, pad, B, H, W, 1)
    need = _size_or_reason(L.dsmil_conv_bwd_workspace_bytes(*shape), "dsmil_conv_bwd_plan", "dsmil_conv_bwd_data", *shape)
    ws = _scratch(dy.device, need, ws)
    dx = torch.empty((B, H, W, Cin), dtype=torch.float32, device=dy.device)
    with torch.cuda.device(dy.device):
        rc = L.dsmil_conv_bwd_data(_ptr(dy), _ptr(w), _ptr(dx), B, H, W, Cin, Cout, ks, stride, pad, _ptr(ws), ws.numel(),
                                   _stream(dy.device))
    _refused(rc, "dsmil_conv_bwd_data")
    return dx


def conv_backward_supported(Cin, Cout, ks, stride, pad, B, H, W, which):
    """True where dsmil_conv_bwd_weight (``which`` = "weight") / dsmil_conv_bwd_data ("data") take the shape.  No device."""
    return _native.lib().dsmil_conv_bwd_workspace_bytes(Cin, Cout, ks, stride, pad, B, H, W, CONV_BWD_WHICH[which]) > 0


# ---------------------------------------------------------------------------------------------
# InstanceNorm / ReLU / residual-add backward for training the embedder (csrc/norm_bwd.hip behind dsmil_norm_bwd*): the gradient
# of a RAW conv output from the gradient of relu(IN(y)) or of a block's relu(IN(y) + identity | IN(yd)).  Refusals as for the
# conv backward: NotImplementedError for DSMIL_E_UNSUPPORTED, RuntimeError otherwise, nothing launched in either case.
# ---------------------------------------------------------------------------------------------
NORM_BWD_KINDS = {"relu": 0, "add": 1, "add_down": 2}
_NORM_BWD_PLAN_FIELDS = ("kind", "chunk", "n_partials", "run_len", "lanes", "n_sums", "grid_partial", "grid_finish", "grid_apply",
                         "block", "groups")


def norm_backward_plan(kind, B, HW, C):
    """What the host decides for this call (no device needed): a dict of ``chunk`` (pixels per chunk), ``n_partials`` (partials
    an (n, c) sum is added from, in chunk order), ``lanes`` (accumulators per channel and chunk, combined in a fixed tree),
    ``run_len`` (the longest serial run of terms one accumulator adds), ``n_sums`` (2; "add_down" 3), ``grid_partial,
    grid_finish, grid_apply, block`` and ``groups`` (4-channel groups per thread)."""
    d = _plan("dsmil_norm_bwd_plan", _NORM_BWD_PLAN_FIELDS, NORM_BWD_KINDS[kind], B, HW, C)
    d["kind"] = kind
    return d


def norm_backward_supported(kind, B, HW, C):
    """True where dsmil_norm_bwd takes the shape.  No device."""
    return _native.lib().dsmil_norm_bwd_workspace_bytes(NORM_BWD_KINDS[kind], B, HW, C) > 0


def norm_backward(kind, g, y, stats, out=None, down=None, ws=None):
    """dsmil_norm_bwd on fp32 maps [B,...,C] (NHWC) with ``stats`` = (mean, rstd) [B,C] of the raw conv output ``y``:
    "relu"      g = the gradient of relu(IN(y))                     -> gy
    "add"       g = the gradient of ``out`` = relu(IN(y) + idn)      -> (gy, gres), gres the gradient of idn
    "add_down"  g = the gradient of ``out`` = relu(IN(y) + IN(yd)), ``down`` = (yd, (md, rd))   -> (gy, gyd)
    ``ws``: a caller's workspace (uint8, any contents); default a fresh one.  No host sync."""
    k = NORM_BWD_KINDS[kind]
    g, y = _f32c(g, "g"), _f32c(y, "y")
    if g.shape != y.shape or y.dim() < 2:
        raise ValueError("g must have y's shape [B, ..., C]")
    B, C = y.shape[0], y.shape[-1]
    HW = y.numel() // max(B * C, 1)
    m, r = (_f32c(t, "stats") for t in stats)
    if (out is None) != (kind == "relu") or (down is None) != (kind != "add_down"):
        raise ValueError(f'kind "{kind}": out is given for "add" and "add_down" only, down for "add_down" only')
    o = yd = md = rd = gyd = gres = None
    if out is not None:
        o = _f32c(out, "out")
    if down is not None:
        yd = _f32c(down[0], "down")
        md, rd = (_f32c(t, "down stats") for t in down[1])
    for t, name in ((o, "out"), (yd, "down")):
        if t is not None and t.shape != y.shape:
            raise ValueError(f"{name} must have y's shape")
    for t in (m, r, md, rd):
        if t is not None and tuple(t.shape) != (B, C):
            raise ValueError("statistics must be [B, C]")
    L = _native.lib()
    need = _size_or_reason(L.dsmil_norm_bwd_workspace_bytes(k, B, HW, C), "dsmil_norm_bwd_plan", "dsmil_norm_bwd", k, B, HW, C)
    ws = _scratch(y.device, need, ws)
    gy = torch.empty_like(y)
    if kind == "add":
        gres = torch.empty_like(y)
    elif kind == "add_down":
        gyd = torch.empty_like(y)
    with torch.cuda.device(y.device):
        rc = L.dsmil_norm_bwd(k, _ptr(g), _ptr(o), _ptr(y), _ptr(m), _ptr(r), _ptr(yd), _ptr(md), _ptr(rd), _ptr(gy), _ptr(gyd),
                              _ptr(gres), B, HW, C, _ptr(ws), ws.numel(), _stream(y.device))
    _refused(rc, "dsmil_norm_bwd")
    return gy if kind == "relu" else (gy, gres) if kind == "add" else (gy, gyd)


# ---------------------------------------------------------------------------------------------
# the stem on the training path (dsmil_trunk32_stem_train in csrc/resnet_fwd.hip, dsmil_stem_pool_bwd* in csrc/stem_bwd.hip): a
# forward that keeps the raw map and the pool's winners, and the gradient of the raw map from the gradient of
# maxpool(relu(IN(y))).  Refusals as above: NotImplementedError for DSMIL_E_UNSUPPORTED, RuntimeError otherwise, nothing launched.
# ---------------------------------------------------------------------------------------------
_STEM_BWD_PLAN_FIELDS = ("Hp", "Wp", "chunk", "n_partials", "run_len", "lanes", "grid_partial", "grid_finish", "grid_apply", "block",
                         "groups")


def trunk32_stem_train_supported(B, H, W):
    """True where dsmil_trunk32_stem_train takes a [B,3,H,W] input.  No device."""
    return _native.lib().dsmil_trunk32_stem_train_workspace_bytes(B, H, W) > 0


def trunk32_stem_train(x, conv1_w, precision="fp32"):
    """The stem of a training forward: x fp32 NCHW [B,3,H,W] or uint8 NHWC [B,H,W,3] -> (pooled fp32 NHWC [B,Hp,Wp,64], the raw
    map y [B,H1,W1,64], (mean, rstd) [B,64], win uint8 [B,Hp,Wp,64]: each pool window's winner as dy * 3 + dx).  pooled, mean
    and rstd are bit-identical to trunk32_stem's."""
    if not x.is_cuda or not x.is_contiguous() or x.dtype not in (torch.float32, torch.uint8) or x.dim() != 4:
        raise RuntimeError("x must be a contiguous float32 NCHW or uint8 NHWC CUDA(HIP) tensor")
    u8 = x.dtype == torch.uint8
    B, H, W = (x.shape[0], x.shape[1], x.shape[2]) if u8 else (x.shape[0], x.shape[2], x.shape[3])
    if (x.shape[3] if u8 else x.shape[1]) != 3:
        raise ValueError("the stem takes three input channels")
    w = _f32c(conv1_w, "conv1_w")
    if tuple(w.shape) != (64, 3, 7, 7):
        raise ValueError("conv1_w must be [64,3,7,7]")
    H1, W1 = _conv_out(H, W, 7, 2, 3)
    Hp, Wp = _conv_out(H1, W1, 3, 2, 1)
    L = _native.lib()
    ws = _scratch(x.device, L.dsmil_trunk32_stem_train_workspace_bytes(B, H, W))
    new = lambda *shape, dtype=torch.float32: torch.empty(shape, dtype=dtype, device=x.device)
    y, pooled, win = new(B, H1, W1, 64), new(B, Hp, Wp, 64), new(B, Hp, Wp, 64, dtype=torch.uint8)
    mean, rstd = new(B, 64), new(B, 64)
    with torch.cuda.device(x.device):
        rc = L.dsmil_trunk32_stem_train(_ptr(x), 1 if u8 else 0, _ptr(w), _ptr(y), _ptr(mean), _ptr(rstd), _ptr(pooled), _ptr(win),
                                        B, H, W, TRUNK32_PRECISIONS[precision], _ptr(ws), ws.numel(), _stream(x.device))
    _refused(rc, "dsmil_trunk32_stem_train")
    return pooled, y, (mean, rstd), win


def stem_pool_backward_plan(B, H1, W1, C):
    """What the host decides for this call (no device needed): ``Hp, Wp`` (the pooled map), and norm_backward_plan's ``chunk,
    n_partials, run_len, lanes, grid_partial, grid_finish, grid_apply, block, groups`` over the H1 W1 pixels of the raw map."""
    return _plan("dsmil_stem_pool_bwd_plan", _STEM_BWD_PLAN_FIELDS, B, H1, W1, C)


def stem_pool_backward_supported(B, H1, W1, C):
    """True where dsmil_stem_pool_bwd takes the shape.  No device."""
    return _native.lib().dsmil_stem_pool_bwd_workspace_bytes(B, H1, W1, C) > 0


def stem_pool_backward(g, y, stats, win, ws=None):
    """dsmil_stem_pool_bwd: g fp32 NHWC [B,Hp,Wp,C] = the gradient of maxpool3x3/2/1(relu(IN(y))), y the raw map [B,H1,W1,C],
    ``stats`` = (mean, rstd) [B,C], ``win`` uint8 [B,Hp,Wp,C] as trunk32_stem_train returns it -> gy [B,H1,W1,C].
    ``ws``: a caller's workspace (uint8, any contents); default a fresh one.  No host sync."""
    g, y = _f32c(g, "g"), _f32c(y, "y")
    if y.dim() != 4 or g.dim() != 4:
        raise ValueError("g and y must be [B, H, W, C]")
    B, H1, W1, C = y.shape
    Hp, Wp = _conv_out(H1, W1, 3, 2, 1)
    if tuple(g.shape) != (B, Hp, Wp, C):
        raise ValueError(f"g is {tuple(g.shape)}, the pool of y gives {(B, Hp, Wp, C)}")
    if not win.is_cuda or win.dtype != torch.uint8 or not win.is_contiguous() or win.shape != g.shape:
        raise RuntimeError("win must be a contiguous uint8 CUDA(HIP) tensor of g's shape")
    m, r = (_f32c(t, "stats") for t in stats)
    if tuple(m.shape) != (B, C) or tuple(r.shape) != (B, C):
        raise ValueError("statistics must be [B, C]")
    L = _native.lib()
    shape = (B, H1, W1, C)
    need = _size_or_reason(L.dsmil_stem_pool_bwd_workspace_bytes(*shape), "dsmil_stem_pool_bwd_plan", "dsmil_stem_pool_bwd", *shape)
    ws = _scratch(y.device, need, ws)
    gy = torch.empty_like(y)
    with torch.cuda.device(y.device):
        rc = L.dsmil_stem_pool_bwd(_ptr(g), _ptr(y), _ptr(m), _ptr(r), _ptr(win), _ptr(gy), B, H1, W1, C, _ptr(ws), ws.numel(),
                                   _stream(y.device))
    _refused(rc, "dsmil_stem_pool_bwd")
    return gy


# ---------------------------------------------------------------------------------------------
# background filters of the tilers (deepzoom_tiler.py:56-61, test_crop_single.py:17-24)
# ---------------------------------------------------------------------------------------------
def tile_stats(tiles):
    """dsmil_tile_stats: uint8 NHWC tiles [B,H,W,3] on the device -> int64 [B,4] = per tile the three band sums of
    PIL's FIND_EDGES image and the sum of the ubyte HSV saturation (exact integers)."""
    if not tiles.is_cuda or tiles.dtype != torch.uint8 or tiles.dim() != 4 or tiles.shape[3] != 3:
        raise RuntimeError("tiles must be a CUDA(HIP) uint8 tensor [B,H,W,3]")
    tiles = tiles if tiles.is_contiguous() else tiles.contiguous()
    B, H, W, _ = tiles.shape
    out = torch.empty((B, 4), dtype=torch.int64, device=tiles.device)
    if B == 0:
        return out
    with torch.cuda.device(tiles.device):
        rc = _native.lib().dsmil_tile_stats(_ptr(tiles), B, H, W, _ptr(out), _stream(tiles.device))
    _native.check(rc, "dsmil_tile_stats")
    return out


# ---------------------------------------------------------------------------------------------
# batched baseline-JPEG decode on the device (compute_feats.py:28,107 `Image.open` in DataLoader workers)
# ---------------------------------------------------------------------------------------------
JPEG_REC = np.dtype([("ecs_begin", "<i8"), ("ecs_end", "<i8"), ("width", "<i4"), ("height", "<i4"), ("ncomp", "<i4"),
                     ("hsamp", "<i4"), ("vsamp", "<i4"), ("restart_interval", "<i4"), ("qt", "<i4", 3), ("dc", "<i4", 3),
                     ("ac", "<i4", 3), ("status", "<i4")])   # struct dsmil_jpeg_image


def jpeg_parse(blobs):
    """dsmil_jpeg_parse (HOST): the files of a batch (bytes-likes) -> (data uint8 [total] numpy, plan uint8 numpy, records =
    a structured view of the plan's per-image records: status 0 = decodable on the device, -2 = outside the decoder's scope,
    -1 = not a JPEG)."""
    n = len(blobs)
    if n == 0:
        raise ValueError("no files")
    sizes = np.fromiter((len(b) for b in blobs), dtype=np.int64, count=n)
    offsets = np.zeros(n + 1, np.int64)
    np.cumsum(sizes, out=offsets[1:])
    # (+32: the device reader prefetches 16 bytes past its position; an EOI behind the last file stops a truncated one)
    data = np.empty(int(offsets[-1]) + 32, np.uint8)
    data[int(offsets[-1]):] = 0
    data[int(offsets[-1])], data[int(offsets[-1]) + 1] = 0xFF, 0xD9
    mv = memoryview(data)
    for b, o, s in zip(blobs, offsets[:-1], sizes):
        mv[int(o):int(o + s)] = b
    L = _native.lib()
    plan = np.zeros(L.dsmil_jpeg_plan_bytes(n) + 16, np.uint8)
    a = (-plan.ctypes.data) % 16
    plan = plan[a:a + L.dsmil_jpeg_plan_bytes(n)]
    _native.check(L.dsmil_jpeg_parse(data.ctypes.data, offsets.ctypes.data, n, plan.ctypes.data), "dsmil_jpeg_parse")
    recs = plan[16:16 + JPEG_REC.itemsize * n].view(JPEG_REC)
    return data, plan, recs


def _pil_rgb(blob):
    import io
    from PIL import Image
    with Image.open(io.BytesIO(blob)) as im:
        return np.array(im.convert("RGB"), dtype=np.uint8, copy=True)


class _JpegPending:
    """A device decode in flight (jpeg_decode_begin): the launch is enqueued, its per-file status not yet read."""
    __slots__ = ("out", "blobs", "H", "W", "st_host", "st_np", "ev")


def jpeg_decode_begin(blobs, device, size=None, out=None, before_launch=None):
    """The first half of jpeg_decode: parse on the host, copy, ENQUEUE the device decode on the current stream and the copy of its
    per-file status into pinned memory — no host wait.  `.ev` (None when no file of the batch is decodable on the device) is
    recorded behind both; `.out` is the result tensor, complete once jpeg_decode_end has run.  A caller with several chunks keeps
    a decode or two in flight this way instead of waiting for every chunk's status before it enqueues anything else
    (pipeline._embed_jpeg_chunks).  `before_launch()` runs between the host-to-device copies of the files and the decode launch:
    the place for a stream wait on whoever still reads `out` — in front of the copies it would hold the HOST, the copy of a
    pageable buffer returns only when it has run."""
    dev = torch.device(device)
    if dev.type != "cuda":
        raise RuntimeError("jpeg_decode needs a CUDA(HIP) device")
    n = len(blobs)
    data, plan, recs = jpeg_parse(blobs)
    n_data = int(data.size) - 32        # (jpeg_parse pads the batch buffer)
    ok = recs["status"] == 0
    if size is None:
        if ok.any():
            j = int(np.argmax(ok))
            size = (int(recs["height"][j]), int(recs["width"][j]))
        else:
            size = _pil_rgb(blobs[0]).shape[:2]
    H, W = int(size[0]), int(size[1])
    on_dev = ok & (recs["height"] == H) & (recs["width"] == W)
    recs["status"][ok & ~on_dev] = -2          # another size: not this batch's launch (the Pillow path below checks the size)
    if out is not None and (not out.is_cuda or out.dtype != torch.uint8 or not out.is_contiguous() or out.numel() < n * H * W * 3):
        raise ValueError("out must be a contiguous uint8 device tensor of at least n * H * W * 3 elements")
    out = (torch.empty((n, H, W, 3), dtype=torch.uint8, device=dev) if out is None
           else out.view(-1)[:n * H * W * 3].view(n, H, W, 3))
    p = _JpegPending()
    p.out, p.blobs, p.H, p.W, p.st_host, p.st_np, p.ev = out, blobs, H, W, None, None, None
    if on_dev.any():
        L = _native.lib()
        status = torch.empty(n, dtype=torch.int32, device=dev)
        d_data = torch.from_numpy(data).to(dev, non_blocking=True)
        d_plan = torch.from_numpy(plan).to(dev, non_blocking=True)
        nbytes = L.dsmil_jpeg_workspace_bytes(n, H, W, n_data)
        ws = _workspace(dev, nbytes)
        if before_launch is not None:
            before_launch()
        with torch.cuda.device(dev):
            rc = L.dsmil_jpeg_decode(_ptr(d_data), n_data, _ptr(d_plan), n, H, W, _ptr(out), _ptr(status), _ptr(ws), ws.numel(), _stream(dev))
        _native.check(rc, "dsmil_jpeg_decode")
        p.st_host = torch.empty(n, dtype=torch.int32, pin_memory=True)
        p.st_host.copy_(status, non_blocking=True)
        p.ev = torch.cuda.Event()
        p.ev.record(torch.cuda.current_stream(dev))
    else:
        if before_launch is not None:
            before_launch()
        p.st_np = recs["status"].copy()
    return p


def jpeg_decode_end(p, stats=None):
    """The second half: wait for the status, decode what the device did not (other formats, other coding processes, streams it
    reports as corrupt) with Pillow and copy those files in on the CURRENT stream.  Returns (out, files redone)."""
    if p.ev is not None:
        p.ev.synchronize()
        st = p.st_host.numpy()
    else:
        st = p.st_np
    redo = np.nonzero(st != 0)[0]
    for i in redo:
        a = _pil_rgb(p.blobs[int(i)])
        if a.shape[:2] != (p.H, p.W):
            raise ValueError(f"file {int(i)} of the batch is {a.shape[1]}x{a.shape[0]}, the batch is {p.W}x{p.H}")
        p.out[int(i)].copy_(torch.from_numpy(a))
    if stats is not None:
        stats["device"] = stats.get("device", 0) + int(len(st) - len(redo))
        stats["pillow"] = stats.get("pillow", 0) + int(len(redo))
    p.blobs = None
    return p.out, int(len(redo))


def jpeg_decode(blobs, device, size=None, stats=None, out=None):
    """A batch of JPEG files (bytes-likes) -> uint8 [n, H, W, 3] on `device`, what
    `np.array(Image.open(f).convert("RGB"))` gives for every file (compute_feats.py:28 + the uint8 half of VF.to_tensor):
    baseline JPEGs are decoded on the device by dsmil_jpeg_decode (bit-identical to Pillow's defaults: islow IDCT, fancy
    upsampling), every other file (progressive, CMYK, a PNG ...) and every stream the device decoder reports as corrupt is
    decoded with Pillow on the host and copied in — the result never depends on which path a file took.
    ``size`` = (H, W) of the batch (default: the first decodable image's); all files must have it.
    ``stats`` (dict, optional) gets the counts {"device": .., "pillow": ..}.
    ``out``: a uint8 device tensor with room for [n, H, W, 3] (a caller's staging buffer); the result is a view of it.
    (= jpeg_decode_begin + jpeg_decode_end, the two halves a pipelining caller uses.)"""
    return jpeg_decode_end(jpeg_decode_begin(blobs, device, size=size, out=out), stats=stats)[0]


def _ntxent_operands(zis, zjs):
    zis = _f32c(zis, "zis"); zjs = _f32c(zjs, "zjs")
    if zis.dim() != 2 or zis.shape != zjs.shape or zis.device != zjs.device:
        raise RuntimeError(f"zis and zjs must be [n, d] tensors of one shape on one device (got {tuple(zis.shape)}, "
                           f"{tuple(zjs.shape)})")
    n, d = zis.shape
    nbytes = _native.lib().dsmil_ntxent_workspace_bytes(n, d)
    if nbytes == 0:
        raise RuntimeError(f"dsmil_ntxent: unsupported shape n = {n}, d = {d} (1 <= n <= 65536, 1 <= d <= 4096)")
    return zis, zjs, n, d, nbytes


def ntxent_forward(zis, zjs, temperature, cosine=True):
    """dsmil_ntxent_forward: the NT-Xent loss of SimCLR (simclr/loss/nt_xent.py:47-65) for the projections ``zis``, ``zjs``
    [n, d] fp32 of the two views.  Returns (loss [], lse [2n]); ``lse`` is what ntxent_backward reads.  No host sync."""
    zis, zjs, n, d, nbytes = _ntxent_operands(zis, zjs)
    dev = zis.device
    out = torch.empty((1 + 2 * n,), dtype=torch.float32, device=dev)
    loss, lse = out[0:1], out[1:]
    with torch.cuda.device(dev):
        ws = _workspace(dev, nbytes)
        rc = _native.lib().dsmil_ntxent_forward(_ptr(zis), _ptr(zjs), n, d, float(temperature), 1 if cosine else 0, _ptr(loss),
                                                _ptr(lse), _ptr(ws), ws.numel(), _stream(dev))
    _native.check(rc, "dsmil_ntxent_forward")
    return loss.reshape(()), lse


def ntxent_backward(zis, zjs, temperature, lse, g_loss, cosine=True):
    """dsmil_ntxent_backward: (g_zis, g_zjs) [n, d] for the upstream gradient ``g_loss`` (a device scalar, read on the
    device).  ``lse`` is ntxent_forward's; the workspace need not be the forward's."""
    zis, zjs, n, d, nbytes = _ntxent_operands(zis, zjs)
    dev = zis.device
    lse = _f32c(lse.reshape(-1), "lse")
    g_loss = _f32c(g_loss.reshape(-1), "g_loss")
    if lse.numel() != 2 * n or g_loss.numel() != 1:
        raise RuntimeError("lse must have 2n elements and g_loss one")
    g = torch.empty((2, n, d), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        ws = _workspace(dev, nbytes)
        rc = _native.lib().dsmil_ntxent_backward(_ptr(zis), _ptr(zjs), n, d, float(temperature), 1 if cosine else 0, _ptr(lse),
                                                 _ptr(g_loss), _ptr(g[0]), _ptr(g[1]), _ptr(ws), ws.numel(), _stream(dev))
    _native.check(rc, "dsmil_ntxent_backward")
    return g[0], g[1]


# ---------------------------------------------------------------------------------------------
# SimCLR's two-view augmentation on decoded tiles (simclr/data_aug/dataset_wrapper.py:48-58, csrc/simclr_aug.hip)
# ---------------------------------------------------------------------------------------------
SIMCLR_FLIP, SIMCLR_JITTER, SIMCLR_GREY, SIMCLR_BLUR = 1, 2, 4, 8      # include/dsmil_hip.h
# struct dsmil_simclr_view as columns of an int32 [n, 12] array; columns 8..11 hold fp32 bits
SIMCLR_COLS = ("tile", "i", "j", "h", "w", "flags", "order", "hue", "brightness", "contrast", "saturation", "sigma")


def _simclr_check_records(rec, n_tiles, H, W):
    """Host validation of the records (numpy int32 [n, 12]): the kernel trusts none of this, but answers a bad record with an
    all-zero view instead of an error."""
    if rec.ndim != 2 or rec.shape[1] != 12 or rec.dtype != np.int32:
        raise ValueError("view records must be int32 [n_views, 12] (struct dsmil_simclr_view)")
    tile, i, j, h, w, flags, order, hue = (rec[:, k].astype(np.int64) for k in range(8))
    fl = np.ascontiguousarray(rec[:, 8:12]).view(np.float32)
    if ((tile < 0) | (tile >= n_tiles)).any():
        raise ValueError(f"a view names a tile outside the batch of {n_tiles}")
    if ((h < 1) | (w < 1) | (i < 0) | (j < 0) | (i + h > H) | (j + w > W)).any():
        raise ValueError(f"a view's crop lies outside its {H} x {W} tile")
    if ((flags < 0) | (flags > 15)).any() or ((hue < 0) | (hue > 255)).any():
        raise ValueError("view flags must be a combination of SIMCLR_* and the hue byte within 0..255")
    jit = (flags & SIMCLR_JITTER) != 0
    ops4 = np.stack([(order >> (2 * k)) & 3 for k in range(4)], 1)
    if ((order < 0) | (order > 255)).any() or (np.sort(ops4[jit], 1) != np.arange(4)).any():
        raise ValueError("a jittered view's order must be a permutation of 0..3, two bits per position")
    if not (np.isfinite(fl[jit, :3]).all() and (fl[jit, :3] >= 0).all()):
        raise ValueError("jitter factors must be finite and non-negative")
    blur = (flags & SIMCLR_BLUR) != 0
    if not (np.isfinite(fl[blur, 3]).all() and (fl[blur, 3] > 0).all()):
        raise ValueError("a blurred view's sigma must be finite and positive")


def simclr_views(tiles_u8, params, size, out="float"):
    """dsmil_simclr_views: SimCLR's augmentation chain (crop + Pillow-bilinear resize, flip, colour jitter, greyscale, Gaussian
    blur) for one record per output view.  ``tiles_u8``: uint8 [n, H, W, 3] (what jpeg_decode returns); ``params``: a
    simclr.ViewParams (or anything with ``.records``, CPU int32 [n_views, 12]); ``size`` = S.  Returns fp32 [n_views, 3, S, S]
    (byte / 255, ``out="float"``) or the bytes as uint8 [n_views, S, S, 3] (``out="uint8"``).  Device tiles: one launch on the
    current stream, no host synchronisation (the records go up in one copy, asynchronous when they are pinned).  CPU tiles take
    dsmil_simclr_views_host, the same arithmetic compiled for the host."""
    if out not in ("float", "uint8"):
        raise ValueError('out must be "float" or "uint8"')
    if tiles_u8.dtype != torch.uint8 or tiles_u8.dim() != 4 or tiles_u8.shape[3] != 3:
        raise ValueError("tiles must be a uint8 tensor [n, H, W, 3]")
    n_tiles, H, W, _ = tiles_u8.shape
    S = int(size)
    rec = params.records
    if rec.is_cuda or rec.dtype != torch.int32 or not rec.is_contiguous():
        raise ValueError("params.records must be a contiguous CPU int32 tensor")
    n_views = rec.shape[0]
    L = _native.lib()
    if n_tiles < 1 or n_views < 1 or L.dsmil_simclr_views_workspace_bytes(n_views, H, W, S) == 0:
        raise ValueError(f"simclr_views: unsupported shape: {n_tiles} tiles of {H} x {W}, {n_views} views of {S} (8 <= H, W <= 256; "
                         f"17 <= S <= 256 with an odd blur kernel int(0.06 S), here {int(0.06 * S)})")
    _simclr_check_records(rec.numpy(), n_tiles, H, W)
    tiles = tiles_u8 if tiles_u8.is_contiguous() else tiles_u8.contiguous()
    dev = tiles.device
    shape, dtype = ((n_views, 3, S, S), torch.float32) if out == "float" else ((n_views, S, S, 3), torch.uint8)
    res = torch.empty(shape, dtype=dtype, device=dev)
    of, ou = (_ptr(res), _ptr(None)) if out == "float" else (_ptr(None), _ptr(res))
    if dev.type != "cuda":
        rc = L.dsmil_simclr_views_host(_ptr(tiles), n_tiles, H, W, _ptr(rec), n_views, S, of, ou, _ptr(None), 0)
        _native.check(rc, "dsmil_simclr_views_host")
        return res
    with torch.cuda.device(dev):
        d_rec = rec.to(dev, non_blocking=True)
        ws = _workspace(dev, L.dsmil_simclr_views_workspace_bytes(n_views, H, W, S))
        rc = L.dsmil_simclr_views(_ptr(tiles), n_tiles, H, W, _ptr(d_rec), n_views, S, of, ou, _ptr(ws), ws.numel(), _stream(dev))
    _native.check(rc, "dsmil_simclr_views")
    return res
