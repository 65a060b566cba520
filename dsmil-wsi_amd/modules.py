"""Drop-in mirror of the reference model API (dsmil.py:6-74): FCLayer, IClassifier, BClassifier,
MILNet — same constructor signatures, forward tuples, attribute names and state_dict keys.

Parameters live in ordinary nn.Linear / nn.Conv1d sub-modules so that ``.apply(init)``
(train_tcga.py:229-239), ``state_dict()/load_state_dict()`` (train_tcga.py:186, testing_c16.py:122),
``copy.deepcopy`` and ``.cuda()/.cpu()`` behave exactly as with the reference.  When the input
is a CUDA(HIP) tensor the forward runs in libdsmil_hip.so (hand-written gfx950 kernels); a CPU
tensor takes the plain torch-CPU route (BASELINE config 0: MUSK1 plumbing via train_mil.py).
There is no silent GPU fallback: a missing native library raises.
"""
import torch
import torch.nn as nn
import torch.nn.functional as F

from . import ops

Q_DIM = 128


def _wdict(fc_w, fc_b, q0_w, q0_b, q2_w, q2_b, fcc_w, fcc_b, detach=False):
    """The weight dict of ops.agg_forward / agg_backward, in ops.W_KEYS order (so ``*w.values()`` are the weight arguments
    of the autograd Functions below)."""
    ts = (fc_w, fc_b, q0_w, q0_b, q2_w, q2_b, fcc_w, fcc_b)
    if detach:
        ts = [None if t is None else t.detach() for t in ts]
    return dict(zip(ops.W_KEYS, ts))


def check_row_map(row_map, n_rows):
    """An out-of-range index of a row map would become an out-of-bounds device read in the native row loads: checked once
    per call on the device, surfaced with the step's only host sync (the loss .item() of train_tcga.py:74)."""
    if row_map is not None and row_map.numel():
        torch._assert_async((row_map.min() >= 0) & (row_map.max() < n_rows), "row_map index out of range")


class FCLayer(nn.Module):
    """dsmil.py:6-12."""

    def __init__(self, in_size, out_size=1):
        super().__init__()
        self.fc = nn.Sequential(nn.Linear(in_size, out_size))

    def forward(self, feats):
        lin = self.fc[0]
        if feats.is_cuda:
            x = _FCFunction.apply(feats, lin.weight, lin.bias)
        else:
            x = lin(feats)
        return feats, x


def resnet_convs_of(fe):
    """(convs, bn_norms) when ``fe`` is a ResNet-18 trunk with fc = Identity that the native embedder
    covers — InstanceNorm (bn_norms None) or eval-mode BatchNorm — else None."""
    from .resnet import resnet18_bn_parts, resnet18_in_convs
    if not isinstance(getattr(fe, "fc", None), nn.Identity):
        return None
    convs = resnet18_in_convs(fe)
    if convs is not None:
        return convs, None
    return resnet18_bn_parts(fe)


class IClassifier(nn.Module):
    """dsmil.py:14-25: (feats.view(B,-1), Linear(feats)) around an arbitrary feature extractor."""

    def __init__(self, feature_extractor, feature_size, output_class):
        super().__init__()
        self.feature_extractor = feature_extractor
        self.fc = nn.Linear(feature_size, output_class)
        # not part of the reference API: "fp32" (the parity path), "half" or "bf16" — OPT-IN reduced precisions of the native
        # trunk (fp16 activations behind the stem / one fp16 plane per conv operand: ~2.6e-3 feature error; bf16 activations:
        # ~2e-2 — ops.resnet18in_forward)
        self.embed_precision = "fp32"

    def forward(self, x):
        fe = self.feature_extractor
        if x.dtype == torch.uint8 and (x.dim() != 4 or x.shape[3] != 3):
            # decoded images, uint8 NHWC [B,H,W,3] (new ingest path)
            raise ValueError(f"uint8 patches must be NHWC [B,H,W,3], got {tuple(x.shape)}")
        grad_on = torch.is_grad_enabled()
        trunk = None
        if x.is_cuda and x.dtype in (torch.float32, torch.uint8) and x.dim() == 4 and not (
                grad_on and (x.requires_grad or any(p.requires_grad for p in fe.parameters()))):
            # ResNet-18/34 + InstanceNorm / frozen BatchNorm with fc = Identity (ours or torchvision's,
            # compute_feats.py:157,170): the trunk runs in one native launch sequence
            trunk = resnet_convs_of(fe)
        if trunk is not None:
            head_trains = grad_on and (self.fc.weight.requires_grad or self.fc.bias.requires_grad)
            if not head_trains:
                # features and instance logits from the same launch sequence (uint8: ToTensor fused in the stem)
                return ops.resnet18in_forward(x, trunk[0], self.fc.weight, self.fc.bias, bn_norms=trunk[1],
                                              precision=self.embed_precision)
            # frozen trunk + trainable linear head (what compute_feats.py:168-173 / attention_map.py set up):
            # the reference differentiates through self.fc (dsmil.py:24), so the head goes through autograd
            feats, _ = ops.resnet18in_forward(x, trunk[0], bn_norms=trunk[1], precision=self.embed_precision)
            return feats, _FCFunction.apply(feats, self.fc.weight, self.fc.bias)
        if x.dtype == torch.uint8:
            # no native stem will take the bytes: apply VF.to_tensor here (compute_feats.py:35-39)
            x = x.permute(0, 3, 1, 2).to(torch.float32).div(255)
        feats = fe(x)
        feats = feats.view(feats.shape[0], -1)
        if feats.is_cuda:
            c = _FCFunction.apply(feats, self.fc.weight, self.fc.bias)
        else:
            c = self.fc(feats)
        return feats, c


class BClassifier(nn.Module):
    """dsmil.py:27-62."""

    train_value_on_bf16 = False
    """Opt-in (set it on an instance): train the value layer of a ``passing_v`` model on bf16-stored rows.  The projection
    then runs INSIDE the aggregator's autograd Function (dsmil_value_forward_bf16 in its forward; in its backward the fp32
    g_vals of dsmil_agg_backward_bags_bf16 go unrounded to dsmil_value_backward_bf16), and v.1.weight / v.1.bias get their
    gradients in their own dtype.  Off, that combination raises NotImplementedError as it always has; the default flips in a
    follow-up that may touch the test pinning the refusal (tests/test_bwd_b16_gpu.py::test_refusals).  Rows that require a
    gradient are refused either way, an ACTIVE dropout keeps the torch route, a frozen value layer stays a constant."""

    def __init__(self, input_size, output_class, dropout_v=0.0, nonlinear=True, passing_v=False):
        super().__init__()
        if nonlinear:
            self.q = nn.Sequential(nn.Linear(input_size, Q_DIM), nn.ReLU(), nn.Linear(Q_DIM, Q_DIM), nn.Tanh())
        else:
            self.q = nn.Linear(input_size, Q_DIM)
        if passing_v:
            self.v = nn.Sequential(nn.Dropout(dropout_v), nn.Linear(input_size, input_size), nn.ReLU())
        else:
            self.v = nn.Identity()
        self.fcc = nn.Conv1d(output_class, output_class, kernel_size=input_size)

    # -- helpers --------------------------------------------------------------------------
    @property
    def nonlinear(self):
        return isinstance(self.q, nn.Sequential)

    @property
    def passing_v(self):
        return not isinstance(self.v, nn.Identity)

    def _weights(self):
        if self.nonlinear:
            q0, q2 = self.q[0], self.q[2]
            d = {"q0_w": q0.weight, "q0_b": q0.bias, "q2_w": q2.weight, "q2_b": q2.bias}
        else:
            d = {"q0_w": self.q.weight, "q0_b": self.q.bias, "q2_w": None, "q2_b": None}
        d["fcc_w"] = self.fcc.weight
        d["fcc_b"] = self.fcc.bias
        return d

    def _forward_cpu(self, feats, c):
        V = self.v(feats)
        Q = self.q(feats).view(feats.shape[0], -1)
        m_indices = torch.argmax(c, dim=0)  # lowest index on ties
        q_max = self.q(feats.index_select(0, m_indices))
        A = F.softmax(Q.mm(q_max.t()) / (Q.shape[1] ** 0.5), dim=0)
        B = A.t().mm(V).unsqueeze(0)
        C = self.fcc(B).view(1, -1)
        return C, A, B

    def _values(self, feats):
        """V = self.v(feats) (dsmil.py:48) for CUDA rows, None for v = Identity.  CUDA fp32 rows take the native projection
        whether or not they require a gradient (ops.value_proj: Linear + ReLU in one HIP launch; its parameter gradients in
        ops.value_proj_backward, the gradient of the rows in ops.value_proj_backward_rows).  An ACTIVE dropout (training
        mode, p > 0) is torch's own, applied to the rows first — the native projection then runs on the dropped rows; torch's
        random stream is not reproduced inside a kernel.  bf16-stored rows take the native projection of the bf16 path
        (dsmil_value_forward_bf16: fp32 master weights are rounded inside, as ops.agg_forward does with the aggregator's),
        as a constant: under autograd a TRAINABLE value layer on bf16 rows is projected inside _AggFunction instead
        (_value_args, with ``train_value_on_bf16``) and raises here (detaching it would train without it and say nothing);
        a frozen one is a constant.  With an ACTIVE dropout they keep the torch route (nn.Linear + ReLU)."""
        if not self.passing_v:
            return None
        drop, lin = self.v[0], self.v[1]
        active = drop.training and drop.p > 0
        if feats.dtype == torch.bfloat16 and not active:
            if torch.is_grad_enabled() and (lin.weight.requires_grad or lin.bias.requires_grad):
                raise NotImplementedError("passing_v with a trainable value layer on bf16-stored rows is opt-in: set "
                                          "b_classifier.train_value_on_bf16 = True (or freeze b_classifier.v, or store "
                                          "the rows in fp32)")
            return ops.value_proj(feats.detach(), lin.weight.detach(), lin.bias.detach())
        if feats.dtype != torch.float32:
            return self.v(feats)
        x = drop(feats) if active else feats
        return _ValueProjFunction.apply(x, lin.weight, lin.bias)

    def _value_args(self, feats):
        """(vals, v_w, v_b) for _AggFunction: ``vals`` = _values(feats) and no layer — except for bf16-stored rows with a
        TRAINABLE value layer under autograd on an instance that set ``train_value_on_bf16`` (no active dropout): then no
        ``vals`` and the layer's two parameters, and the Function projects the rows itself (a bf16 V tensor in the graph
        between two Functions would have the engine round g_vals to bf16 on its way to the value layer)."""
        if self.passing_v and self.train_value_on_bf16 and feats.dtype == torch.bfloat16 and torch.is_grad_enabled():
            drop, lin = self.v[0], self.v[1]
            if not (drop.training and drop.p > 0) and (lin.weight.requires_grad or lin.bias.requires_grad):
                return None, lin.weight, lin.bias
        return self._values(feats), None, None

    def forward(self, feats, c):
        if not feats.is_cuda:
            return self._forward_cpu(feats, c)
        MILNet._loss_dtype(feats)   # (bf16 rows that require a gradient are refused here, under grad mode)
        w = _wdict(None, None, **self._weights())
        vals, v_w, v_b = self._value_args(feats)
        pred, A, B = _AggFunction.apply(feats, c, vals, None, *w.values(), self.nonlinear, False, v_w, v_b)[1:4]
        return pred, A, B


class MILNet(nn.Module):
    """dsmil.py:64-74."""

    def __init__(self, i_classifier, b_classifier):
        super().__init__()
        self.i_classifier = i_classifier
        self.b_classifier = b_classifier

    def _fused(self, x=None):
        """Whether the fused native calls (FCLayer's logits + the aggregator in one call sequence) apply: the two modules
        are FCLayer + BClassifier and — given rows — ``x`` is a 2-D CUDA tensor whose dtype the value stream takes natively
        (with passing_v: fp32 or bf16).  Every caller adds its own further conditions."""
        ic, bc = self.i_classifier, self.b_classifier
        if not (isinstance(ic, FCLayer) and isinstance(bc, BClassifier)):
            return False
        return x is None or (x.is_cuda and x.dim() == 2 and (x.dtype in (torch.float32, torch.bfloat16) or not bc.passing_v))

    def _lin_weights(self, detach=False):
        """(FCLayer's nn.Linear, the eight-key weight dict of the fused native calls)."""
        lin = self.i_classifier.fc[0]
        return lin, _wdict(lin.weight, lin.bias, **self.b_classifier._weights(), detach=detach)

    def forward(self, x):
        return self._forward(x)

    def _forward(self, x, _f32_out=False):
        ic, bc = self.i_classifier, self.b_classifier
        if self._fused(x):
            self._loss_dtype(x)   # (bf16 rows that require a gradient are refused here, under grad mode)
            # one fused native call: instance logits + aggregator (dsmil.py:70-74); with passing_v the native value
            # projection runs in front of it and its result goes in as `vals` (bf16 rows: the bf16 forms of both calls);
            # rows that require a gradient get it from the native backward (k_bwd_gx, k_value_gx).
            # _f32_out (bag_loss / batch_loss): on bf16 rows keep the call's fp32 outputs — the loss is formed from those
            _, w = self._lin_weights()
            vals, v_w, v_b = bc._value_args(x)
            return _AggFunction.apply(x, None, vals, None, *w.values(), bc.nonlinear, _f32_out, v_w, v_b)[0:4]
        feats, classes = ic(x)
        prediction_bag, A, B = bc(feats, classes)
        return classes, prediction_bag, A, B

    def graphed(self, n_rows, dtype=None):
        """A hipGraph-replayed forward for bags of exactly ``n_rows`` rows (inference; weights frozen): returns a
        callable feats -> (classes, pred [1,C], A, B [1,C,K]).  Single-bag latency is launch-bound otherwise.
        ``dtype``: the bags' storage type, torch.float32 or torch.bfloat16 (the bf16-storage path, fp32 outputs); None = the
        parameters' own (bf16 after ``.bfloat16()``, else fp32)."""
        if not self._fused():
            raise NotImplementedError("graphed forward: FCLayer + BClassifier")
        bc = self.b_classifier
        lin, w = self._lin_weights(detach=True)
        # passing_v: the value projection is captured with the rest (inference: the dropout of bc.v is the identity)
        v_w, v_b = (bc.v[1].weight.detach(), bc.v[1].bias.detach()) if bc.passing_v else (None, None)
        if dtype is None:
            dtype = torch.bfloat16 if lin.weight.dtype == torch.bfloat16 else torch.float32
        g = ops.GraphedAggForward(w, n_rows, lin.in_features, nonlinear=bc.nonlinear, device=lin.weight.device, dtype=dtype,
                                  v_w=v_w, v_b=v_b)

        def run(feats):
            classes, pred, A, B, _ = g(feats)
            return classes, pred, A, B
        run.graph = g
        return run

    def bag_loss(self, feats, label, row_map=None, pos_weight=None, weight=None):
        """The training objective of one bag, train_tcga.py:64-71 / train_mil.py, as ONE native forward + loss head
        (and one native backward under autograd):
            bag_feats = feats[row_map]                      (dropout_patches :78-83, folded into the row loads)
            ins, bag, _, _ = milnet(bag_feats);  mx = max(ins, 0)
            loss = 0.5 BCEWithLogitsLoss(bag, y) + 0.5 BCEWithLogitsLoss(mx, y)
        Returns (loss [], bag_prediction [1,C], max_prediction [C]).  CUDA fp32 bags with FCLayer + BClassifier
        (v = Identity) whose rows need no gradient take the fused path (the fused loss call has no row-gradient output); so do
        bf16-stored bags with K % 8 == 0 (the bf16 forward and dsmil_agg_backward_bags_bf16; a row map is ONE index_select
        of the bf16 rows in front of the call; loss and predictions are the fp32 ones of the forward's fp32 logits);
        everything else — a passing_v model and rows that require a gradient included, whose forward and backward are
        native all the same (value projection + aggregator + the row-gradient kernels) — composes the same objective
        around ``self(x)``.  ``pos_weight`` / ``weight``: the class weights of BCEWithLogitsLoss(weight, pos_weight)
        (train_mil.py:172-173), each None or a tensor of 1 or C elements; the fused path hands them to the weighted loss head
        (dsmil_agg_loss_head_w / _bags_w) as fp32 [C] device vectors (ops.bce_class_weights)."""
        out = self._native_loss(feats, label, row_map, None, pos_weight, weight)
        if out is not None:
            return out
        x = feats if row_map is None else feats.index_select(0, row_map)
        ins, bag, _, _ = self._forward(x, _f32_out=True)
        mx, _ = torch.max(ins, 0)
        y = label.view(1, -1).to(bag.dtype)
        loss = 0.5 * F.binary_cross_entropy_with_logits(bag.view(1, -1), y, weight, pos_weight=pos_weight) + \
            0.5 * F.binary_cross_entropy_with_logits(mx.view(1, -1), y, weight, pos_weight=pos_weight)
        return loss, bag, mx

    def _native_loss(self, feats, labels, row_map, lengths, pos_weight, weight):
        """The native objective of ``bag_loss`` (``lengths`` None) / ``batch_loss`` (a tuple): _BagLossFunction's result, or None
        where the rows, the model or the class count are not the native loss call's."""
        # (a batch alone also needs what dsmil_agg_backward_bags asks of the query biases: _batch_native)
        if not (self._batch_native(feats) if lengths is not None else self._fused(feats) and self._loss_dtype(feats)):
            return None
        bc, C = self.b_classifier, self.i_classifier.fc[0].out_features
        if bc.passing_v or feats.requires_grad or C > 64:   # (dsmil_agg_loss_head: one wave of classes; more take the torch expression)
            return None
        if feats.dtype == torch.bfloat16 and row_map is not None:
            feats, row_map = feats.index_select(0, row_map), None
        check_row_map(row_map, feats.shape[0])
        _, w = self._lin_weights()
        cw = ops.bce_class_weights(pos_weight, weight, C, feats.device)
        return _BagLossFunction.apply(feats, labels, row_map, lengths, *w.values(), bc.nonlinear, *cw)

    @torch.no_grad()
    def forward_bags(self, bags):
        """Batched inference over many independent bags in ONE native call sequence ("varlen").

        ``bags`` is a list of [N_i, K] CUDA tensors, or a tuple (feats [sum N_i, K], lengths).
        Returns a list of (classes, pred, A, B) tuples shaped like ``forward``'s.  New capability
        (the reference loops one bag per iteration, train_tcga.py:92-99)."""
        bc = self.b_classifier
        if not self._fused():
            return [self.forward(b) for b in bags]
        if isinstance(bags, tuple):
            feats, lengths = bags
        else:
            lengths = [int(b.shape[0]) for b in bags]
            feats = torch.cat(list(bags), dim=0)
        # passing_v: ONE projection over the concatenated rows, then one aggregator call over the batch (fp32 and bf16 rows)
        vals = bc._values(feats)
        classes, pred, A, B, _ = ops.agg_forward(feats, lengths, self._lin_weights(detach=True)[1], vals=vals,
                                                 nonlinear=bc.nonlinear)
        out, o = [], 0
        for i, n in enumerate(lengths):
            out.append((classes[o:o + n], pred[i:i + 1], A[o:o + n], B[i:i + 1]))
            o += n
        return out

    @staticmethod
    def _loss_dtype(feats):
        """Row storage the native training calls take: fp32, or bf16 with K % 8 == 0 (the bf16 forward's condition)."""
        if feats.dtype == torch.bfloat16:
            if torch.is_grad_enabled() and feats.requires_grad:
                raise NotImplementedError("bf16-stored rows have no row gradient (store the rows in fp32 to differentiate them)")
            return feats.shape[1] % 8 == 0
        return feats.dtype == torch.float32

    # -- minibatches: several bags per call, differentiable ----------------------------------------
    def _batch_native(self, feats):
        """Whether a batch of these rows takes the native batched forward + backward (_AggFunction with lengths): fp32 rows
        (or bf16 rows with K % 8 == 0) under the conditions of ``forward``'s fused call, minus what dsmil_agg_backward_bags
        would reject (query biases off 16-byte alignment)."""
        if not (self._fused(feats) and self._loss_dtype(feats)):
            return False
        w = self.b_classifier._weights()
        return all(t is None or t.data_ptr() % 16 == 0 for t in (w["q0_b"], w["q2_b"]))

    def forward_batch(self, feats, lengths):
        """``forward`` over a batch of bags stored back to back — differentiable, unlike ``forward_bags``.

        feats [sum(lengths), K]; bag b owns rows sum(lengths[:b]) .. + lengths[b].  Returns
        (classes [T,C], pred [n,C], A [T,C], B [n,C,Kv]): per bag what ``forward`` returns, laid end to end.  CUDA fp32 rows
        (bf16-stored rows with K % 8 == 0 likewise: dsmil_agg_backward_bags_bf16, no row gradient, outputs in bf16)
        of MILNet(FCLayer, BClassifier): ONE native batched forward and, under autograd, ONE native batched backward
        (dsmil_agg_backward_bags) whose parameter gradients are summed over the bags; rows that require a gradient get it
        from the same call; with passing_v the value projection and its backward run once over the concatenated rows.
        Everything else (CPU tensors, other modules) runs the same mathematics bag by bag through ``forward``."""
        return self._forward_batch(feats, lengths)

    def _forward_batch(self, feats, lengths, _f32_out=False):
        lengths = [int(n) for n in lengths]
        if sum(lengths) != feats.shape[0] or any(n <= 0 for n in lengths):
            raise ValueError(f"bag lengths must be positive and sum to {feats.shape[0]} rows")
        if self._batch_native(feats):
            bc = self.b_classifier
            _, w = self._lin_weights()
            vals, v_w, v_b = bc._value_args(feats)
            return _AggFunction.apply(feats, None, vals, tuple(lengths), *w.values(), bc.nonlinear, _f32_out, v_w, v_b)[0:4]
        outs, o = [], 0
        for n in lengths:
            classes, pred, A, B = self._forward(feats[o:o + n], _f32_out)
            outs.append((classes, pred.view(1, -1), A, B.view(1, B.shape[-2], B.shape[-1])))
            o += n
        return tuple(torch.cat([t[i] for t in outs], dim=0) for i in range(4))

    def batch_loss(self, feats, lengths, labels, row_map=None, per_bag=False, pos_weight=None, weight=None):
        """The training objective of a BATCH of bags: loss = mean_b loss_b with loss_b the objective of ``bag_loss``
        (train_tcga.py:64-71) for bag b — one optimiser step per batch is this project's addition, the reference steps once
        per bag.  ``lengths`` count LOGICAL rows; ``row_map`` (int64 [sum(lengths)]) maps a logical row to a row of feats
        (every bag's dropout_patches index list with the bag's offset added, concatenated).  labels [n,C].
        Returns (loss [], pred [n,C], max_pred [n,C]) and, with per_bag, each bag's own loss [n] (detached) as a fourth value.
        CUDA fp32 rows that need no gradient, v = Identity, C <= 64: one native batched forward + batched loss head, and one
        native batched backward with the sparse max-stream gradient.  bf16-stored rows (K % 8 == 0) likewise, through the
        bf16 forward and dsmil_agg_backward_bags_bf16; a row map is one index_select of the bf16 rows in front of the call.  Otherwise the same objective from torch ops around
        ``forward_batch``.  ``pos_weight`` / ``weight`` as in ``bag_loss``."""
        lengths = [int(n) for n in lengths]
        n = len(lengths)
        labels = labels.reshape(n, -1)
        out = self._native_loss(feats, labels, row_map, tuple(lengths), pos_weight, weight)
        if out is not None:
            return out if per_bag else out[:3]
        x = feats if row_map is None else feats.index_select(0, row_map)
        ins, pred, _, _ = self._forward_batch(x, lengths, _f32_out=True)
        mx = torch.stack([t.max(0)[0] for t in torch.split(ins, lengths, dim=0)])
        y = labels.to(pred.dtype)
        each = 0.5 * F.binary_cross_entropy_with_logits(pred, y, weight, pos_weight=pos_weight, reduction="none").mean(1) + \
            0.5 * F.binary_cross_entropy_with_logits(mx, y, weight, pos_weight=pos_weight, reduction="none").mean(1)
        loss = each.mean()
        return (loss, pred, mx, each.detach()) if per_bag else (loss, pred, mx)


# ---------------------------------------------------------------------------------------------
# autograd glue
# ---------------------------------------------------------------------------------------------
class _FCFunction(torch.autograd.Function):
    """c = x W^T + b in the native library; backward is three small dense products (torch: the stand-alone FCLayer /
    IClassifier head.  Inside MILNet(FCLayer, BClassifier) the layer is fused into _AggFunction, whose backward — the
    instance stream's share of the row gradient included — is native)."""

    @staticmethod
    def forward(ctx, x, w, b):
        ctx.save_for_backward(x, w)
        if x.dtype != torch.float32:  # non-fp32 rows (bf16 storage): f32 accumulate, result in x.dtype
            return ops.fc_forward(x.detach().float(), w.detach().float(), b.detach().float()).to(x.dtype)
        return ops.fc_forward(x.detach(), w.detach(), b.detach())

    @staticmethod
    def backward(ctx, g):
        x, w = ctx.saved_tensors
        g32, x32 = g.float(), x.float()   # bf16-storage rows: gradients accumulate in f32 like the forward
        gx = g32.mm(w.float()).to(x.dtype) if ctx.needs_input_grad[0] else None
        gw = g32.t().mm(x32).to(w.dtype) if ctx.needs_input_grad[1] else None
        gb = g32.sum(0).to(w.dtype) if ctx.needs_input_grad[2] else None
        return gx, gw, gb


class _ValueProjFunction(torch.autograd.Function):
    """V = ReLU(x Wv^T + bv) in the native library (dsmil_value_forward); backward = dsmil_value_backward for the two
    parameter gradients and dsmil_value_backward_rows for the gradient of the INPUT rows, g_x = (g * (V > 0)) Wv (mask and
    all three contractions in HIP, deterministic)."""

    @staticmethod
    def forward(ctx, x, w, b):
        V = ops.value_proj(x.detach(), w.detach(), b.detach())
        ctx.save_for_backward(x, w, V)
        return V

    @staticmethod
    def backward(ctx, g):
        x, w, V = ctx.saved_tensors
        gw = gb = gx = None
        if ctx.needs_input_grad[1] or ctx.needs_input_grad[2]:
            gw, gb = ops.value_proj_backward(x, V, g)
        if ctx.needs_input_grad[0]:
            gx = ops.value_proj_backward_rows(V, g, w.detach())
        return gx, gw, gb


def _param_grads(g, w):
    """The eight parameter gradients of ops.agg_backward's dict in ops.W_KEYS order (None where the call made none), each in
    its parameter's dtype: fp32 for fp32 masters, bf16 for a module after ``.bfloat16()``."""
    return tuple(None if g.get(k) is None else g[k].to(w[k].dtype) for k in ops.W_KEYS)


class _BagLossFunction(torch.autograd.Function):
    """Forward = dsmil_agg_forward_ex (row map) + dsmil_agg_loss_head; backward = dsmil_agg_backward_ex with the sparse
    max-stream gradient.  Replaces, per training step, the row gather, torch.max, two BCEWithLogitsLoss graphs and the
    dense [N,C] instance-logit gradient of train_tcga.py:64-72.  With ``lengths`` (a tuple) the same over a batch of bags
    stored back to back: the batched forward + dsmil_agg_loss_head_bags, loss = the mean of the bags' losses (each bag's own
    loss is a fourth output), backward = dsmil_agg_backward_bags.  bf16-stored rows (no row map): the bf16 forward, the same
    loss head on its fp32 logits, backward = dsmil_agg_backward_bags_bf16; gradients in the parameters' dtype.
    ``pos_weight`` / ``weight`` (fp32 [C] device vectors or None): the loss head is its class-weighted form
    (dsmil_agg_loss_head_w / dsmil_agg_loss_head_bags_w); the backward is fed its g_pred / g_max as before."""

    @staticmethod
    def forward(ctx, feats, label, row_map, lengths, fc_w, fc_b, q0_w, q0_b, q2_w, q2_b, fcc_w, fcc_b, nonlinear,
                pos_weight=None, weight=None):
        w = _wdict(fc_w, fc_b, q0_w, q0_b, q2_w, q2_b, fcc_w, fcc_b, detach=True)
        if lengths is None:
            N = int(row_map.numel()) if row_map is not None else feats.shape[0]
            classes, pred, A, B, idx = ops.agg_forward(feats.detach(), [N], w, nonlinear=nonlinear, row_map=row_map)
            loss, max_pred, g_pred, g_max = ops.agg_loss_head(classes, pred, idx, label.detach(), pos_weight, weight)
            out = (loss, pred, max_pred)
        else:
            classes, pred, A, B, idx = ops.agg_forward(feats.detach(), lengths, w, nonlinear=nonlinear, row_map=row_map)
            each, max_pred, g_pred, g_max = ops.agg_loss_head_bags(classes, lengths, pred, idx, label.detach(),
                                                                   pos_weight=pos_weight, weight=weight)
            out = (each.mean(), pred, max_pred, each)
        ctx.nonlinear, ctx.lengths = nonlinear, lengths
        ctx.save_for_backward(feats, row_map, fc_w, q0_w, q0_b, q2_w, q2_b, fcc_w, A, B, idx, g_pred, g_max, fc_b, fcc_b)
        ctx.mark_non_differentiable(*out[1:])
        return out

    @staticmethod
    def backward(ctx, g_loss, *_):
        feats, row_map, fc_w, q0_w, q0_b, q2_w, q2_b, fcc_w, A, B, idx, g_pred, g_max, fc_b, fcc_b = ctx.saved_tensors
        # (the biases are not read by the backward; with them the dict is the forward's: the same cached bf16 weight set)
        w = _wdict(fc_w, fc_b, q0_w, q0_b, q2_w, q2_b, fcc_w, fcc_b, detach=True)
        g_loss = g_loss.float()
        # every parameter gradient is linear in (g_pred, g_max): the upstream scalar scales those two vectors (a batch: the
        # mean over the bags is a factor 1 / n on each bag's own)
        if ctx.lengths is None:
            g = ops.agg_backward(feats, w, A, B, idx, g_pred * g_loss, g_max=g_max * g_loss, row_map=row_map,
                                 nonlinear=ctx.nonlinear)
        else:
            scale = g_loss / len(ctx.lengths)
            g = ops.agg_backward_bags(feats, ctx.lengths, w, A, B, idx, g_pred * scale, g_max=g_max * scale, row_map=row_map,
                                      nonlinear=ctx.nonlinear)
        return (None, None, None, None, *_param_grads(g, w), None, None, None)


class _AggFunction(torch.autograd.Function):
    """Forward = dsmil_agg_forward (HIP).  Backward = analytic gradient of dsmil.py:46-62 (the
    arg-max indices are constants, as in the reference's autograd graph); it re-derives Q from
    the saved inputs (dsmil_agg_backward, csrc/agg_bwd.hip — SURVEY.md §8(f) row N1).  The gradient of the input rows,
    when asked for, comes from the same native call (dsmil_agg_backward_rows, k_bwd_gx).
    ``lengths`` None: ONE bag.  A tuple of lengths: a batch of bags stored back to back (fp32 rows, no ``c_in``) — the batched
    forward and, for the backward, dsmil_agg_backward_bags: every parameter gradient summed over the bags in one native call,
    g_vals for a trainable v and the gradient of the input rows from the same call.
    bf16-stored rows: the bf16 forward, outputs cast to the rows' dtype (``f32_out``: left fp32, for the loss); the backward widens the incoming gradients to fp32
    and is dsmil_agg_backward_bags_bf16 — the gradient of the reference function at the bf16 rows and the bf16-rounded
    parameters with the forward's A, B, idx, straight-through for the roundings; fp32 masters get fp32 gradients, a module
    after ``.bfloat16()`` gets them in bf16.  The rows themselves and caller-supplied ``vals`` get no gradient there.
    ``v_w``, ``v_b`` (bf16 rows, no ``vals``): the trainable value layer of a passing_v model.  The forward projects the rows
    itself (ops.value_proj, bf16 V, saved); the backward asks the bf16 aggregator backward for g_vals and hands them — fp32,
    as that call wrote them — with the stored bf16 rows and V to ops.value_proj_backward (dsmil_value_backward_bf16: one
    call over all rows of a batch), whose results come back in those two slots in the parameters' dtype."""

    @staticmethod
    def forward(ctx, feats, c_in, vals, lengths, fc_w, fc_b, q0_w, q0_b, q2_w, q2_b, fcc_w, fcc_b, nonlinear, f32_out=False,
                v_w=None, v_b=None):
        det = lambda t: t.detach() if t is not None else None
        w = _wdict(fc_w, fc_b, q0_w, q0_b, q2_w, q2_b, fcc_w, fcc_b, detach=True)
        ctx.proj = v_w is not None
        if ctx.proj:
            if feats.dtype != torch.bfloat16 or vals is not None or v_b is None:
                raise ValueError("v_w / v_b: the value layer of bf16-stored rows (no vals); fp32 rows take _ValueProjFunction")
            ctx.v_dtype = v_w.dtype
            vals = ops.value_proj(feats.detach(), v_w.detach(), v_b.detach())
        classes, pred, A, B, idx = ops.agg_forward(feats.detach(), [feats.shape[0]] if lengths is None else lengths, w,
                                                   classes_in=det(c_in), vals=det(vals), nonlinear=nonlinear)
        ctx.bf16 = feats.dtype == torch.bfloat16
        ctx.nonlinear, ctx.lengths = nonlinear, lengths
        ctx.has_cin = c_in is not None
        ctx.has_vals = vals is not None
        ctx.save_for_backward(feats, vals, fc_w, q0_w, q0_b, q2_w, q2_b, fcc_w, A, B, idx, fc_b, fcc_b)
        ctx.mark_non_differentiable(idx)
        if ctx.bf16 and not f32_out:   # bf16-storage path (BASELINE config 2): results keep the input dtype
            classes, pred, A, B = (t.to(torch.bfloat16) for t in (classes, pred, A, B))
        return classes, pred, A, B, idx

    @staticmethod
    def backward(ctx, g_cls, g_pred, g_A, g_B, _g_idx):
        if ctx.bf16 and (ctx.needs_input_grad[0] or (ctx.has_vals and ctx.needs_input_grad[2])):
            # (MILNet / BClassifier refuse these at the forward, under grad mode; a direct caller of the Function gets here)
            raise NotImplementedError("bf16-stored rows: the parameters (with v_w / v_b the value layer's too) have a native "
                                      "backward, the rows and caller-supplied vals do not")
        if ctx.bf16 or ctx.lengths is not None or not ctx.needs_input_grad[0] or _AggFunction._native_accepts(ctx):
            return _AggFunction._backward_native(ctx, g_cls, g_pred, g_A, g_B)
        return _AggFunction._backward_dense(ctx, g_cls, g_pred, g_A, g_B)

    @staticmethod
    def _native_accepts(ctx):
        """What dsmil_agg_backward_rows rejects (DSMIL_E_ALIGN): query biases that are not 16-byte aligned, e.g. views into
        a flat parameter buffer.  Every nn.Module parameter allocated by torch passes."""
        q0_b, q2_b = ctx.saved_tensors[4], ctx.saved_tensors[6]
        return all(t is None or t.data_ptr() % 16 == 0 for t in (q0_b, q2_b))

    @staticmethod
    def _backward_native(ctx, g_cls, g_pred, g_A, g_B):
        """dsmil_agg_backward (HIP): every parameter gradient, g_vals for a trainable v, and — when the input rows require
        one — their gradient (v = Identity: A gB included; caller's vals: the value function adds its own share)."""
        feats, vals, fc_w, q0_w, q0_b, q2_w, q2_b, fcc_w, A, B, idx, fc_b, fcc_b = ctx.saved_tensors
        C = fcc_w.shape[0]
        if g_pred is None:
            g_pred = torch.zeros((1 if ctx.lengths is None else len(ctx.lengths), C), device=feats.device)
        if ctx.bf16:   # the saved A, B are the forward's fp32 ones; the incoming gradients arrive in the outputs' dtype
            g_cls, g_pred, g_A, g_B = (None if t is None else t.float() for t in (g_cls, g_pred, g_A, g_B))
        # (the biases are not read by the backward; with them the dict is the forward's: the same cached bf16 weight set)
        w = _wdict(fc_w, fc_b, q0_w, q0_b, q2_w, q2_b, fcc_w, fcc_b, detach=True)
        want_x = ctx.needs_input_grad[0]
        # (vals sharing feats' memory IS v = Identity to the kernels: the rows' gradient then already holds A gB)
        same = ctx.has_vals and vals.data_ptr() == feats.data_ptr()
        want_v = ctx.has_vals and ctx.needs_input_grad[2] and not (want_x and same)
        if ctx.proj:
            want_v = ctx.needs_input_grad[14] or ctx.needs_input_grad[15]
        kw = dict(g_classes=None if ctx.has_cin else g_cls, g_A=g_A, vals=vals if ctx.has_vals else None,
                  nonlinear=ctx.nonlinear, want_g_vals=want_v, want_g_feats=want_x)
        if ctx.lengths is None:
            g = ops.agg_backward(feats, w, A, B, idx, g_pred, g_B=g_B[0] if g_B is not None else None, **kw)
        else:
            g = ops.agg_backward_bags(feats, ctx.lengths, w, A, B, idx, g_pred, g_B=g_B, **kw)
        if ctx.proj:
            g_v_w = g_v_b = None
            if want_v:   # g["vals"]: fp32, as the aggregator backward wrote it — one call over all rows of the batch
                g_v_w, g_v_b = (t.to(ctx.v_dtype) for t in ops.value_proj_backward(feats, vals, g["vals"]))
            return (None, None, None, None, *_param_grads(g, w), None, None, g_v_w, g_v_b)
        return (g.get("feats"), None, g.get("vals"), None, *_param_grads(g, w), None, None, None, None)

    @staticmethod
    def _backward_dense(ctx, g_cls, g_pred, g_A, g_B):
        """The fallback for what the native call rejects when the gradient of the INPUT rows is requested (_native_accepts:
        misaligned query biases): the same analytic gradient composed from dense GPU products.  No fp32 CUDA route of
        FCLayer + BClassifier with ordinary parameters reaches it."""
        feats, vals, fc_w, q0_w, q0_b, q2_w, q2_b, fcc_w, A, B, idx = ctx.saved_tensors[:11]
        x = feats
        V = vals if ctx.has_vals else feats
        idx = idx[0]
        scale = Q_DIM ** -0.5
        C = fcc_w.shape[0]
        zeros = torch.zeros
        g_pred = g_pred if g_pred is not None else zeros((1, C), device=x.device)
        # ---- bag head
        g_fcc_b = g_pred[0]
        g_fcc_w = g_pred[0][:, None, None] * B[0][None]
        gB = torch.einsum("o,ock->ck", g_pred[0], fcc_w)
        if g_B is not None:
            gB = gB + g_B[0]
        gA = V.mm(gB.t())
        if g_A is not None:
            gA = gA + g_A
        gs = A * (gA - (A * gA).sum(0, keepdim=True)) * scale
        # ---- recompute the query stream
        pre1 = F.linear(x, q0_w, q0_b)
        if ctx.nonlinear:
            h1 = pre1.clamp_min(0)
            Q = torch.tanh(F.linear(h1, q2_w, q2_b))
        else:
            Q = pre1
        qmax = Q[idx]
        gQ = gs.mm(qmax)
        gQ.index_add_(0, idx, gs.t().mm(Q))
        if ctx.nonlinear:
            gz2 = gQ * (1 - Q * Q)
            g_q2_w = gz2.t().mm(h1)
            g_q2_b = gz2.sum(0)
            gh1 = gz2.mm(q2_w) * (pre1 > 0)
        else:
            g_q2_w = g_q2_b = None
            gh1 = gQ
        g_q0_w = gh1.t().mm(x)
        g_q0_b = gh1.sum(0)
        # ---- instance stream (FCLayer fused in) and inputs
        g_fc_w = g_fc_b = g_cin = None
        if ctx.has_cin:
            g_cin = None  # c only feeds the (non-differentiable) indices: dsmil.py:52
        elif g_cls is not None:
            g_fc_w = g_cls.t().mm(x)
            g_fc_b = g_cls.sum(0)
        g_x = g_vals = None
        if ctx.needs_input_grad[0]:
            g_x = gh1.mm(q0_w)
            if not ctx.has_cin and g_cls is not None:
                g_x = g_x + g_cls.mm(fc_w)
            if not ctx.has_vals:
                g_x = g_x + A.mm(gB)
        if ctx.has_vals and ctx.needs_input_grad[2]:
            g_vals = A.mm(gB)
        return (g_x, g_cin, g_vals, None, g_fc_w, g_fc_b, g_q0_w, g_q0_b, g_q2_w, g_q2_b,
                g_fcc_w, g_fcc_b, None, None, None, None)
