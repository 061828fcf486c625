"""Post-training phase of the 2stg+ setting (Code/sage+gat+diffpool/train_triplet_pre_train.py:196-270): after the triplet
pre-training the reference replaces ``model.map2_model`` by Linear(output_dim, 64) - LeakyReLU - Linear(64, 32) - LeakyReLU -
Linear(32, 2) and runs one Adam step per ANCHOR graph at B = 1 on ``F.cross_entropy(F.softmax(pred), label)`` (the soft-max applied
twice, kept literally), thousands of times per epoch, without gradient clipping (``FlatTrainer(clip=0)``).

    head = post_train.install_head(model)                    # :201-210, BEFORE the FlatTrainer is built (its bucket holds the new weights)
    loss, pred, out = post_train.post_train_step(model, g)   # :240-256 on one graph object, eager
    st = post_train.PostTrainStream(model, graphs)           # or: the whole epoch replayed from ONE hipGraph
    gs = GraphedStep(FlatTrainer(model, lr=1e-3, clip=0), st.step_loss()); st.load(anchors); gs.step() ...

``map_model``, the three layers, both soft-maxes and the loss are one launch forward and one backward (csrc/posttrain_head.hip) on the
readout rows of the conv stack; the label of a streamed step is read on the device from the index the gather launch wrote
(``ids_out``), so a replayed step needs no host word.  ``two_stage.evaluate_pred`` is the phase's ``evaluate()`` (:36-72).

The driver's other two methods: ``diffpool_stream.PostTrainStream`` (``SoftPoolingGcnEncoder``: the same head on the readout rows of every
level; ``PostTrainSteps`` is what the two share) and ``gat_stream.PostTrainStream`` (``DGATEncoderGraph(final_dim='output_dim')`` returns its
readout row first, so ``pred`` is that row: ``row_loss`` on it, ``evaluate_readout`` for ``evaluate()``).  ``post_train_step`` has a resident
branch for each.

The other two drivers of the reference, whose post-training step is the "original" setting's classification step at B = 1 (their
replacement heads are dead code: the models' ``forward`` never reads them):
``sag_stream.PostTrainStream`` / ``sag_stream.post_train_step`` / ``sag_stream.test_dataset`` for ``sag_layers.Net``
(Code/sag/train_triplet_pre_train.py:219-263: ``F.nll_loss(model(data), data.y)``, a new Adam without clipping), and
``eigen_stream.PostTrainStream`` / ``eigen_stream.post_train_step`` / ``eigen_stream.evaluate_pred`` for ``WavePoolingGcnEncoder``
(Code/eigengcn/train_triplet_pre_train.py:170-249: ``model.loss(ypred, label)`` stepped by the TRIPLET phase's own Adam).  Their heads
live here: ``apply_mlp3_nll`` and ``apply_mlp2_ce`` (csrc/posttrain_cls.hip: the head, its soft-max and the loss in one launch each
way, the label read on the device).
"""
import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _native as nat
from . import message_passing as mp
from . import resident as R
from .triplet_stream import SageArenaStream, _graph_dict, check_schedule

EAGER = "; use the eager drop-in, post_train.post_train_step(model, graph)"


# ----------------------------------------------------------------------------- the replacement head
def make_head(output_dim, hidden=(64, 32), n_classes=2, device=None):
    """the reference's ``pred_model`` (:201-208).  The three ``nn.Linear`` are constructed on the host, in the reference's order, under
    torch's global generator (the reference builds each on the host before its ``.cuda()``: the same draws), then moved to ``device``
    (default: the current GPU when there is one)"""
    if len(hidden) != 2 or min(int(h) for h in hidden) < 1 or int(n_classes) < 2:
        raise ValueError("hidden must be two positive widths and n_classes at least 2")
    h1, h2 = int(hidden[0]), int(hidden[1])
    lin1 = nn.Linear(int(output_dim), h1)
    lin2 = nn.Linear(h1, h2)
    lin3 = nn.Linear(h2, int(n_classes))
    seq = nn.Sequential(lin1, nn.LeakyReLU(), lin2, nn.LeakyReLU(), lin3)
    if device is None:
        from .dense_encoders import _default_device
        device = _default_device()
    return seq.to(device)


def install_head(model, head=None):
    """``model.map2_model = pred_model`` (:210) on the model's device; returns the head.  Call it before a ``FlatTrainer`` is built, so
    the new parameters lie in its bucket"""
    dev = next(model.parameters()).device
    if head is None:
        head = make_head(model.map_model.out_features, device=dev)
    model.map2_model = head.to(dev)
    return model.map2_model


def head_layers(model):
    """(map_model, lin1, lin2, lin3, negative_slope) when ``map_model`` is a Linear and ``map2_model`` is Linear - LeakyReLU - Linear -
    LeakyReLU - Linear with biases and matching widths, else None"""
    lin0, seq = getattr(model, "map_model", None), getattr(model, "map2_model", None)
    if not isinstance(lin0, nn.Linear) or not isinstance(seq, nn.Sequential) or len(seq) != 5:
        return None
    l1, a1, l2, a2, l3 = seq
    if not all(isinstance(m, nn.Linear) for m in (l1, l2, l3)) or not all(isinstance(m, nn.LeakyReLU) for m in (a1, a2)):
        return None
    if a1.negative_slope != a2.negative_slope or any(m.bias is None for m in (lin0, l1, l2, l3)):
        return None
    if l1.in_features != lin0.out_features or l2.in_features != l1.out_features or l3.in_features != l2.out_features:
        return None
    return lin0, l1, l2, l3, float(a1.negative_slope)


def _layers_fit(layers, rows, dev):
    """the library takes these layers on ``rows`` readout rows: fp32, contiguous, 16-byte aligned tensors on ``dev``, supported widths"""
    if layers is None or dev.type != "cuda":
        return False
    lin0, l1, l2, l3, _ = layers
    for m in (lin0, l1, l2, l3):
        for t in (m.weight, m.bias):
            if t.dtype != torch.float32 or not t.is_contiguous() or t.data_ptr() % 16 or t.device != dev:
                return False
    return bool(nat.lib().tsgnn_posttrain_head_supported(lin0.in_features, lin0.out_features, l1.out_features, l2.out_features,
                                                         l3.out_features, int(rows)))


def head_ok(model, r):
    """the fused head applies to the readout rows ``r`` of ``model``; otherwise the torch composition of the same expression is used"""
    layers = head_layers(model)
    return (layers is not None and r is not None and r.is_cuda and r.dim() == 2 and r.dtype == torch.float32 and r.stride(1) == 1
            and r.stride(0) % 4 == 0 and r.stride(0) >= r.size(1) and r.data_ptr() % 16 == 0 and r.size(1) == layers[0].in_features
            and _layers_fit(layers, r.size(0), r.device))


class _PostTrainHead(torch.autograd.Function):
    """(readout rows r [R, P], ids [R] int32, label table int32, slope, the eight head parameters) -> (loss, logits [R, C], out [R, E]):
    tsgnn_posttrain_head_fwd_f32 / _bwd_f32.  ``logits`` and ``out`` are not differentiable (the reference's step reads them only)."""

    @staticmethod
    def forward(ctx, r, ids, labels, slope, w0, b0, w1, b1, w2, b2, w3, b3):
        R_, P = int(r.size(0)), int(r.size(1))
        E, h1, h2, C = int(w0.size(0)), int(w1.size(0)), int(w2.size(0)), int(w3.size(0))
        dev = r.device
        new = lambda *s: torch.empty(*s, dtype=torch.float32, device=dev)
        out, z1, z2, z, p, loss = new(R_, E), new(R_, h1), new(R_, h2), new(R_, C), new(R_, C), new(1)
        nat.call("posttrain_head_fwd_f32", r, r.stride(0), R_, P, w0, b0, E, w1, b1, h1, w2, b2, h2, w3, b3, C, float(slope), ids, labels,
                 int(labels.numel()), out, z1, z2, z, p, loss)
        ctx.save_for_backward(r, w0, w1, w2, w3, out, z1, z2, p, ids, labels)
        ctx.params = (w0, b0, w1, b1, w2, b2, w3, b3)         # (the Parameter objects: their slices of a trainer's flat gradient bucket)
        ctx.slope = float(slope)
        ctx.set_materialize_grads(False)
        ctx.mark_non_differentiable(z, out)
        return loss.view(()), z, out

    @staticmethod
    def backward(ctx, g, _gz, _gout):
        if g is None:
            return (None,) * 12
        r, w0, w1, w2, w3, out, z1, z2, p, ids, labels = ctx.saved_tensors
        R_, P = int(r.size(0)), int(r.size(1))
        E, h1, h2, C = int(w0.size(0)), int(w1.size(0)), int(w2.size(0)), int(w3.size(0))
        dev = r.device
        g = g.contiguous().float()                                # the upstream gradient stays on the device
        d_r = torch.empty(R_, P, dtype=torch.float32, device=dev) if ctx.needs_input_grad[0] else None
        # straight into the trainer's flat gradient bucket when one is installed (FlatTrainer): no AccumulateGrad copy, no zeroing
        bufs, grads = mp._sinks_or_new(ctx.params, ((E, P), (E,), (h1, E), (h1,), (h2, h1), (h2,), (C, h2), (C,)), dev)
        nat.call("posttrain_head_bwd_f32", r, r.stride(0), R_, P, w0, E, w1, h1, w2, h2, w3, C, ctx.slope, ids, labels, int(labels.numel()),
                 out, z1, z2, p, g, d_r, P, *bufs)
        return (d_r, None, None, None) + grads


def head_torch(model, r, label):
    """the same expression as torch modules (:249-256 after the readout): -> (loss, pred, out)"""
    out = model.map_model(r)
    pred = model.map2_model(out)
    return F.cross_entropy(F.softmax(pred, dim=1), label), pred, out


def apply_head(model, r, ids, labels):
    """readout rows -> (loss, pred, out): the fused head where ``head_ok``, else ``head_torch`` on ``labels[ids]``"""
    if head_ok(model, r):
        lin0, l1, l2, l3, slope = head_layers(model)
        return _PostTrainHead.apply(r, ids, labels, slope, lin0.weight, lin0.bias, l1.weight, l1.bias, l2.weight, l2.bias, l3.weight, l3.bias)
    return head_torch(model, r, labels[ids.long()].long())


# ----------------------------------------------------------------------------- the loss on rows that ARE `pred` (the GAT encoder)
def row_loss_ok(z):
    """the row-loss launches take the rows ``z`` [R, C]: fp32 on the GPU, unit column stride, widths of ``tsgnn_posttrain_rowloss_supported``"""
    return (z is not None and z.is_cuda and z.dim() == 2 and z.dtype == torch.float32 and z.stride(1) == 1 and z.stride(0) >= z.size(1)
            and bool(nat.lib().tsgnn_posttrain_rowloss_supported(int(z.size(1)), int(z.size(0)))))


class _RowLoss(torch.autograd.Function):
    """(rows z [R, C], ids [R] int32, label table int32) -> ``F.cross_entropy(F.softmax(z), labels[ids])``, the label read on the
    device: tsgnn_posttrain_rowloss_fwd_f32 / _bwd_f32, one launch each way"""

    @staticmethod
    def forward(ctx, z, ids, labels):
        R_, C = int(z.size(0)), int(z.size(1))
        p = torch.empty(R_, C, dtype=torch.float32, device=z.device)
        loss = torch.empty(1, dtype=torch.float32, device=z.device)
        nat.call("posttrain_rowloss_fwd_f32", z, z.stride(0), R_, C, ids, labels, int(labels.numel()), p, loss)
        ctx.save_for_backward(p, ids, labels)
        ctx.set_materialize_grads(False)
        return loss.view(())

    @staticmethod
    def backward(ctx, g):
        if g is None:
            return None, None, None
        p, ids, labels = ctx.saved_tensors
        R_, C = int(p.size(0)), int(p.size(1))
        dz = torch.empty(R_, C, dtype=torch.float32, device=p.device)
        nat.call("posttrain_rowloss_bwd_f32", p, R_, C, ids, labels, int(labels.numel()), g.contiguous().float(), dz, C)
        return dz, None, None


def row_loss(z, ids, labels):
    """the step's loss on rows that are the reference's ``pred`` themselves (``DGATEncoderGraph``, final_dim 'output_dim'): the fused
    pair where ``row_loss_ok``, else the torch expression on ``labels[ids]``"""
    if row_loss_ok(z):
        return _RowLoss.apply(z, ids, labels)
    return F.cross_entropy(F.softmax(z, dim=1), labels[ids.long()].long())


# ----------------------------------------------------------------------------- the classification heads of SAGPool and EigenGCN
def _rows_fit(r):
    """readout rows the head launches take as they are: fp32 on the GPU, unit column stride, 16-byte rows, at most 8 of them"""
    return (r is not None and r.is_cuda and r.dim() == 2 and r.dtype == torch.float32 and r.stride(1) == 1 and r.stride(0) % 4 == 0
            and r.stride(0) >= r.size(1) and r.data_ptr() % 16 == 0 and 1 <= r.size(0) <= 8)


def _dense_f32(*tensors):
    return all(t is None or (t.dtype == torch.float32 and t.is_contiguous() and t.is_cuda) for t in tensors)


def mlp3_nll_ok(model, r):
    """``tsgnn_posttrain_mlp3_nll_*`` take the head ``lin1 / lin2 / lin3`` of ``model`` (a ``sag_layers.Net``) on the readout rows ``r``"""
    lins = [getattr(model, k, None) for k in ("lin1", "lin2", "lin3")]
    if not (all(isinstance(l, nn.Linear) for l in lins) and _rows_fit(r) and r.size(1) == lins[0].in_features):
        return False
    if not _dense_f32(*[t for l in lins for t in (l.weight, l.bias)]) or any(l.weight.data_ptr() % 16 for l in lins):
        return False
    return bool(nat.lib().tsgnn_posttrain_mlp3_nll_supported(int(lins[0].in_features), int(lins[0].out_features), int(lins[1].out_features),
                                                             int(lins[2].out_features), int(r.size(0))))


class _Mlp3Nll(torch.autograd.Function):
    """(readout rows r [R, D0], ids [R] int32, label table int32, lin1 / lin2 / lin3 weights and biases, (p, seed, state, used) or None)
    -> (loss, logp [R, C]): ``F.nll_loss(log_softmax(lin3(relu(lin2(dropout(relu(lin1(r))))))), labels[ids])``, one launch each way
    (tsgnn_posttrain_mlp3_nll_fwd_f32 / _bwd_f32).  ``logp`` is the step's ``out``: read only, not differentiable."""

    @staticmethod
    def forward(ctx, r, ids, labels, w1, b1, w2, b2, w3, b3, drop):
        R_, D0, D1, D2, C = int(r.size(0)), int(w1.size(1)), int(w1.size(0)), int(w2.size(0)), int(w3.size(0))
        dev = r.device
        new = lambda *s: torch.empty(*s, dtype=torch.float32, device=dev)
        a1, a2, logp, loss = new(R_, D1), new(R_, D2), new(R_, C), new(1)
        p_, seed, state, used = drop if drop is not None else (0.0, 0, None, None)
        nat.call("posttrain_mlp3_nll_fwd_f32", r, r.stride(0), R_, w1, b1, float(p_), int(seed), state, used, w2, b2, w3, b3, D0, D1, D2, C,
                 ids, labels, int(labels.numel()), a1, a2, logp, loss)
        ctx.save_for_backward(r, w1, w2, w3, a1, a2, logp, ids, labels)
        ctx.keep_scale = 1.0 / (1.0 - float(p_))
        ctx.params = (w1, b1, w2, b2, w3, b3)                 # (the Parameter objects: their slices of a trainer's flat gradient bucket)
        ctx.set_materialize_grads(False)
        ctx.mark_non_differentiable(logp)
        return loss.view(()), logp

    @staticmethod
    def backward(ctx, g, _glogp):
        if g is None:
            return (None,) * 10
        r, w1, w2, w3, a1, a2, logp, ids, labels = ctx.saved_tensors
        R_, D0, D1, D2, C = int(r.size(0)), int(w1.size(1)), int(w1.size(0)), int(w2.size(0)), int(w3.size(0))
        dev = r.device
        d_r = torch.empty(R_, D0, dtype=torch.float32, device=dev) if ctx.needs_input_grad[0] else None
        # straight into the trainer's flat gradient bucket when one is installed (FlatTrainer): no AccumulateGrad copy, no zeroing
        bufs, grads = mp._sinks_or_new(ctx.params, ((D1, D0), (D1,), (D2, D1), (D2,), (C, D2), (C,)), dev)
        nat.call("posttrain_mlp3_nll_bwd_f32", r, r.stride(0), R_, w1, w2, w3, D0, D1, D2, C, ctx.keep_scale, ids, labels,
                 int(labels.numel()), a1, a2, logp, g.contiguous().float(), d_r, D0, *bufs)
        return (d_r, None, None) + grads + (None,)


def mlp3_nll_torch(model, r, label):
    """the same expression as torch operators (network.py:48-53 + ``F.nll_loss``) -> (loss, logp)"""
    h = F.relu(F.linear(r, model.lin1.weight, model.lin1.bias))
    h = F.dropout(h, p=model.dropout_ratio, training=model.training)
    h = F.relu(F.linear(h, model.lin2.weight, model.lin2.bias))
    logp = F.log_softmax(F.linear(h, model.lin3.weight, model.lin3.bias), dim=-1)
    return F.nll_loss(logp, label), logp


def apply_mlp3_nll(model, r, ids, labels, drop=None):
    """readout rows of a ``sag_layers.Net`` -> (loss, out): the fused head where ``mlp3_nll_ok``, else ``mlp3_nll_torch`` on
    ``labels[ids]``.  ``drop``: the (p, seed, state, used) words of the in-launch mask for an active dropout (train mode, p > 0); when
    none is given they are ``sag_triplet._in_kernel_dropout``'s (the process seed and device counter every mlp3 launch shares), and a
    counter that would have to be created inside a stream capture sends the call to the torch expression"""
    if mlp3_nll_ok(model, r):
        if model.training and model.dropout_ratio > 0.0 and drop is None:
            from .sag_triplet import _in_kernel_dropout
            drop = _in_kernel_dropout(model.dropout_ratio, r.device)
            if drop is None:
                return mlp3_nll_torch(model, r, labels[ids.long()].long())
        if not (model.training and model.dropout_ratio > 0.0):
            drop = None
        m = model
        return _Mlp3Nll.apply(r, ids, labels, m.lin1.weight, m.lin1.bias, m.lin2.weight, m.lin2.bias, m.lin3.weight, m.lin3.bias, drop)
    return mlp3_nll_torch(model, r, labels[ids.long()].long())


def mlp2_layers(model):
    """(lin1, lin2) when ``model.pred_model`` is Linear - ReLU - Linear (``WavePoolingGcnEncoder`` with one hidden width), else None"""
    seq = getattr(model, "pred_model", None)
    if not isinstance(seq, nn.Sequential) or len(seq) != 3:
        return None
    l1, act, l2 = seq
    if not (isinstance(l1, nn.Linear) and isinstance(act, nn.ReLU) and isinstance(l2, nn.Linear)) or l2.in_features != l1.out_features:
        return None
    return l1, l2


def mlp2_ce_ok(model, r):
    """``tsgnn_posttrain_mlp2_ce_*`` take ``model.pred_model`` on the readout rows ``r``"""
    layers = mlp2_layers(model)
    if layers is None or not _rows_fit(r) or r.size(1) != layers[0].in_features:
        return False
    l1, l2 = layers
    if not _dense_f32(l1.weight, l1.bias, l2.weight, l2.bias) or l1.weight.data_ptr() % 16:
        return False
    return bool(nat.lib().tsgnn_posttrain_mlp2_ce_supported(int(l1.in_features), int(l1.out_features), int(l2.out_features), int(r.size(0))))


class _Mlp2Ce(torch.autograd.Function):
    """(readout rows r [R, D], ids [R] int32, label table int32, W1, b1, W2, b2) -> (loss, ypred [R, C]):
    ``F.cross_entropy(pred_model(r), labels[ids])`` for pred_model = Linear - ReLU - Linear, one launch each way
    (tsgnn_posttrain_mlp2_ce_fwd_f32 / _bwd_f32).  ``ypred`` is read only: not differentiable."""

    @staticmethod
    def forward(ctx, r, ids, labels, w1, b1, w2, b2):
        R_, D, H, C = int(r.size(0)), int(w1.size(1)), int(w1.size(0)), int(w2.size(0))
        dev = r.device
        new = lambda *s: torch.empty(*s, dtype=torch.float32, device=dev)
        h, z, p, loss = new(R_, H), new(R_, C), new(R_, C), new(1)
        nat.call("posttrain_mlp2_ce_fwd_f32", r, r.stride(0), R_, w1, b1, w2, b2, D, H, C, ids, labels, int(labels.numel()), h, z, p, loss)
        ctx.save_for_backward(r, w1, w2, h, p, ids, labels)
        ctx.params = (w1, b1, w2, b2)
        ctx.set_materialize_grads(False)
        ctx.mark_non_differentiable(z)
        return loss.view(()), z

    @staticmethod
    def backward(ctx, g, _gz):
        if g is None:
            return (None,) * 7
        r, w1, w2, h, p, ids, labels = ctx.saved_tensors
        R_, D, H, C = int(r.size(0)), int(w1.size(1)), int(w1.size(0)), int(w2.size(0))
        dev = r.device
        d_r = torch.empty(R_, D, dtype=torch.float32, device=dev) if ctx.needs_input_grad[0] else None
        bufs, grads = mp._sinks_or_new(ctx.params, ((H, D), (H,), (C, H), (C,)), dev)
        nat.call("posttrain_mlp2_ce_bwd_f32", r, r.stride(0), R_, w1, w2, D, H, C, ids, labels, int(labels.numel()), h, p,
                 g.contiguous().float(), d_r, D, *bufs)
        return (d_r, None, None) + grads


def apply_mlp2_ce(model, r, ids, labels):
    """readout rows of a ``WavePoolingGcnEncoder`` -> (loss, ypred): the fused head where ``mlp2_ce_ok``, else ``pred_model`` and
    ``model.loss`` (``mp.cross_entropy``) composed on ``labels[ids]``"""
    if mlp2_ce_ok(model, r):
        l1, l2 = mlp2_layers(model)
        return _Mlp2Ce.apply(r, ids, labels, l1.weight, l1.bias, l2.weight, l2.bias)
    ypred = model.pred_model(r)
    return model.loss(ypred, labels[ids.long()].long()), ypred


def readout_out(model, pred):
    """``out = map2_model(map_model(pred))`` of a ``DGATEncoderGraph`` step (encoders_GAT.py:191-198): the reference's loop binds it and
    never reads it, so it is computed outside the autograd graph"""
    with torch.no_grad():
        return model.map2_model(model.map_model(pred.detach()))


def _readout(model, x, g, sizes, assign_x):
    """the model up to its concatenated readout rows under the statistics of a B = 1 call (``_heads`` honours ``_defer_map`` for
    "pretrain"); the flag is put back on every exit path"""
    prev = getattr(model, "_defer_map", False)
    model._defer_map = True
    try:
        with R.per_graph_statistics(model):
            return model(x, g, sizes, assign_x=assign_x)[1]
    finally:
        model._defer_map = prev


# ----------------------------------------------------------------------------- the eager step
_consts = {}


def _const_i32(dev, value):
    """a cached one-element int32 device tensor (row 0's index, a label): uploaded once per value, not per step"""
    key = (dev.type, dev.index, int(value))
    t = _consts.get(key)
    if t is None:
        t = _consts[key] = torch.tensor([int(value)], dtype=torch.int32, device=dev)
    return t


def _label_of(d, what="graph"):
    if "label" not in d:
        raise ValueError("%s carries no 'label'" % what)
    a = np.asarray(d["label"])
    if a.size != 1 or not np.issubdtype(a.dtype, np.integer):
        raise ValueError("%s: 'label' must be one integer; got %r" % (what, d["label"]))
    return int(a.reshape(-1)[0])


def post_train_step(model, graph):
    """forward of the reference's post-training step (:240-256) on one graph object (``.graph`` = {'adj', 'feats', 'num_nodes',
    'assign_feats', 'label'}) -> (loss, pred, out); the caller runs ``backward`` and the optimiser.  A plain ``GcnEncoderGraph`` with
    final_dim "pretrain" takes the graph's resident pieces from the model's ``ResidentCache`` and applies the fused head to its readout
    row; so does a ``SoftPoolingGcnEncoder`` (its rows hold every level's readout: P = pred_input_dim * (num_pooling + 1)).
    A ``gat_encoders.DGATEncoderGraph`` with final_dim "output_dim" (no dropout active, a graph one ghost representative stands
    for) takes its resident piece through ``gat_triplet.assemble`` at B = 1: ``pred`` is the max-readout row itself
    (encoders_GAT.py:189-198: the model returns it first), the loss is ``row_loss`` over its ``embedding_dim`` columns, ``map_model`` and
    ``map2_model`` receive no gradient and ``out`` is computed outside the autograd graph; a label >= ``embedding_dim`` is a ValueError.
    Any other model gets the module call on the dense arrays and the torch expression."""
    from . import gat_triplet as GT
    from . import triplet as T
    from .dense_encoders import GcnEncoderGraph, SoftPoolingGcnEncoder
    from .gat_encoders import DGATEncoderGraph
    dev = next(model.parameters()).device
    d = graph.graph
    label = _label_of(d)
    if isinstance(model, DGATEncoderGraph) and model.final_dim == "output_dim":
        if not 0 <= label < int(model.pred_input_dim):
            raise ValueError("label %d lies outside [0, %d): pred is the readout row of embedding_dim columns" % (label, model.pred_input_dim))
        if GT.packable(model, dev):
            piece = GT.resident_piece(graph, dev, R.resident_cache(model))
            if piece.exact:
                x, g = GT.assemble([piece], dev, GT.head_counts(model))
                pred = GT.readout_rows(model, x, g)
                return row_loss(pred, _const_i32(dev, 0), _const_i32(dev, label)), pred, readout_out(model, pred)
    if (R.RESIDENT and dev.type == "cuda" and type(model) in (GcnEncoderGraph, SoftPoolingGcnEncoder) and model.final_dim == "pretrain"
            and isinstance(getattr(model, "map_model", None), nn.Linear)):
        g, x, xa, sizes = T.assemble([T.resident_graph(graph, dev, R.resident_cache(model))], dev)
        r = _readout(model, x, g, sizes, x if xa is None else xa)
        return apply_head(model, r, _const_i32(dev, 0), _const_i32(dev, label))
    adj = torch.as_tensor(np.asarray(d["adj"], dtype=np.float32)[None], device=dev)
    h0 = torch.as_tensor(np.asarray(d["feats"], dtype=np.float32)[None], device=dev)
    assign = torch.as_tensor(np.asarray(d["assign_feats"], dtype=np.float32), device=dev) if "assign_feats" in d else h0
    pred, out = model(h0, adj, np.array([int(d["num_nodes"])]), assign_x=assign)
    return F.cross_entropy(F.softmax(pred, dim=1), torch.tensor([label], device=dev)), pred, out


# ----------------------------------------------------------------------------- the streamed step
def label_table(graphs, n_classes):
    """int32 [G] of ``graph['label']``; ValueError, naming the graph's index, for a label that is no integer in [0, n_classes)"""
    out = np.zeros(len(graphs), dtype=np.int32)
    for i, obj in enumerate(graphs):
        y = _label_of(_graph_dict(obj), "graph %d" % i)
        if not 0 <= y < int(n_classes):
            raise ValueError("graph %d: label %d lies outside [0, %d)" % (i, y, int(n_classes)))
        out[i] = y
    return out


def check_anchors(anchors, n_graphs):
    """[T] or [T, 1] integer indices into the dataset -> contiguous int32 [T, 1] (``triplet_stream.check_schedule``'s refusals)"""
    s = np.asarray(anchors)
    if s.ndim == 1:
        s = s.reshape(-1, 1)
    return check_schedule(s, n_graphs, 1)


class AnchorSteps:
    """What every family's post-training stream shares: a schedule entry names ONE graph (``check_anchors``), and the callable for
    ``GraphedStep`` is the loss of the family's ``step()``.  ``STEP_ARGS``: what ``step_loss()`` passes to ``step``."""

    STEP_ARGS = {}

    def _checked(self, anchors):
        return check_anchors(anchors, self.arena.n_graphs)

    def step_loss(self):
        """-> callable for ``GraphedStep``: every call (every replay) consumes the next entry and returns its loss"""
        def step():
            return self.step(**self.STEP_ARGS)[0]
        return step


class PostTrainSteps(AnchorSteps):
    """What the post-training streams over a ``SageArenaStream`` at ``batch=1`` share (this module's for the plain ``GcnEncoderGraph``,
    ``diffpool_stream.PostTrainStream`` for DiffPool): the final_dim and head refusals, the device label table and the step — the
    model's concatenated readout rows under per-graph statistics with ``_defer_map``, then the fused head, whose label is
    ``labels[ids_out[0]]`` read on the device.  ``SIZES``: what the model's forward gets as ``batch_num_nodes``;
    ``_readout_width(model)``: the columns of its concatenated readout rows."""

    SIZES = None

    def _readout_width(self, model):
        return int(model.pred_input_dim)

    def _init_post_train(self, model, graphs):
        if model.final_dim != "pretrain":
            self._refuse("takes a model with final_dim = 'pretrain'")
        layers = head_layers(model)
        P = self._readout_width(model)
        if not _layers_fit(layers, 1, self.device) or layers[0].in_features != P or P % 4:
            raise TypeError("%s: map_model / map2_model are not the head the fused launches take (post_train.install_head)%s"
                            % (self.NAME, self.EAGER))
        self.n_classes = int(layers[3].out_features)
        self.labels = torch.from_numpy(label_table(graphs, self.n_classes)).to(self.device)
        self._warm_up_schedule()

    def step(self):
        """gather launch + the stack's readout row + the head -> (loss, pred, out) of the cursor's entry"""
        self.gather()
        r = _readout(self.model, self.x, self.g, self.SIZES, self.x)
        if not head_ok(self.model, r):
            raise RuntimeError("%s: the fused head does not take this model's readout rows%s" % (self.NAME, self.EAGER))
        return apply_head(self.model, r, self.ids_out, self.labels)


class PostTrainStream(PostTrainSteps, SageArenaStream):
    """An epoch of post-training steps from ONE hipGraph: the arena of ``triplet_stream.pack_arena(..., batch=1)``, a device label
    table, and per replay the gather launch (the anchor of "schedule entry number cursor"), the fused per-graph conv stack on the
    gathered capacity-padded batch and the fused head, whose label is ``labels[ids_out[0]]`` read on the device.

    ``model``: what ``TripletStream`` takes (a plain ``GcnEncoderGraph`` with concat and bn whose stack runs as the fused node on the
    gathered batch) with final_dim "pretrain" and the installed head of ``head_ok``'s shape; anything else is a TypeError pointing to
    ``post_train_step``.  ``load(anchors)``: [T] or [T, 1] indices into ``graphs`` (``schedule_of(sampler, graphs)[:, :1]`` is the
    reference's epoch).  ``step_loss()`` is the callable for ``GraphedStep``.  ``max_steps``: as ``TripletStream``.
    ``gat_stream.PostTrainStream`` and ``diffpool_stream.PostTrainStream`` are the same phase for the other two methods of the driver."""

    NAME = "PostTrainStream"
    EAGER = EAGER

    def __init__(self, model, graphs, nmax=None, max_steps=None):
        graphs = list(graphs)
        super().__init__(model, graphs, 1, nmax, max_steps)
        self._init_post_train(model, graphs)


# ----------------------------------------------------------------------------- evaluate() of a model whose `pred` is its readout row
def predict_readout(graphs, model, chunk=None):
    """class index per graph, int32 on the model's device: the argmax (a tie to the lowest index) of the readout row of a
    ``gat_encoders.DGATEncoderGraph`` — the reference's ``evaluate()`` (train_triplet_pre_train.py:36-72) takes ``torch.max`` of the
    model's FIRST output, which for final_dim 'output_dim' is that row.  The rows come from the packed chunks ``two_stage.embed_dataset``
    builds for GAT (``gat_triplet.assemble`` of resident pieces; a chunk holding a graph that cannot be packed takes one dense B = 1
    call per graph), in eval mode without autograd"""
    from . import gat_triplet as GT
    from . import two_stage as TS
    from .gat_encoders import DGATEncoderGraph
    if not isinstance(model, DGATEncoderGraph):
        raise TypeError("predict_readout takes a gat_encoders.DGATEncoderGraph; two_stage.predict_dataset serves the other encoders")
    graphs = TS._flatten(graphs)
    dev = next(model.parameters()).device
    if not graphs:
        return torch.zeros(0, dtype=torch.int32, device=dev)
    step = int(chunk) if chunk is not None else GT.DEFAULT_CHUNK
    if step < 1:
        raise ValueError("chunk must be at least 1")
    cache, rows = R.cache_for(model), []
    with TS._eval_mode(model):
        for i in range(0, len(graphs), step):
            part = graphs[i:i + step]
            pieces = [GT.resident_piece(o, dev, cache) for o in part] if GT.packable(model, dev) else None
            if pieces is not None and all(q.exact for q in pieces):
                rows.append(GT.readout_rows(model, *GT.assemble(pieces, dev, GT.head_counts(model))))
            else:
                for o in part:
                    dd = o.graph
                    adj = torch.as_tensor(np.asarray(dd["adj"], dtype=np.float32)[None], device=dev)
                    h0 = torch.as_tensor(np.asarray(dd["feats"], dtype=np.float32)[None], device=dev)
                    rows.append(model(h0, adj, None)[0])
        z = torch.cat(rows)
    return (z == z.max(dim=1, keepdim=True).values).int().argmax(dim=1).int()      # (the first maximum: the lowest index)


def evaluate_readout(graphs, model, chunk=None):
    """``two_stage.evaluate_pred`` for a model whose ``pred`` is its readout row (``predict_readout``): the same metrics dictionary
    {'prec' (macro), 'recall' (macro), 'acc', 'F1' (micro)} against ``graph.graph['label']``"""
    from . import two_stage as TS
    graphs = TS._flatten(graphs)
    y = TS._labels(graphs).reshape(-1)
    pred = predict_readout(graphs, model, chunk).cpu().numpy().astype(np.int64)
    labels = np.unique(np.concatenate([y.astype(np.int64), pred]))
    return TS.metrics_from_confusion(TS.confusion_matrix(y, pred, labels))
