"""SAGPool triplet stream: a NEW triplet at every replay of ONE hipGraph for ``sag_triplet.tripletnet`` over ``sag_layers.Net``
(Code/sag/train_triplet.py:198-214: ``tripletsampler_tr.sampler()`` -> ``TNet(a, p, n)`` -> margin loss -> Adam, thousands of times
per epoch).

``triplet_stream.TripletStream`` does this for the GraphSage family and ``diffpool_stream.TripletStream`` for DiffPool.  Here the
dataset's ``Data`` objects are packed once into a device-resident arena (``pack_arena``), an epoch's triplets go up as one index array
(``load``), and the step's first launch (``tsgnn_sag_triplet_gather_f32``, csrc/sag_stream.hip) writes the batch of "schedule entry
number ``cursor``" — CSR, feature rows, gcn_norm coefficients and the graph pointer of every pooled level — padded to capacities, and
advances the cursor.  ``sag_stack``'s node then runs on a ``CapacityPlan``: every allocation, slab plan and launch grid is sized by
three times the largest graph, the row counts of the replay live in the graph pointers on the device, and the two per-graph level
kernels zero the padding rows they leave behind (``tsgnn_sag_pool_graph_cap_f32 / _bwd_cap_f32``).

``conv="gcn"`` only (the reference's network); anything else is a TypeError that names the eager drop-in.

The second half of 2stg+ (Code/sag/train_triplet_pre_train.py:219-263: one optimiser step per graph on ``F.nll_loss(model(data),
data.y)``; the driver's ``model.map2_model`` is never read by ``Net.forward``) is ``PostTrainStream`` on the same machinery at ONE graph
per entry (``SagArenaStream`` holds what the two streams share; ``tsgnn_sag_anchor_gather_f32``; the head, its log_softmax and the
loss in one launch each way, ``post_train.apply_mlp3_nll``), ``post_train_step`` its eager drop-in and ``test_dataset`` the driver's
``test()``.

The family's "original" setting (Code/sag/train.py:181-198: ``DataLoader(batch_size=128, shuffle=True)``, ``F.nll_loss(model(data),
data.y)``, Adam) is ``MiniBatchStream``: a NEW mini-batch of 1..128 graphs per replay (``tsgnn_sag_batch_gather_f32``,
csrc/sag_batch_stream.hip), at capacities that default to the ``batch`` largest graphs level by level and are checked per entry at
``load`` (``level_sums``, ``default_level_caps``, ``schedule_capacity``, ``check_fit``)."""
import numpy as np
import torch

from . import _native as nat
from .minibatch_stream import MAX_BATCH, MiniBatchSteps, compare, top_sum
from .post_train import AnchorSteps
from .sag_triplet import _np, tail_ok
from .triplet_stream import HEAD, TICKET_WORDS, Arena, ArenaStream, TripletSteps, _align4, check_schedule, schedule_of  # noqa: F401  (the stream's vocabulary)

REC_WORDS = 8          # int32 words of a graph's record: n, nnz, first row, first entry, index, 0, 0, 0
EAGER = "; use the eager drop-in, tripletnet.forward(a, p, n)"


def pack_arena(datas, batch=3, limit=1 << 31, n_classes=None, labels=None):
    """``Data``-like objects (``.x [n, F]``, ``.edge_index [2, E]``: row 0 = source, row 1 = target) -> ``Arena``.  ValueError, naming
    the graph's index, for what the fused SAGPool node cannot take on a gathered batch: n < 1, n above
    ``tsgnn_sag_pool_graph_max_nodes()``, an edge id outside the graph, a graph that is not symmetric as a multiset (the in-kernel
    filter needs it), feature widths that differ; and for offsets that reach ``limit`` (the records are int32).  With ``n_classes``
    the arena carries ``labels`` (int32 [G]: ``label_table`` of ``data.y`` or of ``labels``).  Pure numpy: no GPU is touched.
    The arena's fields:
      records  int32 [G, 8]          n, nnz, first row, first entry, the graph's index, 0, 0, 0
      buf      int32 [words]         sections ``rowptr`` | ``col`` at the word offsets ``off[...]`` (each on 16 bytes); graph i's n + 1
                                     row pointers (graph-local) start at ``first row + i``, its columns (graph-local, rows are
                                     targets, sources ascending, repeated edges kept: ``sag_triplet.pack_host``'s order) at ``first entry``
      feats    float32 [nodes, ld]   ld = fin rounded up to 4, zero in the pad columns
      caps     (rows, nnz)           ``batch`` (3: a triplet, 1: the anchor of the post-training step) times the largest n / nnz: no
                                     entry needs more, also when one object fills every place
      largest  the largest n"""
    datas = list(datas)
    if not datas:
        raise ValueError("pack_arena: no graphs")
    max_nodes = int(nat.lib().tsgnn_sag_pool_graph_max_nodes())
    G = len(datas)
    rec = np.zeros((G, REC_WORDS), dtype=np.int64)
    rps, cols, fts = [], [], []
    fin = None
    row0 = ent0 = 0
    for i, d in enumerate(datas):
        x = _np(d.x)
        n = int(x.shape[0])
        if n < 1:
            raise ValueError("graph %d: a graph needs at least one node" % i)
        if n > max_nodes:
            raise ValueError("graph %d: %d nodes exceed the per-graph level kernels' %d" % (i, n, max_nodes))
        x = x.reshape(n, -1).astype(np.float32, copy=False)
        if fin is None:
            fin = int(x.shape[1])
        elif int(x.shape[1]) != fin:
            raise ValueError("graph %d: feature width %d differs from the other graphs' %d" % (i, x.shape[1], fin))
        ei = _np(d.edge_index).astype(np.int64).reshape(2, -1)
        if ei.size and (ei.min() < 0 or ei.max() >= n):
            raise ValueError("graph %d: edge_index holds node ids outside [0, %d)" % (i, n))
        src, dst = ei[0], ei[1]
        if not np.array_equal(np.sort(src * n + dst), np.sort(dst * n + src)):
            raise ValueError("graph %d: the edge list is not symmetric (every edge needs its reverse, as a multiset)" % i)
        order = np.lexsort((src, dst))                                      # by target, sources ascending inside a target
        rp = np.zeros(n + 1, dtype=np.int64)
        np.cumsum(np.bincount(dst, minlength=n), out=rp[1:])
        rec[i] = (n, src.size, row0, ent0, i, 0, 0, 0)
        rps.append(rp); cols.append(src[order]); fts.append(x)
        row0 += n; ent0 += int(src.size)
    off = {"rowptr": 0, "col": _align4(row0 + G)}
    words = off["col"] + _align4(max(ent0, 1))
    ld = (fin + 3) // 4 * 4
    top = lambda c: int(batch) * int(rec[:, c].max())
    if max(words, row0 * ld, top(0) + 64, top(1)) >= int(limit):
        raise ValueError("pack_arena: offsets reach %d (int32 records): %d buffer words, %d nodes" % (limit, words, row0))
    buf = np.zeros(words, dtype=np.int32)
    buf[:row0 + G] = np.concatenate(rps)
    buf[off["col"]:off["col"] + ent0] = np.concatenate(cols)
    feats = np.zeros((row0, ld), dtype=np.float32)
    feats[:, :fin] = np.concatenate(fts)
    table = label_table(datas, n_classes, labels) if n_classes is not None else None
    return Arena(records=rec.astype(np.int32), buf=buf, off=off, words=words, feats=feats, fin=fin, ld=ld, caps=(top(0), top(1)),
                 batch=int(batch), largest=int(rec[:, 0].max()), n_graphs=G, total_nodes=row0, labels=table)


def k_chain(n, ratio, depth=3):
    """[n, k(n), k(k(n)), ...]: k = min(n, ceil(float32(ratio) * float32(n))), what ``SagPlan`` computes and the gather launch repeats"""
    out = [int(n)]
    for _ in range(depth):
        n = out[-1]
        out.append(min(n, int(np.ceil(np.float32(ratio) * np.float32(n)))))
    return out


class _CapLevel:
    __slots__ = ("B", "N", "sizes", "gp", "row_graph", "max_seg")


class CapacityPlan:
    """what ``sag_stack._SagStack`` reads from a ``SagPlan`` (``depth``, ``levels[l].B / N / gp / max_seg``) with every host value a
    capacity: N = batch k^l(largest n), max_seg = k^l(largest n) (k is monotone in n, so this bounds every graph at every level;
    ``batch``: 3 graphs per entry, or 1 for the post-training stream); ``gp`` are
    the device tensors the gather launch writes (``gp_all [depth + 1, ldg]``, ldg = batch + 1 rounded up to 4: 4 for a triplet and
    for the anchor; pass ``device=None`` for the host values alone).  ``level_caps`` (``MiniBatchStream``): N of every level in place
    of batch k^l(largest n), where the caller knows that no entry needs that much.  ``capacity = True`` is what ``_SagStack`` asks for."""

    capacity = True

    def __init__(self, largest, ratio, depth=3, device=None, batch=3, level_caps=None):
        self.ratio, self.depth, self.device, self.batch = float(ratio), int(depth), device, int(batch)
        self.ldg = _align4(self.batch + 1)
        self.gp_all = torch.zeros(depth + 1, self.ldg, dtype=torch.int32, device=device) if device is not None else None
        chain = k_chain(largest, ratio, depth)
        if level_caps is not None:
            level_caps = [int(c) for c in level_caps]
            if len(level_caps) != depth + 1 or any(c < seg for c, seg in zip(level_caps, chain)):
                raise ValueError("level_caps %s: one capacity per level, none below the largest graph's %s" % (level_caps, chain))
        self.levels = []
        for l, seg in enumerate(chain):
            L = _CapLevel()
            L.B, L.N, L.max_seg, L.sizes, L.row_graph = self.batch, level_caps[l] if level_caps is not None else self.batch * seg, seg, None, None
            L.gp = self.gp_all[l] if self.gp_all is not None else None
            self.levels.append(L)


class _CapGraph:
    """what ``_SagStack`` reads from a ``GraphBatch``: the gathered CSR at its capacities, unit weights, symmetric by construction of
    the arena, the coefficients already in place (no ``gcn_coef`` launch)"""

    val = None
    symmetric = True

    def __init__(self, rowptr, col, dinv, self_w, rows):
        self.rowptr, self.col, self.total_rows, self.device = rowptr, col, int(rows), rowptr.device
        self._gcn_coef = (dinv, self_w)


class SagArenaStream(ArenaStream):
    """What the SAGPool streams share, whatever the number ``B`` of graphs a schedule entry names (3: ``TripletStream``; 1:
    ``PostTrainStream``): the model refusals (TypeError ending in the stream's eager drop-in), the arena upload, the capacity buffers
    the gather launch writes and the ``CapacityPlan`` over them, the gather launch (``GATHER``: its entry point), ``_params`` and the
    fused node on the gathered batch (``readout``)."""

    NAME = "sag_stream.SagArenaStream"
    TAKES = "takes a sag_layers.Net"
    EAGER = EAGER
    GATHER = "sag_triplet_gather_f32"
    DEPTH = 3

    def _check_model(self, model):
        """the refusals every SAGPool stream shares -> the model's device"""
        from . import sag_stack
        from .sag_layers import Net
        if type(model) is not Net:
            self._refuse(self.TAKES)
        if model.conv_kind != "gcn":
            self._refuse("takes conv=\"gcn\" only (conv=%r)" % (model.conv_kind,))
        dev = next(model.parameters()).device
        if dev.type != "cuda":
            self._refuse("runs on the GPU only")
        if not model._fused_ok():
            self._refuse("needs the fused SAGPool node (fused=True, a hidden width sag_stack supports, tanh gates, biases)")
        if not (sag_stack.PER_GRAPH_POOL and sag_stack.FUSED_NEXT_PROPAGATE and sag_stack.DEFERRED_REDUCE):
            self._refuse("needs sag_stack's per-graph level kernels with the in-kernel filter")
        return dev

    def _init_arena(self, model, datas, dev, batch, max_steps, arena=None, row_cap=None, nnz_cap=None, level_caps=None, tickets=False):
        """pack and upload the dataset (or ``arena``, packed by the caller), allocate the batch at ``batch`` times the largest graph
        (or at ``row_cap`` / ``nnz_cap`` / ``level_caps``: ``MiniBatchStream``, whose ``load`` checks every entry against them)"""
        ar = pack_arena(datas, batch=batch) if arena is None else arena
        if ar.fin != int(model.num_features):
            raise ValueError("%s: the dataset has %d features per node, the model takes %d" % (self.NAME, ar.fin, model.num_features))
        self._init_protocol(model, dev, batch, ar, max_steps, lambda: self._allocate(row_cap, nnz_cap, level_caps), tickets)

    def _allocate(self, row_cap, nnz_cap, level_caps):
        """the capacity buffers the gather launch writes and the ``CapacityPlan`` over them"""
        ar, model, dev = self.arena, self.model, self.device
        self.row_cap = ar.caps[0] if row_cap is None else int(row_cap)
        self.nnz_cap = max(ar.caps[1] if nnz_cap is None else int(nnz_cap), 1)
        self.plan = CapacityPlan(ar.largest, model.pooling_ratio, self.DEPTH, dev, batch=self.B, level_caps=level_caps)
        i32 = lambda n: torch.zeros(n, dtype=torch.int32, device=dev)
        f32 = lambda *s: torch.zeros(*s, dtype=torch.float32, device=dev)
        self.rowptr, self.col = i32(self.row_cap + 1), i32(self.nnz_cap)
        self.dinv, self.self_w = f32(self.row_cap), f32(self.row_cap)
        self._x = f32(self.row_cap, ar.ld)
        self.x = self._x[:, :ar.fin]                        # the node reads fin columns at the row stride ld
        self.g = _CapGraph(self.rowptr, self.col, self.dinv, self.self_w, self.row_cap)

    def gather(self):
        """enqueue (current stream; capturable) the launch that writes the batch of the cursor's entry and advances the cursor"""
        entries, ticket = self._loaded(self.NAME)
        ar = self.arena
        nat.call(self.GATHER, self.records, ar.n_graphs, self.buf, ar.off["rowptr"], ar.off["col"], ar.words, self.feats,
                 ar.ld, ar.caps[0], ar.caps[1], entries, self.max_steps, self._sched, ticket, self.row_cap,
                 self.nnz_cap, float(self.plan.ratio), self.plan.depth, self.rowptr, self.col, self._x, self._x.stride(0), self.dinv,
                 self.self_w, self.plan.gp_all, self.ids_out)

    def _params(self):
        m = self.model
        out = []
        for conv, pool in ((m.conv1, m.pool1), (m.conv2, m.pool2), (m.conv3, m.pool3)):
            out += [conv.weight, conv.bias, pool.score_layer.weight, pool.score_layer.bias]
        return out

    def readout(self):
        """the fused SAGPool node on the gathered batch and the capacity plan -> readout rows [B, 2 nhid]"""
        from . import sag_stack
        return sag_stack.sag_stack(self.x, self.g, self.plan, self._params())


class TripletStream(TripletSteps, SagArenaStream):
    """``net``: a ``sag_triplet.tripletnet`` over a ``sag_layers.Net`` with ``conv="gcn"``; ``datas``: the dataset's ``Data`` objects
    (host or device tensors; they are packed once).  The interface of ``triplet_stream.TripletStream``: ``load(schedule)`` (``[T, 3]``
    indices into ``datas``), ``gather``, ``embed``, ``loss(criterion, target)`` (the step for ``GraphedStep``: every call, every replay,
    consumes the next entry), ``position``, ``ids_out``, ``len``; with ``max_steps`` the stream starts on the one-entry schedule
    [0, 0, 0].  TypeError (ending in the eager drop-in) for ``conv="sage"``, a model whose levels do not run as the fused node, a head
    the tail kernel does not take, a model that is not on the GPU."""

    NAME = "sag_stream.TripletStream"
    TAKES = "takes a sag_triplet.tripletnet over a sag_layers.Net"

    def __init__(self, net, datas, max_steps=None):
        model = getattr(net, "model", None)
        dev = self._check_model(model)
        if not tail_ok(model, torch.empty(3, 2 * int(model.nhid), dtype=torch.float32, device=dev)):
            self._refuse("needs a head the triplet tail kernel takes (tsgnn_mlp3_triplet_supported)")
        self.net = net
        self._init_arena(model, datas, dev, 3, max_steps)
        self._warm_up_schedule()

    def embed(self):
        """gather + the fused SAGPool node on the capacity plan + the triplet tail -> (dist_p, dist_n, embed_a, embed_p, embed_n), as
        ``tripletnet.forward`` returns"""
        self.gather()
        return self.net._tail(self.readout())


# ----------------------------------------------------------------------------- the post-training phase of 2stg+ (eager)
def _const0(dev):
    from .post_train import _const_i32
    return _const_i32(dev, 0)


def _device_label(data, n_classes, dev, what="data"):
    """``data.y`` as a one-element int32 device tensor for the head (a label on the host is checked against [0, n_classes) first; one
    that already lives on the device is not read back: the head clamps it)"""
    from .post_train import _const_i32
    y = getattr(data, "y", None)
    if y is None:
        raise ValueError("%s carries no label (.y)" % what)
    if isinstance(y, torch.Tensor) and y.is_cuda:
        if y.numel() != 1 or y.dtype not in (torch.int64, torch.int32):
            raise ValueError("%s: .y must be one integer; got %s of %d elements" % (what, y.dtype, y.numel()))
        return y.reshape(1).to(torch.int32)
    a = _np(y)
    if a.size != 1 or not np.issubdtype(a.dtype, np.integer):
        raise ValueError("%s: .y must be one integer; got %r" % (what, y))
    v = int(a.reshape(-1)[0])
    if not 0 <= v < int(n_classes):
        raise ValueError("%s: label %d lies outside [0, %d)" % (what, v, int(n_classes)))
    return _const_i32(dev, v)


def post_train_step(model, data):
    """forward of the reference's fine-tuning step (Code/sag/train_triplet_pre_train.py:219-263: ``loss = F.nll_loss(model(data),
    data.y)`` on ONE graph, under ``model.train()``) -> (loss, out); the caller runs ``backward`` and the optimiser
    (``FlatTrainer(model, lr=1e-3, clip=0)``).  A ``sag_layers.Net`` on the GPU takes the graph's resident structure from the model's
    ``ResidentCache`` (what ``sag_triplet.tripletnet`` and ``two_stage.embed_dataset`` share), runs the three levels once and applies
    the head, its log_softmax and the loss in one launch each way (``post_train.apply_mlp3_nll``: dropout after ``lin1`` is drawn inside
    the launch); a head outside ``tsgnn_posttrain_mlp3_nll_supported`` is the same expression as torch operators.  Any other model
    gets ``model(data)`` and ``mp.nll_loss``.  A ``map2_model`` the caller installed (the reference's dead ``pred_model``) is never
    read."""
    from . import message_passing as mp
    from . import post_train as PT
    from . import sag_triplet as ST
    from .sag_layers import Net
    dev = next(model.parameters()).device
    if type(model) is Net and dev.type == "cuda" and isinstance(data.x, torch.Tensor) and data.x.is_cuda:
        labels = _device_label(data, model.num_classes, dev)
        net = ST.tripletnet(model)                          # (a view of the model and of its shared cache: nothing is copied)
        r = net.readout(net.batch_of((data,)))
        return PT.apply_mlp3_nll(model, r, _const0(dev), labels)
    out = model(data)
    return mp.nll_loss(out, data.y), out


def test_dataset(model, datas, chunk=None):
    """the reference's ``test(model, loader)`` (Code/sag/train_triplet_pre_train.py:21-31) -> (accuracy, summed nll / N) in eval mode:
    rows of ``two_stage.embed_dataset`` (= ``out`` of every graph alone), arg-max (a tie to the lowest class), nll and the label-range
    check on the device, ONE device-to-host copy.  ValueError for a label outside [0, num_classes)."""
    from . import two_stage as TS
    datas = TS._flatten(datas)
    if not datas:
        raise ValueError("test_dataset: no graphs")
    out = TS.embed_dataset(model, datas, chunk)
    dev, C = out.device, int(out.size(1))
    ys = [d.y if isinstance(d.y, torch.Tensor) else torch.as_tensor(np.asarray(d.y)) for d in datas]
    if all(y.device == dev for y in ys):
        y = torch.cat([t.reshape(-1)[:1] for t in ys]).long()
    else:
        y = torch.from_numpy(np.asarray([int(_np(t).reshape(-1)[0]) for t in ys], dtype=np.int64)).to(dev)
    pred = (out == out.max(dim=1, keepdim=True).values).int().argmax(dim=1)        # (the first maximum: the lowest index)
    nll = -out.double().gather(1, y.clamp(0, C - 1).view(-1, 1)).sum()
    res = torch.stack([(pred == y).sum().double(), nll, y.min().double(), y.max().double()]).cpu().numpy()
    if res[2] < 0 or res[3] >= C:
        raise ValueError("test_dataset: labels span [%d, %d], the model has %d classes" % (int(res[2]), int(res[3]), C))
    return float(res[0]) / len(datas), float(res[1]) / len(datas)


test_dataset.__test__ = False       # (pytest: a library function, not a test)


# ----------------------------------------------------------------------------- the post-training phase of 2stg+ (streamed)
POST_EAGER = "; use the eager drop-in, sag_stream.post_train_step(model, data)"


def label_table(datas, n_classes, labels=None):
    """int32 [G] of ``data.y`` (or of ``labels``, one integer per graph); ValueError, naming the graph's index, for a label that is
    missing, no single integer, or outside [0, n_classes).  Labels that live on the device come to the host in one copy."""
    datas = list(datas)
    if labels is None:
        ys = [getattr(d, "y", None) for d in datas]
        for i, y in enumerate(ys):
            if y is None:
                raise ValueError("graph %d carries no label (.y)" % i)
        if ys and all(isinstance(y, torch.Tensor) and y.is_cuda and y.numel() == 1 for y in ys):
            ys = list(torch.cat([y.reshape(1) for y in ys]).cpu().numpy())
    else:
        ys = list(_np(labels).reshape(-1)) if not isinstance(labels, (list, tuple)) else list(labels)
        if len(ys) != len(datas):
            raise ValueError("%d labels for %d graphs" % (len(ys), len(datas)))
    out = np.zeros(len(datas), dtype=np.int32)
    for i, y in enumerate(ys):
        a = _np(y)
        if a.size != 1 or not np.issubdtype(a.dtype, np.integer):
            raise ValueError("graph %d: the label must be one integer; got %r" % (i, y))
        v = int(a.reshape(-1)[0])
        if not 0 <= v < int(n_classes):
            raise ValueError("graph %d: label %d lies outside [0, %d)" % (i, v, int(n_classes)))
        out[i] = v
    return out


class PostTrainStream(AnchorSteps, SagArenaStream):
    """An epoch of the SAGPool fine-tuning steps (Code/sag/train_triplet_pre_train.py:219-263: ``F.nll_loss(model(data), data.y)`` on
    ONE graph per optimiser step) from ONE hipGraph: the arena of ``pack_arena(datas, batch=1)``, a device label table, and per replay
    the anchor gather launch (``tsgnn_sag_anchor_gather_f32``: the graph of "schedule entry number cursor" at capacities of one
    largest graph), ``sag_stack``'s fused node on the B = 1 capacity plan and the head with its log_softmax and the loss in one launch
    each way (``tsgnn_posttrain_mlp3_nll_*``), whose label is ``labels[ids_out[0]]`` read on the device.

    ``model``: a bare ``sag_layers.Net`` with ``conv="gcn"`` (what ``TripletStream`` takes under its ``tripletnet``); a
    ``map2_model`` the caller installed, as the reference does, is never read.  Labels: ``data.y`` or ``labels``.
    ``load(anchors)``: [T] or [T, 1] indices into ``datas``; ``step()`` -> (loss, out); ``step_loss()`` is the callable for
    ``GraphedStep`` (the reference's trainer here is a NEW ``FlatTrainer(model, lr=1e-3, clip=0)``).  In train mode with
    ``dropout_ratio`` > 0 the mask after ``lin1`` is drawn inside the head's launch from the process seed and device counter every
    mlp3 launch shares; they are created here, so a capture never has to.  TypeError ending in the eager drop-in for a model or a head
    the fused launches do not take."""

    NAME = "sag_stream.PostTrainStream"
    TAKES = "takes a bare sag_layers.Net"
    EAGER = POST_EAGER
    GATHER = "sag_anchor_gather_f32"

    def __init__(self, model, datas, labels=None, max_steps=None):
        from . import post_train as PT
        from .sag_triplet import _in_kernel_dropout
        dev = self._check_model(model)
        if not PT.mlp3_nll_ok(model, torch.empty(1, 2 * int(model.nhid), dtype=torch.float32, device=dev)):
            self._refuse("needs a head the fused launches take (tsgnn_posttrain_mlp3_nll_supported)")
        datas = list(datas)
        self.n_classes = int(model.num_classes)
        table = label_table(datas, self.n_classes, labels)
        self._init_arena(model, datas, dev, 1, max_steps)
        self.labels = torch.from_numpy(table).to(dev)
        _in_kernel_dropout(max(float(model.dropout_ratio), 0.0), dev)         # (creates the seed and the device counter)
        self._warm_up_schedule()

    def step(self):
        """gather launch + the fused node's readout row + the head -> (loss, out) of the cursor's entry"""
        from . import post_train as PT
        self.gather()
        r = self.readout()
        if not PT.mlp3_nll_ok(self.model, r):
            raise RuntimeError("%s: the fused head does not take this model's readout rows%s" % (self.NAME, self.EAGER))
        return PT.apply_mlp3_nll(self.model, r, self.ids_out, self.labels)


# ----------------------------------------------------------------------------- the mini-batch stream (the "original" setting)
BATCH_EAGER = "; use the eager route, MiniBatchStream.eager_loss(ids) / mp.nll_loss(Net(use_batch=True)(collated batch), y)"


def size_records(datas):
    """int64 [G, 2] of (n, nnz) per ``Data``-like object: what the capacity helpers below read of an arena's records, without packing
    one (``schedule_capacity`` in front of the stream's constructor)"""
    return np.asarray([[int(d.x.shape[0]), int(np.prod(d.edge_index.shape)) // 2] for d in datas], dtype=np.int64).reshape(-1, 2)


def k_levels(n, ratio, depth=3):
    """``k_chain`` vectorised: int64 [..., depth + 1] of n, k(n), k(k(n)), ... with k = min(n, ceil(float32(ratio) * float32(n)))"""
    out = [np.asarray(n, dtype=np.int64)]
    for _ in range(int(depth)):
        k = np.ceil(np.float32(ratio) * out[-1].astype(np.float32)).astype(np.int64)
        out.append(np.minimum(out[-1], k))
    return np.stack(out, axis=-1)


def level_sums(records, schedule, ratio, depth=3):
    """the rows of every level of every schedule entry: int64 [T, depth + 1] (a graph counts as often as the entry names it)"""
    rec = np.asarray(records, dtype=np.int64)
    return k_levels(rec[:, 0], ratio, depth)[np.asarray(schedule, dtype=np.int64)].sum(axis=1)


def nnz_sums(records, schedule):
    """the CSR entries of every schedule entry: int64 [T]"""
    return np.asarray(records, dtype=np.int64)[:, 1][np.asarray(schedule, dtype=np.int64)].sum(axis=1)


def default_level_caps(records, batch, ratio, depth=3):
    """rows no entry of ``batch`` DISTINCT graphs exceeds, per level: the sum of the ``batch`` largest k^l(n) (k is monotone in n, so
    these are the ``batch`` largest graphs at every level; a dataset of fewer graphs: the largest stands in for the missing ones)"""
    K = k_levels(np.asarray(records, dtype=np.int64)[:, 0], ratio, depth)
    return [top_sum(K[:, l], batch) for l in range(int(depth) + 1)]


def default_nnz_cap(records, batch):
    """CSR entries no entry of ``batch`` DISTINCT graphs exceeds (at least 1)"""
    return max(top_sum(np.asarray(records, dtype=np.int64)[:, 1], batch), 1)


def schedule_capacity(records, schedule, ratio, depth=3):
    """the schedule's own maxima -> {row_cap, nnz_cap, level_caps}, the constructor's keywords: the smallest capacities every entry
    of ``schedule`` fits (never below the dataset's largest graph).  The default capacity has to cover the ``batch`` largest graphs in
    one entry, which a shuffled epoch hardly ever draws; a loop that knows its schedules passes these instead"""
    rec = np.asarray(records, dtype=np.int64)
    s = np.asarray(schedule)
    s = check_schedule(s, len(rec), s.shape[1] if s.ndim == 2 else 1)
    floor = k_levels(rec[:, 0].max(), ratio, depth)
    caps = np.maximum(level_sums(rec, s, ratio, depth).max(axis=0), floor)
    return {"row_cap": int(caps[0]), "nnz_cap": int(max(nnz_sums(rec, s).max(), rec[:, 1].max(), 1)), "level_caps": [int(c) for c in caps]}


def _compare(schedule, records, batch, row_cap, nnz_cap, level_caps, ratio):
    """need [T, depth + 3]: the rows of every level, the rows of level 0 once more (against ``row_cap``), the CSR entries"""
    def need(s):
        lv = level_sums(records, s, ratio, len(level_caps) - 1)
        return np.concatenate([lv, lv[:, :1], nnz_sums(records, s).reshape(-1, 1)], axis=1)
    return compare(schedule, len(records), batch, need, list(level_caps) + [row_cap, nnz_cap])


def fits_mask(schedule, records, batch, row_cap, nnz_cap, level_caps, ratio):
    """bool [T]: the entry's rows at every level and its CSR entries lie within the capacities (duplicates inside an entry count as often
    as they appear).  ``check_schedule``'s ValueError for a wrong shape, a wrong dtype or an index out of range"""
    return ~_compare(schedule, records, batch, row_cap, nnz_cap, level_caps, ratio)[2]


def check_fit(schedule, records, batch, row_cap, nnz_cap, level_caps, ratio):
    """-> the checked int32 schedule; ValueError naming the first entry that exceeds a capacity, and the eager route"""
    s, need, over = _compare(schedule, records, batch, row_cap, nnz_cap, level_caps, ratio)
    if over.any():
        k = int(np.argmax(over))
        raise ValueError("schedule entry %d has %s rows (level by level) and %d CSR entries: more than this stream's capacity (row_cap %d, "
                         "nnz_cap %d, level_caps %s)%s" % (k, need[k, :-2].tolist(), need[k, -1], int(row_cap), int(nnz_cap),
                                                           [int(c) for c in level_caps], BATCH_EAGER))
    return s


class _DeviceData:
    """a ``Data`` object's tensors on the device, for the eager route of a stream that was given host tensors"""
    __slots__ = ("x", "edge_index", "__weakref__")

    def __init__(self, d, dev):
        self.x = torch.as_tensor(_np(d.x)).to(dev)
        self.edge_index = torch.as_tensor(_np(d.edge_index)).long().reshape(2, -1).to(dev)


class MiniBatchStream(MiniBatchSteps, SagArenaStream):
    """An epoch of the SAGPool family's "original" setting (Code/sag/train.py:181-198: ``DataLoader(batch_size=128, shuffle=True)``,
    ``F.nll_loss(model(data), data.y)``, Adam) from ONE hipGraph: the arena of ``pack_arena(datas, batch=B)``, a device label table, and
    per replay the batch gather launch (``tsgnn_sag_batch_gather_f32``: the B graphs of "schedule entry number cursor" as one batch at
    the stream's capacities, the graph pointer of every level, ``label`` int64 [B]), ``sag_stack``'s fused node on the capacity plan and
    the head with in-kernel dropout and the loss folded into its backward (``mp.mlp3_log_softmax`` + ``mp.nll_loss``):

        st = MiniBatchStream(model, datas, 128, max_steps=len(datas) // 128)
        gs = GraphedStep(FlatTrainer(model, lr=5e-4, weight_decay=1e-4, clip=0), st.loss())
        for epoch in ...:
            full, rest = minibatch_stream.epoch_schedule(len(datas), 128, rng)
            st.load(full)
            for _ in range(len(full)): gs.step()
            gs.synchronize()
            ... st.eager_loss(rest) ...                          # the epoch's remainder: an exact batch

    ``model``: a bare ``sag_layers.Net`` with ``conv="gcn"`` and, for ``batch`` > 1, ``use_batch=True``: the reference's ``Net`` throws
    ``data.batch`` away (Code/sag/network.py:32, trap T6) and pools a mini-batch as ONE graph, whose [1, C] output cannot meet B labels;
    the stream pools per graph.  Labels: ``data.y`` or ``labels``.  ``row_cap`` / ``nnz_cap`` / ``level_caps``: the capacities
    (default: the sums of the ``batch`` largest graphs, level by level — any entry of distinct graphs fits; ``schedule_capacity`` gives
    a schedule's own); ``load`` checks every entry against them on the host, so the launch never sees one that does not fit.
    ``load(schedule [T, batch])``, ``fits(schedule)``, ``gather``, ``step() -> (loss, logp [batch, C])``, ``loss()`` (the callable for
    ``GraphedStep``), ``eager_step(ids)`` / ``eager_loss(ids)``: the same step on the exact, unpadded batch of 1..``batch`` graphs
    through ``Net``'s own fused forward with host-known sizes, for entries that do not fit and the epoch's remainder.  ``max_steps``
    as ``TripletStream`` (the warm-up entry: ``batch`` copies of the smallest graph whose copies fit).  The dropout seed and device
    counter are created here, so a capture never has to.  TypeError / ValueError ending in the eager route for whatever the fused
    launches do not take."""

    NAME = "sag_stream.MiniBatchStream"
    TAKES = "takes a bare sag_layers.Net"
    EAGER = BATCH_EAGER
    GATHER = "sag_batch_gather_f32"

    def __init__(self, model, datas, batch, labels=None, row_cap=None, nnz_cap=None, level_caps=None, max_steps=None):
        from . import message_passing as mp
        from .sag_triplet import _in_kernel_dropout, tripletnet
        B = self._batch_in_range(batch)
        dev = self._check_model(model)
        if B > 1 and not model.use_batch:
            self._refuse("pools every graph of a mini-batch on its own, which is Net(use_batch=True): use_batch=False keeps the "
                         "reference's network.py:32, which throws data.batch away and pools the mini-batch as ONE graph, so that its "
                         "[1, C] output cannot meet %d labels" % B)
        if not mp.mlp3_ok(torch.empty(B, 2 * int(model.nhid), dtype=torch.float32, device=dev), model.lin1, model.lin2, model.lin3):
            self._refuse("needs a head the fused launches take at %d rows (tsgnn_mlp3_supported)" % B)
        datas = list(datas)
        self.n_classes = int(model.num_classes)
        try:
            ar = pack_arena(datas, batch=B, n_classes=self.n_classes, labels=labels)
        except ValueError as e:
            raise ValueError("%s: %s%s" % (self.NAME, e, self.EAGER)) from None
        ratio = float(model.pooling_ratio)
        self.max_n, self.max_nnz = int(ar.records[:, 0].max()), int(ar.records[:, 1].max())
        caps = default_level_caps(ar.records, B, ratio, self.DEPTH) if level_caps is None else [int(c) for c in level_caps]
        if row_cap is not None:
            if level_caps is not None and int(row_cap) != caps[0]:
                raise ValueError("%s: row_cap %d is not level_caps[0] = %d%s" % (self.NAME, int(row_cap), caps[0], self.EAGER))
            caps[0] = int(row_cap)
            if level_caps is None:                              # (a smaller level 0 bounds the levels behind it: k is monotone)
                caps = [min(c, caps[0]) for c in caps]
        nnz_cap = default_nnz_cap(ar.records, B) if nnz_cap is None else int(nnz_cap)
        chain = k_chain(self.max_n, ratio, self.DEPTH)
        if len(caps) != self.DEPTH + 1 or any(c < s for c, s in zip(caps, chain)) or nnz_cap < max(self.max_nnz, 1):
            raise ValueError("%s: level_caps %s / nnz_cap %d lie below the dataset's largest graph (%s rows level by level, %d CSR entries)%s"
                             % (self.NAME, caps, nnz_cap, chain, self.max_nnz, self.EAGER))
        self._init_arena(model, datas, dev, B, max_steps, arena=ar, row_cap=caps[0], nnz_cap=nnz_cap, level_caps=caps, tickets=True)
        self.level_caps = np.asarray(caps, dtype=np.int64)          # (host: the launch reads it at enqueue time)
        self._init_labels(ar.labels)                                # (label: what mp.nll_loss takes)
        self.datas, self._dev_datas, self._net = datas, {}, tripletnet(model)
        _in_kernel_dropout(max(float(model.dropout_ratio), 0.0), dev)         # (creates the seed and the device counter)
        self._warm_up_schedule()

    def _capacity_words(self):
        return "the capacities (level_caps %s, nnz_cap %d)" % (self.level_caps.tolist(), self.nnz_cap)

    def _checked(self, schedule):
        return check_fit(schedule, self.arena.records, self.B, self.row_cap, self.nnz_cap, self.level_caps, self.plan.ratio)

    def fits(self, schedule):
        return fits_mask(schedule, self.arena.records, self.B, self.row_cap, self.nnz_cap, self.level_caps, self.plan.ratio)

    def gather(self):
        """enqueue (current stream; capturable) the launch that writes the batch, the graph pointers and the labels of the cursor's
        entry and advances the cursor"""
        entries, _ = self._loaded(self.NAME)
        ar = self.arena
        nat.call(self.GATHER, self.records, ar.n_graphs, self.buf, ar.off["rowptr"], ar.off["col"], ar.words, self.feats, ar.ld,
                 self.labels, self.max_n, self.max_nnz, entries, self.max_steps, self._sched, self._tickets, self.B,
                 self.row_cap, self.nnz_cap, self.level_caps.ctypes.data, float(self.plan.ratio), self.plan.depth, self.rowptr, self.col,
                 self._x, self._x.stride(0), self.dinv, self.self_w, self.plan.gp_all, self.plan.ldg, self.ids_out, self.label)

    def _head(self, r, label):
        from . import message_passing as mp
        m = self.model
        if not mp.mlp3_ok(r, m.lin1, m.lin2, m.lin3):
            raise RuntimeError("%s: the fused head does not take this model's readout rows%s" % (self.NAME, self.EAGER))
        logp = mp.mlp3_log_softmax(r, m.lin1, m.lin2, m.lin3, m.dropout_ratio, m.training)
        return mp.nll_loss(logp, label), logp

    def _gathered(self):
        return (self.readout(),)

    # ------------------------------------------------------------------ the eager route
    def _device_data(self, i):
        d = self.datas[i]
        if isinstance(d.x, torch.Tensor) and d.x.is_cuda and isinstance(d.edge_index, torch.Tensor) and d.edge_index.is_cuda:
            return d
        if i not in self._dev_datas:
            self._dev_datas[i] = _DeviceData(d, self.device)
        return self._dev_datas[i]

    def eager_step(self, ids):
        """the same step on the exact, unpadded batch of ``ids`` (1 to ``batch`` graphs): cached structure concatenated on the device,
        ``Net``'s fused forward with host-known sizes, the same head -> (loss, logp)"""
        ids = self._checked_ids(ids)
        r = self._net.readout(self._net.batch_of([self._device_data(int(i)) for i in ids]))
        y = torch.from_numpy(self.arena.labels[ids].astype(np.int64)).to(self.device)
        return self._head(r, y)
