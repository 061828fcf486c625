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

``conv="gcn"`` only (the reference's network); anything else is a TypeError that names the eager drop-in."""
import numpy as np
import torch

from . import _native as nat
from .sag_triplet import _np, tail_ok
from .triplet_stream import HEAD, ArenaStream, _align4, check_schedule, schedule_of  # noqa: F401  (the stream's vocabulary)

REC_WORDS = 8          # int32 words of a graph's record: n, nnz, first row, first entry, index, 0, 0, 0
EAGER = "; use the eager drop-in, tripletnet.forward(a, p, n)"


class Arena:
    """host arrays of a packed dataset (``pack_arena``):
      records  int32 [G, 8]          n, nnz, first row, first entry, the graph's index, 0, 0, 0
      buf      int32 [words]         sections ``rowptr`` | ``col`` at the word offsets ``off[...]`` (each on 16 bytes); graph i's n + 1
                                     row pointers (graph-local) start at ``first row + i``, its columns (graph-local, rows are
                                     targets, sources ascending, repeated edges kept: ``sag_triplet.pack_host``'s order) at ``first entry``
      feats    float32 [nodes, ld]   ld = fin rounded up to 4, zero in the pad columns
      caps     (rows, nnz)           three times the largest n / nnz: no triplet needs more, also when one object fills all three places
      largest  the largest n"""

    def __init__(self, **kw):
        self.__dict__.update(kw)


def pack_arena(datas, limit=1 << 31):
    """``Data``-like objects (``.x [n, F]``, ``.edge_index [2, E]``: row 0 = source, row 1 = target) -> ``Arena``.  ValueError, naming
    the graph's index, for what the fused SAGPool node cannot take on a gathered batch: n < 1, n above
    ``tsgnn_sag_pool_graph_max_nodes()``, an edge id outside the graph, a graph that is not symmetric as a multiset (the in-kernel
    filter needs it), feature widths that differ; and for offsets that reach ``limit`` (the records are int32).  Pure numpy: no GPU is touched."""
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
    top = lambda c: 3 * int(rec[:, c].max())
    if max(words, row0 * ld, top(0) + 64, top(1)) >= int(limit):
        raise ValueError("pack_arena: offsets reach %d (int32 records): %d buffer words, %d nodes" % (limit, words, row0))
    buf = np.zeros(words, dtype=np.int32)
    buf[:row0 + G] = np.concatenate(rps)
    buf[off["col"]:off["col"] + ent0] = np.concatenate(cols)
    feats = np.zeros((row0, ld), dtype=np.float32)
    feats[:, :fin] = np.concatenate(fts)
    return Arena(records=rec.astype(np.int32), buf=buf, off=off, words=words, feats=feats, fin=fin, ld=ld, caps=(top(0), top(1)),
                 largest=int(rec[:, 0].max()), n_graphs=G, total_nodes=row0)


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
    capacity: N = 3 k^l(largest n), max_seg = k^l(largest n) (k is monotone in n, so this bounds every graph at every level); ``gp`` are
    the device tensors the gather launch writes (``gp_all [depth + 1, 4]``; pass ``device=None`` for the host values alone).
    ``capacity = True`` is what ``_SagStack`` asks for."""

    capacity = True

    def __init__(self, largest, ratio, depth=3, device=None):
        self.ratio, self.depth, self.device = float(ratio), int(depth), device
        self.gp_all = torch.zeros(depth + 1, 4, dtype=torch.int32, device=device) if device is not None else None
        self.levels = []
        for l, seg in enumerate(k_chain(largest, ratio, depth)):
            L = _CapLevel()
            L.B, L.N, L.max_seg, L.sizes, L.row_graph = 3, 3 * seg, seg, None, None
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


class TripletStream(ArenaStream):
    """``net``: a ``sag_triplet.tripletnet`` over a ``sag_layers.Net`` with ``conv="gcn"``; ``datas``: the dataset's ``Data`` objects
    (host or device tensors; they are packed once).  The interface of ``triplet_stream.TripletStream``: ``load(schedule)`` (``[T, 3]``
    indices into ``datas``), ``gather``, ``embed``, ``loss(criterion, target)`` (the step for ``GraphedStep``: every call, every replay,
    consumes the next entry), ``position``, ``ids_out``, ``len``; with ``max_steps`` the stream starts on the one-entry schedule
    [0, 0, 0].  TypeError (ending in the eager drop-in) for ``conv="sage"``, a model whose levels do not run as the fused node, a head
    the tail kernel does not take, a model that is not on the GPU."""

    NAME = "sag_stream.TripletStream"
    DEPTH = 3

    def __init__(self, net, datas, max_steps=None):
        from . import sag_stack
        from .sag_layers import Net
        model = getattr(net, "model", None)

        def refuse(what):
            raise TypeError("%s %s%s" % (self.NAME, what, EAGER))
        if type(model) is not Net:
            refuse("takes a sag_triplet.tripletnet over a sag_layers.Net")
        if model.conv_kind != "gcn":
            refuse("takes conv=\"gcn\" only (conv=%r)" % (model.conv_kind,))
        dev = next(model.parameters()).device
        if dev.type != "cuda":
            refuse("runs on the GPU only")
        if not model._fused_ok():
            refuse("needs the fused SAGPool node (fused=True, a hidden width sag_stack supports, tanh gates, biases)")
        if not (sag_stack.PER_GRAPH_POOL and sag_stack.FUSED_NEXT_PROPAGATE and sag_stack.DEFERRED_REDUCE):
            refuse("needs sag_stack's per-graph level kernels with the in-kernel filter")
        if not tail_ok(model, torch.empty(3, 2 * int(model.nhid), dtype=torch.float32, device=dev)):
            refuse("needs a head the triplet tail kernel takes (tsgnn_mlp3_triplet_supported)")
        ar = self.arena = pack_arena(datas)
        if ar.fin != int(model.num_features):
            raise ValueError("%s: the dataset has %d features per node, the model takes %d" % (self.NAME, ar.fin, model.num_features))
        self.net, self.model, self.device, self.B = net, model, dev, 3
        self.row_cap, self.nnz_cap = ar.caps[0], max(ar.caps[1], 1)
        self.plan = CapacityPlan(ar.largest, model.pooling_ratio, self.DEPTH, dev)
        i32 = lambda n: torch.zeros(n, dtype=torch.int32, device=dev)
        f32 = lambda *s: torch.zeros(*s, dtype=torch.float32, device=dev)
        self.rowptr, self.col = i32(self.row_cap + 1), i32(self.nnz_cap)
        self.dinv, self.self_w = f32(self.row_cap), f32(self.row_cap)
        self._x = f32(self.row_cap, ar.ld)
        self.x = self._x[:, :ar.fin]                        # the node reads fin columns at the row stride ld
        self.g = _CapGraph(self.rowptr, self.col, self.dinv, self.self_w, self.row_cap)
        self.records = torch.from_numpy(ar.records).to(dev)
        self.buf = torch.from_numpy(ar.buf).to(dev)
        self.feats = torch.from_numpy(ar.feats).to(dev)
        self.ids_out = torch.zeros(3, dtype=torch.int32, device=dev)
        self.max_steps = int(max_steps) if max_steps is not None else None
        self._sched = self._host = None
        self.T = 0
        self._warm_up_schedule()

    def gather(self):
        """enqueue (current stream; capturable) the launch that writes the batch of the cursor's entry and advances the cursor"""
        if self._sched is None:
            raise RuntimeError("%s: load(schedule) before the first step" % self.NAME)
        ar = self.arena
        nat.call("sag_triplet_gather_f32", self.records, ar.n_graphs, self.buf, ar.off["rowptr"], ar.off["col"], ar.words, self.feats,
                 ar.ld, ar.caps[0], ar.caps[1], self._sched[HEAD:], self.max_steps, self._sched, self._sched[4:HEAD], self.row_cap,
                 self.nnz_cap, float(self.plan.ratio), self.plan.depth, self.rowptr, self.col, self._x, self._x.stride(0), self.dinv,
                 self.self_w, self.plan.gp_all, self.ids_out)

    def _params(self):
        m = self.model
        out = []
        for conv, pool in ((m.conv1, m.pool1), (m.conv2, m.pool2), (m.conv3, m.pool3)):
            out += [conv.weight, conv.bias, pool.score_layer.weight, pool.score_layer.bias]
        return out

    def embed(self):
        """gather + the fused SAGPool node on the capacity plan + the triplet tail -> (dist_p, dist_n, embed_a, embed_p, embed_n), as
        ``tripletnet.forward`` returns"""
        from . import sag_stack
        self.gather()
        return self.net._tail(sag_stack.sag_stack(self.x, self.g, self.plan, self._params()))

    def loss(self, criterion, target):
        """-> callable for ``GraphedStep``: gather launch + the node + the tail + ``criterion(dist_p, dist_n, target)``"""
        def step():
            out = self.embed()
            return criterion(out[0], out[1], target)
        return step
