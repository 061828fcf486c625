"""Drop-in for Code/sag/tripletnet.py:9-24 — the triplet pre-training step of the SAGPool family (Code/sag/train_triplet.py:188-214).

The reference calls the model three times at B = 1 (anchor, positive, negative).  ``sag_layers.Net`` has no batch-norm, so three graphs
in ONE batch with per-graph pooling and read-outs are exactly those three calls: the triplet goes through the fused conv -> SAGPool ->
readout node once (``sag_stack`` / ``sag_stack_sage``), and the head on the three readout rows, its log_softmax and both
``F.pairwise_distance`` are one launch each way (csrc/mlp_head.hip, ``tsgnn_mlp3_triplet_fwd_f32 / _bwd_f32``).

A ``Data`` object's graph structure (CSR rows of its edge list, symmetry flag) is built at its first use and stays on the device, in
the model's ``resident.ResidentCache`` (``TSGNN_TRIPLET_CACHE=0``: rebuilt every step); a step concatenates three cached graphs on the device.  The
feature rows are NOT cached: ``data.x`` already is a device tensor (the loop's ``.to(device)``), one concatenation launch per step reads it
in place, and a copy kept here would go stale when a caller refills ``data.x``.
"""
import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _native as nat
from . import message_passing as mp
from . import resident as R
from . import triplet as _t
from .graph import GraphBatch
from .resident import ResidentCache, resident_cache       # (importable from here as before)

MarginRankingLoss = _t.MarginRankingLoss        # the documented replacement for the loop's `criterion` (train_triplet.py:196)


# ----------------------------------------------------------------------------- host half: edge lists -> CSR (pure numpy)
def _np(t):
    return t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)


def pack_host(datas):
    """Data-like objects (``.x [n, F]``, ``.edge_index [2, E]``: row 0 = source, row 1 = target) -> the block-diagonal batch of their
    graphs: (rowptr int32[N + 1], col int32[E_total], batch int64[N], sizes int64[B], symmetric (bool per graph)).  CSR rows are
    targets, the columns of a row ascend (repeated edges stay repeated), node ids are offset by the graphs before.  A graph is
    symmetric when every edge has its reverse (as a multiset)."""
    rps, cols, sizes, sym = [np.zeros(1, dtype=np.int64)], [], [], []
    n0 = e0 = 0
    for d in datas:
        n = int(d.x.shape[0])
        ei = _np(d.edge_index).astype(np.int64).reshape(2, -1)
        if n < 1:
            raise ValueError("every graph needs at least one node")
        if ei.size and (ei.min() < 0 or ei.max() >= n):
            raise IndexError("edge_index contains node ids outside [0, num_nodes)")
        src, dst = ei[0], ei[1]
        order = np.lexsort((src, dst))                                      # by target, sources ascending inside a target
        cols.append(src[order] + n0)
        rps.append(np.cumsum(np.bincount(dst, minlength=n)) + e0)
        sym.append(bool(np.array_equal(np.sort(src * n + dst), np.sort(dst * n + src))))
        sizes.append(n)
        n0 += n
        e0 += int(src.size)
    sizes = np.asarray(sizes, dtype=np.int64)
    col = np.concatenate(cols).astype(np.int32) if cols else np.zeros(0, dtype=np.int32)
    return (np.concatenate(rps).astype(np.int32), col, np.repeat(np.arange(sizes.size, dtype=np.int64), sizes), sizes, tuple(sym))


# ----------------------------------------------------------------------------- the graphs of the dataset, resident (see resident.py)
class _Graph:
    """device-side structure of one Data object"""
    __slots__ = ("ref", "n", "nnz", "rowptr", "col", "symmetric")


class _Triplet:
    """three graphs (``batch``) or a chunk of a dataset (``batch_of``) as one batch on the device: ``x [N, F]`` (refill it in place
    between hipGraph replays), the CSR batch ``g``, the host-known ``sizes``, and the pieces the composed path needs (``edge_index`` / ``batch``, built on demand)"""
    __slots__ = ("x", "g", "sizes", "datas", "_ei", "_batch")


def _check_gpu(datas):
    for d in datas:
        for t in (d.x, d.edge_index):
            if not (isinstance(t, torch.Tensor) and t.is_cuda):
                raise RuntimeError(R.GPU_ONLY)


# ----------------------------------------------------------------------------- head + log_softmax + both distances: one launch each way
class _SagTripletTail(torch.autograd.Function):
    """(readouts r[3, D0], lin1 / lin2 / lin3 weights and biases, (p, seed, state, used) or None) -> (dist_p[1], dist_n[1], embed_a[1, C],
    embed_p, embed_n).  The five outputs are separate tensors, so no slice (and no zero-filled slice gradient) is launched around them."""

    @staticmethod
    def forward(ctx, r, w1, b1, w2, b2, w3, b3, drop):
        params = (w1, b1, w2, b2, w3, b3)                 # (the Parameter objects: their slices of a trainer's flat gradient bucket)
        r, w1, w2, w3 = r.contiguous(), w1.contiguous(), w2.contiguous(), w3.contiguous()
        D0, D1, D2, C = int(w1.size(1)), int(w1.size(0)), int(w2.size(0)), int(w3.size(0))
        dev = r.device
        a1, a2 = mp._f32(3, D1, device=dev), mp._f32(3, D2, device=dev)
        embed, dist = mp._f32(3, C, device=dev), mp._f32(2, device=dev)
        p_, seed, state, used = drop if drop is not None else (0.0, 0, None, None)
        nat.call("mlp3_triplet_fwd_f32", r, r.stride(0), w1, b1, float(p_), int(seed), state, used, w2, b2, w3, b3, D0, D1, D2, C, R.EPS,
                 a1, a2, embed, dist)
        ctx.save_for_backward(r, w1, w2, w3, a1, a2, embed, dist)
        ctx.keep_scale = 1.0 / (1.0 - float(p_))
        ctx.params = params
        ctx.set_materialize_grads(False)                  # an unused output's gradient arrives as None, not as a zero-filled tensor
        return dist[0:1], dist[1:2], embed[0:1], embed[1:2], embed[2:3]

    @staticmethod
    def backward(ctx, g_dp, g_dn, g_a, g_p, g_n):
        r, w1, w2, w3, a1, a2, embed, dist = ctx.saved_tensors
        D0, D1, D2, C = int(w1.size(1)), int(w1.size(0)), int(w2.size(0)), int(w3.size(0))
        dev = r.device
        c = lambda t: t.contiguous() if t is not None else None
        # straight into the trainer's flat gradient bucket when one is installed (FlatTrainer): no AccumulateGrad copy, no zeroing
        (dw1, db1, dw2, db2, dw3, db3), grads = mp._sinks_or_new(ctx.params, ((D1, D0), (D1,), (D2, D1), (D2,), (C, D2), (C,)), dev)
        dx = mp._f32(3, D0, device=dev) if ctx.needs_input_grad[0] else None
        nat.call("mlp3_triplet_bwd_f32", r, r.stride(0), w1, w2, w3, a1, a2, embed, dist, R.EPS, ctx.keep_scale, c(g_dp), c(g_dn), c(g_a),
                 c(g_p), c(g_n), D0, D1, D2, C, dw1, db1, dw2, db2, dw3, db3, dx, D0)
        return (dx,) + grads + (None,)


def tail_ok(model, r):
    """the fused tail takes this head on these readout rows (``TSGNN_TRIPLET_TAIL=0``: never)"""
    lins = [getattr(model, k, None) for k in ("lin1", "lin2", "lin3")]
    if not (_t.FUSED_TAIL and all(isinstance(l, nn.Linear) for l in lins) and r is not None and r.is_cuda and r.dim() == 2
            and r.size(0) == 3 and r.dtype == torch.float32 and r.size(1) == lins[0].in_features):
        return False
    if any(l.weight.dtype != torch.float32 or l.weight.data_ptr() % 16 or not l.weight.is_contiguous() for l in lins):
        return False
    return bool(nat.lib().tsgnn_mlp3_triplet_supported(int(lins[0].in_features), int(lins[0].out_features), int(lins[1].out_features),
                                                       int(lins[2].out_features)))


def _in_kernel_dropout(p, dev):
    """(p, seed, state, used) of the in-kernel mask — the Philox seed / device counter that ``mp.mlp3_log_softmax`` uses, so
    ``torch.manual_seed`` governs it, a hipGraph replay draws a new mask and ``mp.mlp3_dropout_mask(p, seed, used, 3, D1)`` regenerates
    it —, or None when the counter would have to be created inside a stream capture"""
    st = mp._mlp3_drop.get(dev)
    if st is None:
        if torch.cuda.is_current_stream_capturing():
            return None
        seed = int(torch.empty((), dtype=torch.int64).random_().item())
        st = mp._mlp3_drop[dev] = (seed, torch.zeros(2, dtype=torch.int64, device=dev))
    used = torch.empty(1, dtype=torch.int64, device=dev)
    mp.last_mlp3_dropout = (float(p), st[0], used)
    return float(p), st[0], st[1], used


class tripletnet(nn.Module):
    """``tripletnet(model).forward(a, p, n) -> (dist_p, dist_n, embed_a, embed_p, embed_n)`` for ``model`` = ``sag_layers.Net`` (either
    ``conv``); per-graph pooling and read-outs whatever ``model.use_batch`` says (the reference calls the model on one graph at a
    time here).  ``batch(a, p, n)`` / ``embed(batch)`` split the call for a step replayed from a hipGraph on a resident triplet."""

    def __init__(self, model):
        super().__init__()
        self.model = model
        self.cache = R.cache_for(model)
        self._batch_vec = {}

    # ------------------------------------------------------------------ graphs
    def _graph(self, d, dev):
        """the device-side structure of one Data object (built at its first use)"""
        e = self.cache.lookup(d, dev.index) if R.RESIDENT else None
        if e is not None:
            return e
        rowptr, col, _, sizes, sym = pack_host([d])
        e = _Graph()
        e.n, e.nnz, e.symmetric = int(sizes[0]), int(col.size), sym[0]
        e.rowptr = torch.from_numpy(rowptr).to(dev)
        e.col = torch.from_numpy(col).to(dev) if col.size else torch.zeros(0, dtype=torch.int32, device=dev)
        self.cache.h2d += 2
        return self.cache.store(d, e, dev.index) if R.RESIDENT else e

    def batch(self, a, p, n):
        """the three graphs as one block-diagonal batch: cached structure concatenated on the device (no host synchronisation, no
        upload once the three objects have been seen), the feature rows read from ``data.x``"""
        return self.batch_of((a, p, n))

    def batch_of(self, datas):
        """any number of graphs as one block-diagonal batch (``two_stage.embed_dataset``: a chunk of a dataset)"""
        trip = tuple(datas)
        _check_gpu(trip)
        dev = trip[0].x.device
        parts = [self._graph(d, dev) for d in trip]
        g = GraphBatch()                                                         # (filled by hand: no bookkeeping upload, no row_maps launch)
        g.sizes = np.array([q.n for q in parts], dtype=np.int64)
        g.rowptr, g.col, g.val, g.nnz, g.symmetric = R.concat_csr([(q.rowptr, q.col, None, q.n, q.nnz, q.symmetric) for q in parts], 1)
        g.B, g.nmax, g.n_rows, g.n_ghost, g.layout, g.device = len(parts), int(g.sizes.max()), int(g.sizes.sum()), 0, "packed", dev
        b = _Triplet()
        x = torch.cat([d.x if d.x.dim() == 2 else d.x.view(d.x.size(0), -1) for d in trip])
        b.x = x if x.dtype == torch.float32 else x.float()
        b.g, b.sizes, b.datas, b._ei, b._batch = g, g.sizes, trip, None, None
        return b

    def _composed_inputs(self, b):
        """edge_index [2, E] and batch [N] of the batch for the level-by-level operators (device-side concatenation)"""
        if b._ei is None:
            off, eis = 0, []
            for d in b.datas:
                eis.append(d.edge_index + off if off else d.edge_index)
                off += int(d.x.size(0))
            b._ei = torch.cat(eis, dim=1)
            key = (b.sizes.tobytes(), b.x.device.index)
            bv = self._batch_vec.get(key)
            if bv is None:
                if len(self._batch_vec) > 64:
                    self._batch_vec.clear()
                bv = self._batch_vec[key] = torch.from_numpy(np.repeat(np.arange(len(b.sizes), dtype=np.int64), b.sizes)).to(b.x.device)
                bv._tsgnn_sizes = (bv._version, b.sizes)
                self.cache.h2d += 1
            b._batch = bv
        return b._ei, b._batch

    # ------------------------------------------------------------------ forward
    def readout(self, b):
        """[3, 2 nhid]: the three levels' [gmp || gap] summed (network.py:33-46), per graph"""
        from . import pyg
        m = self.model
        if m._fused_ok():
            r = m._forward_fused(_FusedInput(b.x, b.g), sizes=b.sizes)
            if r is not None:
                return r
        x = b.x
        edge_index, batch = self._composed_inputs(b)
        outs = []
        for conv, pool in ((m.conv1, m.pool1), (m.conv2, m.pool2), (m.conv3, m.pool3)):
            x = pyg.relu(conv(x, edge_index))
            x, edge_index, _, batch, _ = pool(x, edge_index, None, batch)
            outs.append(torch.cat([pyg.global_max_pool(x, batch), pyg.global_mean_pool(x, batch)], dim=1))
        return outs[0] + outs[1] + outs[2]

    _readout = readout

    def _torch_tail(self, r):
        from . import pyg
        m = self.model
        x = pyg.relu(mp.linear_oi(r, m.lin1.weight, m.lin1.bias))
        x = F.dropout(x, p=m.dropout_ratio, training=m.training)
        x = pyg.relu(mp.linear_oi(x, m.lin2.weight, m.lin2.bias))
        e = F.log_softmax(mp.linear_oi(x, m.lin3.weight, m.lin3.bias), dim=-1)
        return R.torch_distances(e)

    def _tail(self, r):
        """readout rows [3, 2 nhid] -> (dist_p, dist_n, embed_a, embed_p, embed_n): one launch, or the torch composition for a head
        the kernel does not take"""
        m = self.model
        if tail_ok(m, r):
            drop = None
            if m.training and m.dropout_ratio > 0.0:
                drop = _in_kernel_dropout(m.dropout_ratio, r.device)
                if drop is None:
                    return self._torch_tail(r)
            return _SagTripletTail.apply(r, m.lin1.weight, m.lin1.bias, m.lin2.weight, m.lin2.bias, m.lin3.weight, m.lin3.bias, drop)
        return self._torch_tail(r)

    def embed(self, b):
        return self._tail(self.readout(b))

    def forward(self, a, p, n):
        """a, p, n: PyG-``Data``-like objects with ``.x [n, F]`` and ``.edge_index [2, E]`` on the GPU (anything else on them is
        ignored, as network.py:32 ignores it)"""
        return self.embed(self.batch(a, p, n))


class _FusedInput:
    """what ``Net._forward_fused`` reads from its argument"""
    __slots__ = ("x", "edge_index")

    def __init__(self, x, g):
        self.x, self.edge_index = x, g
