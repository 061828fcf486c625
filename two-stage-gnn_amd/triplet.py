"""Drop-in for Code/sage+gat+diffpool/tripletnet.py:11-45 — the 2stg / 2stg+ training step.

The reference runs the encoder three times at B = 1 (anchor, positive, negative: three uploads of a dense
[1,Nmax,Nmax] adjacency and three sequential forwards, tripletnet.py:18-38).  Here the three graphs form ONE
block-diagonal GraphBatch and go through the kernels once; ``per_graph_bn`` keeps every graph on the per-row statistics it
would have alone in its batch, so embeddings and gradients equal the three separate B = 1 calls.
"""
import os
import sys
import types

import numpy as np
import torch
import torch.nn as nn

from . import _native as nat
from . import message_passing as mp
from . import resident as R
from .graph import GraphBatch
from .resident import resident_cache                               # (the documented name of the model's cache)
from .triplet_stream import TripletStream, pack_arena, schedule_of  # a new triplet per replay of one hipGraph (triplet_stream.py)


class _Module(types.ModuleType):
    """``triplet.RESIDENT`` (TSGNN_TRIPLET_CACHE) reads and assigns ``resident.RESIDENT``, the one switch every caller reads"""
    RESIDENT = property(lambda self: R.RESIDENT, lambda self, on: setattr(R, "RESIDENT", bool(on)))


sys.modules[__name__].__class__ = _Module


# ----------------------------------------------------------------------------- the graphs of the dataset, resident (see resident.py)
class _Resident:
    """device pieces of one graph object (~100 KB for a DD graph), keyed by its ``adj`` array"""
    __slots__ = ("ref", "n", "nnz", "nmax", "rowptr", "col", "val", "feats", "assign", "symmetric")


def resident_graph(obj, dev, cache):
    """the device-side pieces of one graph object (built at its first use): CSR rows of ``adj[:n, :n]`` (no ``val`` when every weight
    is 1.0), feature rows and, when they differ from those, assignment feature rows"""
    adj = obj.graph["adj"]
    e = cache.lookup(adj, dev.index)
    if e is not None:
        return e
    a = np.asarray(adj)
    n = int(obj.graph["num_nodes"])
    if a.ndim != 2 or a.shape[0] != a.shape[1] or not 0 <= n <= a.shape[0]:
        raise ValueError("adj must be [Nmax, Nmax] with num_nodes <= Nmax")
    rp, c, v, sym = R.dense_csr_host(a, n)
    e = _Resident()
    e.n, e.nnz, e.nmax, e.symmetric = n, int(c.size), int(a.shape[0]), sym
    e.rowptr, e.col = torch.from_numpy(rp).to(dev), torch.from_numpy(c).to(dev)
    e.val = None if bool((v == 1.0).all()) else torch.from_numpy(v).to(dev)
    e.feats = R.padded_rows(obj.graph["feats"], n, dev)
    fa, ff = np.asarray(obj.graph["assign_feats"]), np.asarray(obj.graph["feats"])
    e.assign = None if (fa.shape == ff.shape and np.array_equal(fa, ff)) else R.padded_rows(fa, n, dev)
    cache.h2d += 3 + (e.val is not None) + (e.assign is not None)
    return cache.store(adj, e, dev.index)


def assemble(parts, dev):
    """resident graphs (the three of a triplet, or a chunk of a dataset) -> (GraphBatch, feature rows, assignment rows or None, sizes):
    the block-diagonal batch of packed rows + Nmax empty ghost-slot rows (GraphBatch.from_csr's layout)"""
    nmax = parts[0].nmax
    if any(p.nmax != nmax for p in parts):
        raise ValueError("the graphs of a batch must be padded to the same Nmax")
    sizes = np.array([p.n for p in parts], dtype=np.int64)
    rowptr, col, val, nnz, sym = R.concat_csr([(p.rowptr, p.col, p.val, p.n, p.nnz, p.symmetric) for p in parts], nmax + 1)
    g = GraphBatch.from_csr(rowptr, col, val, sizes, nmax, assume_symmetric=sym)
    g.nnz = nnz
    x = torch.cat([p.feats for p in parts] + [R.ghost_zeros(nmax, parts[0].feats.size(1), dev)])
    xa = None
    if any(p.assign is not None for p in parts):
        pa = [p.assign if p.assign is not None else p.feats for p in parts]
        xa = torch.cat(pa + [R.ghost_zeros(nmax, pa[0].size(1), dev)])
    return g, x, xa, sizes


# ----------------------------------------------------------------------------- embeddings + distances: one launch each way
FUSED_TAIL = os.environ.get("TSGNN_TRIPLET_TAIL", "1") != "0"


class _TripletTail(torch.autograd.Function):
    """(readouts r[3, D], map_model's weight [E, D], bias) -> (dist_p[1], dist_n[1], embed_a[1, E], embed_p, embed_n): the Linear on
    the three readout rows and both pairwise distances (tripletnet.py:35-45) as tsgnn_triplet_embed_fwd_f32 / _bwd_f32.  The five
    outputs are separate tensors, so no slice (and no zero-filled slice gradient) is launched around them."""

    @staticmethod
    def forward(ctx, r, w, b):
        w0 = w
        r, w = r.contiguous(), w.contiguous()
        D, E = int(w.size(1)), int(w.size(0))
        embed = torch.empty(3, E, dtype=torch.float32, device=r.device)
        dist = torch.empty(2, dtype=torch.float32, device=r.device)
        nat.call("triplet_embed_fwd_f32", r, r.stride(0), w, w.stride(0), b, D, E, R.EPS, embed, dist)
        ctx.save_for_backward(r, w, embed, dist)
        ctx.params = (w0, b)                              # (the Parameter objects: their slices of a trainer's flat gradient bucket)
        ctx.set_materialize_grads(False)                  # an unused output's gradient arrives as None, not as a zero-filled tensor
        outs = (dist[0:1], dist[1:2], embed[0:1], embed[1:2], embed[2:3])
        return outs

    @staticmethod
    def backward(ctx, g_dp, g_dn, g_a, g_p, g_n):
        r, w, embed, dist = ctx.saved_tensors
        D, E = int(w.size(1)), int(w.size(0))
        dev = r.device
        c = lambda t: t.contiguous() if t is not None else None
        d_r = torch.empty(3, D, dtype=torch.float32, device=dev)
        # straight into the trainer's flat gradient bucket when one is installed (FlatTrainer): no AccumulateGrad copy, no zeroing
        (dw, db), grads = mp._sinks_or_new(ctx.params, ((E, D), (E,)), dev)
        nat.call("triplet_embed_bwd_f32", r, r.stride(0), w, w.stride(0), D, E, R.EPS, embed, dist, c(g_dp), c(g_dn), c(g_a), c(g_p), c(g_n), d_r,
                 d_r.stride(0), dw, dw.stride(0), db)
        return (d_r,) + grads


class _MarginRank(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x1, x2, target, margin, mean):
        x1, x2, target = x1.contiguous().view(-1), x2.contiguous().view(-1), target.contiguous().view(-1).float()
        n = int(x1.numel())
        loss = torch.empty(1, dtype=torch.float32, device=x1.device)
        coef = torch.empty(n, dtype=torch.float32, device=x1.device)
        nat.call("margin_rank_fwd_f32", x1, x2, target, n, float(margin), int(mean), loss, coef)
        ctx.save_for_backward(coef)
        return loss.view(())

    @staticmethod
    def backward(ctx, g):
        coef, = ctx.saved_tensors
        n = int(coef.numel())
        dx1 = torch.empty(n, dtype=torch.float32, device=coef.device) if ctx.needs_input_grad[0] else None
        dx2 = torch.empty(n, dtype=torch.float32, device=coef.device) if ctx.needs_input_grad[1] else None
        nat.call("margin_rank_bwd_f32", g.contiguous().view(-1), coef, n, dx1, dx2)
        return dx1, dx2, None, None, None


class MarginRankingLoss(nn.Module):
    """torch.nn.MarginRankingLoss (train_triplet.py:235: `criterion = torch.nn.MarginRankingLoss(margin=args.alpha)`) as one launch
    forward and one backward; same constructor and call.  Inputs that are not float32 CUDA vectors of one shape, or reduction
    'none', go to torch's implementation."""

    def __init__(self, margin=0.0, size_average=None, reduce=None, reduction="mean"):
        super().__init__()
        self.margin, self.reduction = float(margin), reduction
        self._torch = nn.MarginRankingLoss(margin=margin, size_average=size_average, reduce=reduce, reduction=reduction)
        self.reduction = self._torch.reduction

    def forward(self, input1, input2, target):
        if (self.reduction in ("mean", "sum") and input1.is_cuda and input1.dtype == torch.float32 and input2.dtype == torch.float32
                and input1.shape == input2.shape == target.shape and input1.numel() > 0):
            return _MarginRank.apply(input1, input2, target, self.margin, self.reduction == "mean")
        return self._torch(input1, input2, target)


def tail_ok(model, r):
    lin = getattr(model, "map_model", None)
    return (FUSED_TAIL and isinstance(lin, nn.Linear) and r is not None and r.is_cuda and r.dim() == 2 and r.size(0) == 3
            and r.dtype == torch.float32 and lin.in_features == r.size(1) and lin.in_features % 4 == 0 and lin.out_features <= 512
            and lin.weight.dtype == torch.float32)


def _rows_models():
    """encoders whose forward takes (packed rows, GraphBatch with ghost-slot rows): the GraphSage / DiffPool family.  Others (the GAT
    encoder packs its batch itself, with one ghost representative per graph) keep the dense inputs."""
    from .dense_encoders import GcnEncoderGraph
    return (GcnEncoderGraph,)


class tripletnet(nn.Module):
    def __init__(self, model):
        super().__init__()
        self.model = model
        self._resident = R.cache_for(model)

    def _embed(self, x, g_or_adj, sizes, assign_x):
        """model forward with the per-graph batch-norm statistics of a B = 1 call -> (dist_p, dist_n, embed_a, embed_p, embed_n)"""
        m = self.model
        fuse = (FUSED_TAIL and isinstance(m, _rows_models()) and getattr(m, "final_dim", None) in ("output_dim", "pretrain")
                and isinstance(getattr(m, "map_model", None), nn.Linear))       # (encoders whose _heads honours _defer_map)
        m._defer_map = fuse
        try:
            with R.per_graph_statistics(m):
                out, embed = m(x, g_or_adj, sizes, assign_x=assign_x)
        finally:
            m._defer_map = False
        if fuse:
            r = out if m.final_dim == "output_dim" else embed      # the concatenated readouts (encoders.py:201-205)
            if tail_ok(m, r):
                return _TripletTail.apply(r, m.map_model.weight, m.map_model.bias)
            embed = m.map_model(r)
        return R.torch_distances(embed)

    @staticmethod
    def _stack(graphs, key, device):
        return torch.as_tensor(np.stack([np.asarray(g.graph[key], dtype=np.float32) for g in graphs]), device=device)

    def forward(self, a, p, n):
        """a, p, n: objects with ``.graph`` = {'adj','feats','num_nodes','assign_feats'} as cross_val.split_train_val
        prepares them (cross_val.py:158-184)."""
        dev = next(self.model.parameters()).device
        trip = (a, p, n)
        if R.RESIDENT and dev.type == "cuda" and isinstance(self.model, _rows_models()):
            g, x, xa, sizes = assemble([resident_graph(t, dev, self._resident) for t in trip], dev)
            return self._embed(x, g, sizes, x if xa is None else xa)
        adj = self._stack(trip, "adj", dev)
        h0 = self._stack(trip, "feats", dev)
        assign = self._stack(trip, "assign_feats", dev)
        sizes = np.array([int(g.graph["num_nodes"]) for g in trip])
        return self._embed(h0, adj, sizes, assign if assign.shape == h0.shape and not torch.equal(assign, h0) else h0)
