"""Drop-in for Code/eigengcn/tripletnet.py:11-155 — the triplet pre-training step of the EigenGCN family (train_triplet.py:289-317).

The reference calls ``WavePoolingGcnEncoder`` three times at B = 1 (anchor, positive, negative), each time from 1 + L + L J + Jf dense
``[1, Nmax, Nmax]`` tensors built from the graph object's ``.graph`` dict.  Here

* a graph object's dict is packed ONCE on the host (``pack_host``: CSR of the adjacency and of every pooled adjacency, the rows'
  clusters / coefficients / bucket lists, the final coefficients — the compact pieces ``eigen_pool.collate`` builds) and goes to the
  device at the object's first use, together with its feature rows (16-byte row stride).  No ``[Nmax, Nmax]`` array is uploaded.
  ``feats`` are host numpy arrays that cross_val.py builds once and the reference never writes, so they are cached with the structure
  (as ``triplet.resident_graph`` caches them; ``Code/sag`` keeps device tensors instead, which ``sag_triplet`` reads in place).  The
  cache is the model's ``resident.ResidentCache``, keyed by the object's identity; ``TSGNN_TRIPLET_CACHE=0`` rebuilds every step;
* a step concatenates three cached graphs into one three-graph ``EigenBatch`` on the device (``eigen_pool.concat_batches``) and runs the
  model ONCE with per-graph statistics (``per_graph_bn``: the fresh ``BatchNorm1d(Nmax)`` at B = 1 is a per-row layer norm) — level 0
  as the fused stack node, pooled levels layer by layer;
* ``pred_model`` on the three readout rows and both ``F.pairwise_distance`` are one launch each way (csrc/mlp2_triplet.hip for
  Linear-ReLU-Linear, csrc/triplet.hip for a single Linear); any other head runs through torch.

``batch(a, p, n)`` / ``embed(batch)`` split the call for a step replayed from a hipGraph on a resident triplet (refill ``batch.x`` in place).
"""
import numpy as np
import torch
import torch.nn as nn

from . import _native as nat
from . import eigen_pool as ep
from . import message_passing as mp
from . import resident as R
from . import triplet as _t
from .graph import GraphBatch

MarginRankingLoss = _t.MarginRankingLoss        # the documented replacement for the loop's `criterion` (train_triplet.py:292)


# ----------------------------------------------------------------------------- host half: a .graph dict -> compact pieces (pure numpy)
def _square(d, key, nmax):
    if key not in d:
        raise ValueError("the graph dict has no '%s'" % key)
    a = np.asarray(d[key])
    if a.ndim != 2 or a.shape[0] != a.shape[1] or (nmax is not None and a.shape[0] != nmax):
        raise ValueError("%s has shape %s, expected [Nmax, Nmax]%s" % (key, a.shape, "" if nmax is None else " with Nmax = %d" % nmax))
    return a


def pack_host(graph, L, J, Jf):
    """One ``.graph`` dict (cross_val.py: 'adj', 'feats', 'num_nodes', 'adj_pool_{i+1}', 'num_nodes_{i+1}', 'pool_adj_{i}_{j}') -> the
    compact form of its L pooling levels, J matrices per level and Jf final matrices:

    ``n`` [L + 1] node counts, ``nmax``, ``graphs`` [L + 1] (rowptr int32[n_i + 1], col int32, val float32, symmetric) of
    ``adj[:n, :n]`` and ``adj_pool_{i+1}[:k, :k]``, ``levels`` [L] dicts with ``cluster_of`` int32[n_i] (the first column with a
    non-zero entry in any of the J matrices — the rule of tsgnn_eigen_pool_from_dense_f32 —, -1 for a row whose J entries are all
    zero), ``coef`` float32[n_i, J], and the local bucket list ``bptr`` int32[k + 2] / ``members`` int32[n_i] (bucket 0 = the
    unassigned rows, bucket c + 1 = cluster c; rows ascending inside a bucket), ``final`` float32[n_L, Jf] (column 0 of
    ``pool_adj_{L}_{j}``) or None.

    ValueError for: a matrix that is not [Nmax, Nmax]; an entry in a column >= the pooled node count; a row with entries in two
    different columns; a non-zero in a row >= n_i."""
    nmax = _square(graph, "adj", None).shape[0]
    n0 = int(graph["num_nodes"])
    if not 1 <= n0 <= nmax:
        raise ValueError("num_nodes must lie in [1, Nmax]")
    sizes, graphs, levels = [n0], [R.dense_csr_host(_square(graph, "adj", nmax), n0)], []
    for i in range(L):
        n = sizes[-1]
        k = int(graph["num_nodes_%d" % (i + 1)])
        if not 1 <= k <= nmax:
            raise ValueError("num_nodes_%d must lie in [1, Nmax]" % (i + 1))
        P = np.stack([np.asarray(_square(graph, "pool_adj_%d_%d" % (i, j), nmax), dtype=np.float32) for j in range(J)])    # [J, N, N]
        nz = (P != 0).any(axis=0)
        if nz[n:].any():
            raise ValueError("pool_adj_%d_*: a non-zero entry in a row >= the level's node count %d" % (i, n))
        if nz[:, k:].any():
            raise ValueError("pool_adj_%d_*: an entry in a column >= the pooled node count %d" % (i, k))
        cnt = nz[:n].sum(axis=1)
        if (cnt > 1).any():
            raise ValueError("pool_adj_%d_*: row %d has entries in two different columns" % (i, int(np.nonzero(cnt > 1)[0][0])))
        clus = np.where(cnt > 0, nz[:n].argmax(axis=1), -1).astype(np.int32)
        coef = np.where(clus[None, :] >= 0, P[:, np.arange(n), np.maximum(clus, 0)], 0.0).T.astype(np.float32)
        key = clus.astype(np.int64) + 1
        members = np.argsort(key, kind="stable").astype(np.int32)
        bptr = np.zeros(k + 2, dtype=np.int32)
        np.cumsum(np.bincount(key, minlength=k + 1), out=bptr[1:])
        levels.append({"cluster_of": clus, "coef": np.ascontiguousarray(coef), "bptr": bptr, "members": members})
        graphs.append(R.dense_csr_host(_square(graph, "adj_pool_%d" % (i + 1), nmax), k))
        sizes.append(k)
    final = None
    if Jf:
        nL = sizes[-1]
        P = np.stack([np.asarray(_square(graph, "pool_adj_%d_%d" % (L, j), nmax), dtype=np.float32) for j in range(Jf)])
        nz = (P != 0).any(axis=0)
        if nz[nL:].any():
            raise ValueError("pool_adj_%d_*: a non-zero entry in a row >= the level's node count %d" % (L, nL))
        if nz[:, 1:].any():
            raise ValueError("pool_adj_%d_*: an entry in a column >= the pooled node count 1" % L)
        final = np.ascontiguousarray(P[:, :nL, 0].T)
    return {"n": sizes, "nmax": nmax, "graphs": graphs, "levels": levels, "final": final}


# ----------------------------------------------------------------------------- the graphs of the dataset, resident
class _Graph:
    """device side of one graph object: a one-graph EigenBatch and its feature rows [n, ld]"""
    __slots__ = ("ref", "eb", "feats", "n", "nmax")


class _Triplet:
    """three graphs as one batch on the device: the ``EigenBatch`` ``eb`` and the feature rows ``x`` [rows + Nmax, ld] (refill it in
    place between hipGraph replays; the Nmax ghost-slot rows stay zero)"""
    __slots__ = ("eb", "x", "sizes")


def _up(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _device_graph(csr, n, nmax, dev):
    rp, col, val, sym = csr
    rowptr = np.concatenate([rp, np.full(nmax, rp[-1], dtype=np.int32)])
    g = GraphBatch.from_csr(_up(rowptr, dev), _up(col if col.size else np.zeros(1, np.int32), dev),
                            _up(val if val.size else np.zeros(1, np.float32), dev), np.array([n], dtype=np.int64), nmax,
                            assume_symmetric=sym)
    g.nnz = int(col.size)
    return g


def to_device(packed, feats, dev):
    """pack_host's result + the feature rows -> (one-graph EigenBatch, feats [n, ld] with a 16-byte row stride, host-to-device copies)"""
    nmax, sizes = packed["nmax"], packed["n"]
    gs = [_device_graph(c, n, nmax, dev) for c, n in zip(packed["graphs"], sizes)]
    copies = 3 * len(gs)
    levels = []
    for i, h in enumerate(packed["levels"]):
        lv = ep.EigenLevel()
        lv.g, lv.J = gs[i + 1], int(h["coef"].shape[1])
        lv.cluster_of, lv.coef, lv.bptr, lv.members = (_up(h[k], dev) for k in ("cluster_of", "coef", "bptr", "members"))
        levels.append(lv)
        copies += 4
    fc = None
    if packed["final"] is not None:
        fc = _up(packed["final"], dev)
        copies += 1
    return ep.EigenBatch(gs[0], levels, fc, nmax), R.padded_rows(feats, sizes[0], dev), copies + 1


# ----------------------------------------------------------------------------- pred_model + both distances: one launch each way
class _Mlp2TripletTail(torch.autograd.Function):
    """(readouts r[3, D], Linear-ReLU-Linear weights and biases) -> (dist_p[1], dist_n[1], embed_a[1, E], embed_p, embed_n).  The five
    outputs are separate tensors, so no slice (and no zero-filled slice gradient) is launched around them."""

    @staticmethod
    def forward(ctx, r, w1, b1, w2, b2):
        params = (w1, b1, w2, b2)                         # (the Parameter objects: their slices of a trainer's flat gradient bucket)
        r, w1, w2 = r.contiguous(), w1.contiguous(), w2.contiguous()
        D, H, E = int(w1.size(1)), int(w1.size(0)), int(w2.size(0))
        dev = r.device
        h, embed, dist = mp._f32(3, H, device=dev), mp._f32(3, E, device=dev), mp._f32(2, device=dev)
        nat.call("mlp2_triplet_fwd_f32", r, r.stride(0), w1, b1, w2, b2, D, H, E, R.EPS, h, embed, dist)
        ctx.save_for_backward(r, w1, w2, h, embed, dist)
        ctx.params = params
        ctx.set_materialize_grads(False)                  # an unused output's gradient arrives as None, not as a zero-filled tensor
        return dist[0:1], dist[1:2], embed[0:1], embed[1:2], embed[2:3]

    @staticmethod
    def backward(ctx, g_dp, g_dn, g_a, g_p, g_n):
        r, w1, w2, h, embed, dist = ctx.saved_tensors
        D, H, E = int(w1.size(1)), int(w1.size(0)), int(w2.size(0))
        dev = r.device
        c = lambda t: t.contiguous() if t is not None else None
        # straight into the trainer's flat gradient bucket when one is installed (FlatTrainer): no AccumulateGrad copy, no zeroing
        (dw1, db1, dw2, db2), grads = mp._sinks_or_new(ctx.params, ((H, D), (H,), (E, H), (E,)), dev)
        dr = mp._f32(3, D, device=dev) if ctx.needs_input_grad[0] else None
        nat.call("mlp2_triplet_bwd_f32", r, r.stride(0), w1, w2, h, embed, dist, R.EPS, c(g_dp), c(g_dn), c(g_a), c(g_p), c(g_n), D, H, E,
                 dr, D, dw1, db1, dw2, db2)
        return (dr,) + grads


def _linears(pred):
    """the nn.Linear layers of a pred_model built by build_pred_layers (Linear, or Linear (ReLU Linear)*), or None"""
    if isinstance(pred, nn.Linear):
        return [pred]
    if isinstance(pred, nn.Sequential) and len(pred) % 2 == 1 and all(
            isinstance(m, nn.Linear if i % 2 == 0 else nn.ReLU) for i, m in enumerate(pred)):
        return [m for m in pred if isinstance(m, nn.Linear)]
    return None


def _lin_ok(lin):
    w = lin.weight
    return w.dtype == torch.float32 and w.is_cuda and w.is_contiguous() and w.data_ptr() % 16 == 0 and \
        (lin.bias is None or lin.bias.dtype == torch.float32)


def tail_kind(model, r):
    """'mlp2' (csrc/mlp2_triplet.hip), 'linear' (csrc/triplet.hip) or None (torch) for this pred_model on these readout rows
    (``TSGNN_TRIPLET_TAIL=0``: never a fused tail)"""
    lins = _linears(getattr(model, "pred_model", None))
    if not (_t.FUSED_TAIL and lins and r is not None and r.is_cuda and r.dim() == 2 and r.size(0) == 3 and r.dtype == torch.float32
            and r.size(1) == lins[0].in_features and r.is_contiguous() and r.data_ptr() % 16 == 0 and all(_lin_ok(l) for l in lins)):
        return None
    if len(lins) == 2 and nat.lib().tsgnn_mlp2_triplet_supported(int(lins[0].in_features), int(lins[0].out_features),
                                                                  int(lins[1].out_features)):
        return "mlp2"
    if len(lins) == 1 and lins[0].in_features % 4 == 0 and lins[0].out_features <= 512:      # (triplet.tail_ok's limits)
        return "linear"
    return None


class tripletnet(nn.Module):
    """``tripletnet(model, args).forward(a, p, n) -> (dist_p, dist_n, embed_a, embed_p, embed_n)`` for ``model`` =
    ``eigen_encoders.WavePoolingGcnEncoder``; ``args`` supplies ``pool_sizes`` ('10', '3_2'), ``num_pool_matrix`` and
    ``num_pool_final_matrix``, which must agree with the model's."""

    def __init__(self, model, args):
        super().__init__()
        self.model = model
        self.args = args
        pool_sizes = [int(i) for i in str(args.pool_sizes).split("_")]
        if pool_sizes != [int(s) for s in model.pool_sizes]:
            raise ValueError("args.pool_sizes = %r, the model was built with %r" % (args.pool_sizes, list(model.pool_sizes)))
        if int(args.num_pool_matrix) != int(model.num_pool_matrix):
            raise ValueError("args.num_pool_matrix = %d, the model's is %d" % (args.num_pool_matrix, model.num_pool_matrix))
        if int(args.num_pool_final_matrix) != int(model.num_pool_final_matrix):
            raise ValueError("args.num_pool_final_matrix = %d, the model's is %d"
                             % (args.num_pool_final_matrix, model.num_pool_final_matrix))
        self.L, self.J, self.Jf = len(pool_sizes), int(args.num_pool_matrix), int(args.num_pool_final_matrix)
        self.cache = R.cache_for(model)                      # (the entries depend on (L, J, Jf) only, which equal the model's)

    # ------------------------------------------------------------------ graphs
    def _graph(self, obj, dev):
        """the device side of one graph object (built at its first use)"""
        e = self.cache.lookup(obj, dev.index) if R.RESIDENT else None
        if e is not None:
            return e
        e = _Graph()
        packed = pack_host(obj.graph, self.L, self.J, self.Jf)
        e.eb, e.feats, copies = to_device(packed, obj.graph["feats"], dev)
        e.n, e.nmax = packed["n"][0], packed["nmax"]
        self.cache.h2d += copies
        return self.cache.store(obj, e, dev.index) if R.RESIDENT else e

    def batch(self, a, p, n):
        """the triplet as one three-graph batch on the device: the cached pieces concatenated there (no host synchronisation, no
        upload of the graphs' structure or features once the three objects have been seen).  What a step still sends is the row
        bookkeeping of the new batch: every one of its L + 1 ``GraphBatch``es uploads ``graph_ptr`` and ``slot_count`` (a few dozen
        bytes from host-known sizes, ``GraphBatch._set_sizes``) and launches ``row_maps``; ``cache.h2d`` does not count these, and they
        lie outside a step captured on ``embed(batch)``."""
        dev = next(self.model.parameters()).device
        if dev.type != "cuda":
            raise RuntimeError(R.GPU_ONLY)
        parts = [self._graph(o, dev) for o in (a, p, n)]
        if any(q.nmax != parts[0].nmax for q in parts):
            raise ValueError("the graphs of a triplet must be padded to the same Nmax")
        if any(q.feats.size(1) != parts[0].feats.size(1) for q in parts):
            raise ValueError("the graphs of a triplet must have the same number of features")
        b = _Triplet()
        b.eb = ep.concat_batches([q.eb for q in parts])
        b.x = torch.cat([q.feats for q in parts] + [R.ghost_zeros(parts[0].nmax, parts[0].feats.size(1), dev)])
        b.sizes = b.eb.g0.sizes
        return b

    # ------------------------------------------------------------------ forward
    def _tail(self, r):
        """readout rows [3, D] -> (dist_p, dist_n, embed_a, embed_p, embed_n): one launch, or the torch composition for a head the
        kernels do not take"""
        pm = self.model.pred_model
        kind = tail_kind(self.model, r)
        if kind == "mlp2":
            return _Mlp2TripletTail.apply(r, pm[0].weight, pm[0].bias, pm[2].weight, pm[2].bias)
        if kind == "linear":
            return _t._TripletTail.apply(r, pm.weight, pm.bias)
        return R.torch_distances(pm(r))

    def embed(self, b):
        """the step on a batch from ``batch()``: the model once with the per-graph statistics of a B = 1 call, then the tail"""
        with R.per_graph_statistics(self.model):
            r = self.model(b.x, b.eb, readout_only=True)
        return self._tail(r)

    def forward(self, a, p, n):
        """a, p, n: objects with ``.graph`` = {'adj', 'feats', 'num_nodes', 'adj_pool_i', 'num_nodes_i', 'pool_adj_i_j'} as
        cross_val.py prepares them ('assign_feats' is not needed: the reference reads it and never uses it)"""
        return self.embed(self.batch(a, p, n))
