"""torch_geometric-named operators on the hot path, backed by the HIP kernels.

(A) what Code/sag actually calls: ``GCNConv``, ``topk``, ``filter_adj``, ``global_max_pool``,
    ``global_mean_pool`` (Code/sag/network.py:2-4, layers.py:1-2) — signatures, parameter names
    (``weight[in,out]``, ``bias``; PyG 1.6.x layout) and return conventions preserved;
(B) the operators BASELINE.json's north_star names: ``SAGEConv``, ``GATConv``, ``SAGPooling``,
    ``dense_diff_pool`` (plus PyG's ``GraphConv``, SAGPooling's default scorer, and ``TopKPooling``, which network.py:3 imports).
Inputs are PyG's: ``x[N,F]`` fp32, ``edge_index[2,E]`` int64 (row 0 = source, row 1 = target), ``batch[N]``.
The COO list is converted to CSR (grouped by target) on the GPU once per distinct edge_index tensor.
"""
import math
import weakref

import numpy as np
import torch
import torch.nn as nn

from . import _native as nat
from . import attention as att
from . import message_passing as mp
from .graph import GraphBatch, exclusive_scan


def _default_device():
    return torch.device("cuda", torch.cuda.current_device()) if torch.cuda.is_available() else torch.device("cpu")


def _f32(*shape, device, zero=False):
    return (torch.zeros if zero else torch.empty)(*shape, dtype=torch.float32, device=device)


_graph_cache = {}
_gat_graph_cache = {}
_eye_cache = {}


def graph_of(edge_index, num_nodes, check_symmetry=False, sizes=None):
    """CSR (rows = targets) of a PyG edge list, cached per edge_index tensor.  ``check_symmetry``: also find out (once per
    edge list, at ingest) whether every edge has its reverse — all TU datasets do —, in which case backward passes reuse
    the CSR instead of building its transpose.  ``sizes`` (np.int64[B], from PyG's ``batch``): the graphs of the mini-batch, for the
    operators that need per-graph structure (readouts, pooling)."""
    if not edge_index.is_cuda:
        raise RuntimeError("two_stage_gnn_amd operators run on the GPU only (no CPU fallback)")
    skey = None if sizes is None else np.asarray(sizes, dtype=np.int64).tobytes()
    key = (edge_index.data_ptr(), tuple(edge_index.shape), edge_index._version, int(num_nodes), skey)
    hit = _graph_cache.get(key)
    if hit is not None and hit[0]() is edge_index:
        g = hit[1]
        if check_symmetry and not getattr(g, "_sym_checked", False):
            _check_symmetry(g, edge_index, num_nodes)
        return g
    if sizes is None:
        g = GraphBatch.from_edge_index(edge_index, num_nodes, ghosts=False)
    else:
        sizes = np.asarray(sizes, dtype=np.int64)
        g = GraphBatch.from_edge_index(edge_index, num_nodes, sizes=sizes, nmax=int(max(1, sizes.max())), ghosts=False)
    if check_symmetry:
        _check_symmetry(g, edge_index, num_nodes)
    if len(_graph_cache) > 16:
        _graph_cache.clear()
    _graph_cache[key] = (weakref.ref(edge_index), g)
    return g


def _check_symmetry(g, edge_index, num_nodes):
    n = int(num_nodes)
    fwd = torch.sort(edge_index[0] * n + edge_index[1]).values
    rev = torch.sort(edge_index[1] * n + edge_index[0]).values
    g.symmetric = bool(torch.equal(fwd, rev))                 # one host sync per distinct edge list (ingest, not the step)
    g._sym_checked = True


def segment_sizes(batch, num_nodes):
    """np.int64[B] graph sizes of PyG's ``batch`` vector (sorted graph ids); cached on the tensor object, so a mini-batch
    pays the host round trip once (a CSR-native collate can set ``batch._tsgnn_sizes`` itself and pay none)."""
    if batch is None:
        return np.array([int(num_nodes)], dtype=np.int64)
    hit = getattr(batch, "_tsgnn_sizes", None)
    if hit is not None and hit[0] == batch._version:
        return hit[1]
    sizes = torch.bincount(batch).cpu().numpy().astype(np.int64)
    batch._tsgnn_sizes = (batch._version, sizes)
    return sizes


def _segments(batch, num_nodes, device):
    """batch[N] (sorted graph ids, PyG convention) -> (sizes np.int64[B], graph_ptr int32[B+1] on device)."""
    sizes = segment_sizes(batch, num_nodes)
    gp = np.zeros(len(sizes) + 1, dtype=np.int32)
    np.cumsum(sizes, out=gp[1:])
    return sizes, torch.from_numpy(gp).to(device)


# ----------------------------------------------------------------------------- small element-wise ops
class _Relu(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        x = x.contiguous()
        y = torch.empty_like(x)
        nat.call("relu_fwd_f32", x, x.numel(), y)
        ctx.save_for_backward(y)
        return y

    @staticmethod
    def backward(ctx, dy):
        (y,) = ctx.saved_tensors
        dx = torch.empty_like(y)
        nat.call("relu_bwd_f32", y, dy.contiguous(), y.numel(), dx)
        return dx


def relu(x):
    return _Relu.apply(x)


class _BiasAdd(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, bias):
        y = x.clone()
        nat.call("broadcast_add_f32", y, y.stride(0), y.size(0), 1, y.size(1), None, bias, bias.numel(), None, 0, 0, 1.0)
        return y

    @staticmethod
    def backward(ctx, dy):
        dy = dy.contiguous()
        return dy, mp.colsum(dy)


def bias_add(x, bias):
    return x if bias is None else _BiasAdd.apply(x, bias)


def linear(x, weight_in_out, bias=None):
    """x @ W (+ b) with W stored [in, out] — the fp32 MFMA kernel."""
    return mp.linear_l2norm(x, weight_in_out, bias, normalize=False)


# ----------------------------------------------------------------------------- GCNConv (a11)
class _GcnPropagate(torch.autograd.Function):
    """A^ x = D^-1/2 (A + I) D^-1/2 x from the per-row coefficients of gcn_norm (no per-edge weight tensor):
    tsgnn_gcn_propagate_f32 forward, the same operator on A^T backward (A^T = A for symmetric edge lists)."""

    @staticmethod
    def forward(ctx, x, g):
        from . import sag_stack as ss
        x = x.contiguous()
        dinv, self_w = ss.gcn_coef(g)
        ctx.g = g
        y, _ = ss.propagate(g.rowptr, g.col, dinv, self_w, x, g.total_rows)
        return y

    @staticmethod
    def backward(ctx, dy):
        from . import sag_stack as ss
        g = ctx.g
        dinv, self_w = ss.gcn_coef(g)
        rp_t, col_t = (g.rowptr, g.col) if g.symmetric else g.transposed(None)[:2]
        dx, _ = ss.propagate(rp_t, col_t, dinv, self_w, dy.contiguous(), g.total_rows)
        return dx, None


def _gcn_propagate_learnt(x, g, edge_weight, fill):
    """A^ x with edge weights that require grad (PyG gcn_norm is differentiable in them; no reference call site passes weights,
    layers.py:18).  The normalisation is a handful of per-entry device operations under autograd; the aggregation and the sampled
    product dval[e] = dy[i] . x[col[e]] of its backward are the native kernels (tsgnn_csr_spmm_f32, tsgnn_sddmm_rows_f32)."""
    R, nnz = g.total_rows, g.nnz
    w = edge_weight.float().view(-1)
    eid = getattr(g, "eid", None)
    w = w[eid[:nnz].long()] if eid is not None else w[:nnz]            # CSR entry order
    rows = torch.repeat_interleave(torch.arange(R, device=x.device), (g.rowptr[1:] - g.rowptr[:-1]).long())
    cols = g.col[:nnz].long()
    no_self = torch.ones(R, device=x.device)
    no_self[rows[rows == cols]] = 0.0                                  # add_remaining_self_loops keeps an existing self loop
    deg = torch.zeros(R, device=x.device).index_add(0, rows, w) + fill * no_self
    dinv = torch.where(deg > 0, deg.clamp(min=1e-38).rsqrt(), torch.zeros_like(deg))
    val = dinv[rows] * w * dinv[cols]
    self_w = dinv * dinv * (fill * no_self)
    if val.numel() == 0:
        val = None
    return mp.aggregate(x, g, False, val=val, self_w=self_w)


def gcn_propagate(x, g, edge_weight=None, improved=False):
    """A^ x.  Unit weights, fill 1 (every reference call site, network.py:34, layers.py:18): the per-row-coefficient kernels.
    ``edge_weight`` (per edge of the edge list the graph was built from, or per CSR entry for a GraphBatch without ``eid``) and
    ``improved`` (self loops of weight 2) take PyG's general gcn_norm: per-entry normalised weights (tsgnn_gcn_norm_f32) and the
    weighted aggregation; weights that require grad take _gcn_propagate_learnt."""
    if edge_weight is None and not improved and g.val is None:
        return _GcnPropagate.apply(x, g)
    val = g.val
    if edge_weight is not None:
        if edge_weight.requires_grad:
            return _gcn_propagate_learnt(x, g, edge_weight, 2.0 if improved else 1.0)
        w = edge_weight.detach().contiguous().float().view(-1)
        eid = getattr(g, "eid", None)
        val = w[eid[: g.nnz].long()] if eid is not None else w          # CSR entry order
    R = g.total_rows
    dev = x.device
    dinv, self_w = torch.empty(R, device=dev), torch.empty(R, device=dev)
    val_out = torch.empty(max(g.nnz, 1), device=dev)
    nat.call("gcn_norm_f32", g.rowptr, g.col, val, R, 2.0 if improved else 1.0, dinv, val_out, self_w)
    return mp.aggregate(x, g, False, val=val_out, self_w=self_w)


class GCNConv(nn.Module):
    """out = D^-1/2 (A+I) D^-1/2 (x W) + b — PyG GCNConv as called at Code/sag/network.py:19-23, layers.py:12."""

    def __init__(self, in_channels, out_channels, improved=False, cached=False, bias=True, **kwargs):
        super().__init__()
        self.improved = bool(improved)
        self.in_channels, self.out_channels = in_channels, out_channels
        dev = _default_device()
        self.weight = nn.Parameter(torch.empty(in_channels, out_channels, device=dev))
        self.bias = nn.Parameter(torch.empty(out_channels, device=dev)) if bias else None
        self.reset_parameters()

    def reset_parameters(self):
        stdv = math.sqrt(6.0 / (self.weight.size(0) + self.weight.size(1)))        # PyG glorot
        self.weight.data.uniform_(-stdv, stdv)
        if self.bias is not None:
            self.bias.data.zero_()

    def forward(self, x, edge_index, edge_weight=None):
        g = edge_index if isinstance(edge_index, GraphBatch) else graph_of(edge_index, x.size(0))
        xw = linear(x, self.weight)
        return bias_add(gcn_propagate(xw, g, edge_weight, self.improved), self.bias)


# ----------------------------------------------------------------------------- topk / filter_adj (a12, a13)
def topk(x, ratio, batch, min_score=None):
    """PyG topk (layers.py:20): per graph the ceil(ratio*n) best nodes, descending.  Returns int64 perm."""
    if min_score is not None:
        # PyG's threshold mode: keep every node whose score exceeds min(min_score, its graph's maximum - 1e-7), in node order
        # (at least the best node of each graph survives).  Never used by the reference (layers.py:20 passes a ratio).
        score = x.contiguous().float().view(-1)
        if batch is None:
            batch = torch.zeros(score.numel(), dtype=torch.int64, device=score.device)
        B = int(batch.max().item()) + 1 if batch.numel() else 0
        smax = torch.full((B,), float("-inf"), device=score.device).scatter_reduce_(0, batch, score, "amax")[batch] - 1e-7
        return (score > smax.clamp(max=float(min_score))).nonzero(as_tuple=False).view(-1)
    score = x.contiguous().float().view(-1)
    N = score.numel()
    sizes, gp = _segments(batch, N, score.device)
    k = np.ceil(np.float32(ratio) * sizes.astype(np.float32)).astype(np.int64)      # float32, as PyG computes it
    k = np.minimum(k, sizes)
    kp = np.zeros(len(k) + 1, dtype=np.int32)
    np.cumsum(k, out=kp[1:])
    perm = torch.empty(max(int(kp[-1]), 1), dtype=torch.int32, device=score.device)
    nat.call("topk_segments_f32", score, gp, torch.from_numpy(kp).to(score.device), len(sizes), int(sizes.max()), perm, None)
    return perm[: int(kp[-1])].long()


def filter_adj(edge_index, edge_attr, perm, num_nodes=None):
    """PyG filter_adj (layers.py:23-24): relabel nodes by perm, drop edges that lost an end."""
    N = int(num_nodes) if num_nodes is not None else int(edge_index.max().item()) + 1
    dev = edge_index.device
    ei = edge_index.contiguous()
    E = int(ei.size(1))
    p32 = perm.to(torch.int32).contiguous()
    new_id = torch.empty(max(N, 1), dtype=torch.int32, device=dev)
    flag = torch.zeros(max(E, 1), dtype=torch.int32, device=dev)
    nat.call("filter_edges_mark", p32, p32.numel(), N, ei[0], ei[1], E, new_id, flag)
    pos = exclusive_scan(flag[:E] if E else flag[:0])
    E2 = int(pos[-1].item())
    out = torch.empty(2, E2, dtype=torch.int64, device=dev)
    kept = torch.empty(max(E2, 1), dtype=torch.int64, device=dev)
    if E2 > 0:
        nat.call("filter_edges_compact", ei[0], ei[1], E, new_id, flag, pos, out[0], out[1], kept)
    if edge_attr is not None:
        edge_attr = edge_attr[kept[:E2]]
    return out, edge_attr


# ----------------------------------------------------------------------------- readouts (a14)
class _SegmentMean(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, gp, B, ctx_max_seg):
        x = x.contiguous()
        ctx.save_for_backward(gp)
        ctx.shape = x.shape
        return att.segment_wsum(x, None, 1, x.size(1), gp, B, mean=True, max_seg=ctx_max_seg)

    @staticmethod
    def backward(ctx, dout):
        (gp,) = ctx.saved_tensors
        R, F = ctx.shape
        dx = _f32(R, F, device=dout.device, zero=True)
        sizes = (gp[1:] - gp[:-1]).to(torch.float32).clamp(min=1).unsqueeze(1)
        scaled = (dout / sizes).contiguous()
        # dx[r,:] += dout[seg(r),:] / n_seg : ragged broadcast through the row->graph map
        rows = torch.repeat_interleave(torch.arange(gp.numel() - 1, device=gp.device), (gp[1:] - gp[:-1]).long())
        dx = scaled[rows]
        return dx, None, None, None


def _pool_struct(x, batch, size):
    sizes, gp = _segments(batch, x.size(0), x.device)
    B = len(sizes) if size is None else int(size)
    return sizes, gp, B


def global_mean_pool(x, batch, size=None):
    sizes, gp, B = _pool_struct(x, batch, size)
    return _SegmentMean.apply(x, gp, B, int(sizes.max()) if len(sizes) else 0)


def _pool_graph(x, batch):
    """structure-only GraphBatch of PyG's ``batch`` vector, cached on the tensor object (a step replayed from a hipGraph must not
    upload anything)"""
    hit = getattr(batch, "_tsgnn_pool_g", None) if batch is not None else None
    if hit is not None and hit[0] == batch._version:
        return hit[1]
    sizes = segment_sizes(batch, x.size(0))
    g = GraphBatch.structure_only(sizes, int(max(1, sizes.max())), x.device, ghosts=False)
    if batch is not None:
        batch._tsgnn_pool_g = (batch._version, g)
    return g


def global_max_pool(x, batch, size=None):
    return mp.readout_max(x, _pool_graph(x, batch))


# ----------------------------------------------------------------------------- gated gather of the kept nodes
class _GatherGate(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, score, perm32, use_tanh):
        x = x.contiguous()
        score = score.contiguous()
        K, F = perm32.numel(), x.size(1)
        out = _f32(K, F, device=x.device)
        nat.call("gather_gate_fwd_f32", x, x.stride(0), score, perm32, K, F, int(use_tanh), out, out.stride(0))
        ctx.save_for_backward(x, score, perm32)
        ctx.use_tanh = use_tanh
        return out

    @staticmethod
    def backward(ctx, dout):
        x, score, perm32 = ctx.saved_tensors
        dout = dout.contiguous()
        K, F = perm32.numel(), x.size(1)
        dx = torch.zeros_like(x)
        ds = torch.zeros_like(score)
        nat.call("gather_gate_bwd_f32", x, x.stride(0), score, perm32, K, F, int(ctx.use_tanh), dout, dout.stride(0), dx,
                 dx.stride(0), ds)
        return dx, ds, None, None


def gather_gate(x, score, perm, use_tanh=True):
    """x[perm] * tanh(score[perm]).view(-1,1)  (Code/sag/layers.py:21) as one kernel."""
    return _GatherGate.apply(x, score, perm.to(torch.int32).contiguous(), bool(use_tanh))


# ----------------------------------------------------------------------------- north_star-named operators (a15)
def _inv_degree(g):
    """1 / max(in-degree, 1) per row, cached on the graph"""
    inv = getattr(g, "_inv_deg", None)
    if inv is None:
        inv = g._inv_deg = (1.0 / (g.rowptr[1:] - g.rowptr[:-1]).clamp(min=1).to(torch.float32)).unsqueeze(1)
    return inv


def _mean_aggregate(x, g):
    """mean_{j in N(i)} x_j = (A x)_i / deg_i: the unit-weight aggregation kernel (fixed-width index table while the batch is
    cache-resident) followed by a row scale; its backward is A^T (dy / deg) through the same operator.  No host round trip."""
    return mp.aggregate(x, g, val=None) * _inv_degree(g)


class SAGEConv(nn.Module):
    """PyG SAGEConv (mean aggregator): lin_l(mean_j x_j) + lin_r(x_i) [, L2-normalised].  No call site in the reference (north_star
    names it).  ONE launch forward (pyg_sage.py / csrc/sageconv.hip: gather + 1/deg + both products + bias + normalise);
    backward: weight-gradient slabs, one reduction into nn.Linear's layout, the input gradient through the same fused kernel."""

    aggr = "mean"

    def __init__(self, in_channels, out_channels, normalize=False, root_weight=True, bias=True, **kwargs):
        super().__init__()
        self.in_channels, self.out_channels = in_channels, out_channels
        self.normalize, self.root_weight = normalize, root_weight
        dev = _default_device()
        self.lin_l = nn.Linear(in_channels, out_channels, bias=bias).to(dev)
        if root_weight:
            self.lin_r = nn.Linear(in_channels, out_channels, bias=False).to(dev)

    def _graph(self, x, edge_index):
        return edge_index if isinstance(edge_index, GraphBatch) else graph_of(edge_index, x.size(0), check_symmetry=True)

    def forward(self, x, edge_index):
        from . import pyg_sage as ps
        g = self._graph(x, edge_index)
        if self.root_weight and g.val is None and self.out_channels % 4 == 0 and ps.conv_ok(self.in_channels, self.out_channels):
            return ps.sage_conv(x, g, self.lin_l.weight, self.lin_l.bias, self.lin_r.weight, mean=self.aggr == "mean",
                                normalize=self.normalize)
        agg = mp.aggregate(x, g, val=None)
        if self.aggr == "mean":
            agg = agg * _inv_degree(g)
        out = mp.linear_oi(agg, self.lin_l.weight, self.lin_l.bias)
        if self.root_weight:
            out = out + mp.linear_oi(x, self.lin_r.weight)
        if self.normalize:
            out = torch.nn.functional.normalize(out, p=2.0, dim=-1)
        return out


class GraphConv(SAGEConv):
    """PyG GraphConv: lin_l(sum_j x_j) + lin_r(x_i) — SAGPooling's default scorer.  The same fused launch without the 1/deg scale."""

    aggr = "add"

    def __init__(self, in_channels, out_channels, aggr="add", bias=True, **kwargs):
        super().__init__(in_channels, out_channels, normalize=False, root_weight=True, bias=bias)
        self.aggr = aggr

    def forward(self, x, edge_index, edge_weight=None):
        if edge_weight is not None:
            raise NotImplementedError("GraphConv(edge_weight=) has no call site (Code/sag passes none)")
        return super().forward(x, edge_index)


class GATConv(nn.Module):
    """PyG GATConv: per-TARGET edge softmax (standard GAT), self loops added, heads concatenated / averaged, attention dropout.
    No call site in the reference (north_star names it; SURVEY 8 a15 — PARITY UNPINNED).  Parameters as PyG 1.6: lin_l (shared
    projection, no bias), att_l / att_r [1, H, C] (dotted with the SOURCE / TARGET node), bias."""

    def __init__(self, in_channels, out_channels, heads=1, concat=True, negative_slope=0.2, dropout=0.0, bias=True, **kwargs):
        super().__init__()
        self.in_channels = in_channels
        self.heads, self.out_channels, self.concat, self.negative_slope = heads, out_channels, concat, negative_slope
        self.dropout = float(dropout)
        dev = _default_device()
        self.lin_l = nn.Linear(in_channels, heads * out_channels, bias=False).to(dev)
        self.att_l = nn.Parameter(torch.empty(1, heads, out_channels, device=dev))
        self.att_r = nn.Parameter(torch.empty(1, heads, out_channels, device=dev))
        self.bias = nn.Parameter(torch.zeros(heads * out_channels if concat else out_channels, device=dev)) if bias else None
        nn.init.xavier_uniform_(self.lin_l.weight)
        nn.init.xavier_uniform_(self.att_l)
        nn.init.xavier_uniform_(self.att_r)
        self.last_drop_mult = None          # [nnz, H] multiplier of the most recent training forward, in g.eid order (tests)

    @staticmethod
    def _loop_graph(edge_index, n, sizes=None):
        """remove_self_loops + add_self_loops, as a CSR cached per edge_index tensor (the boolean compaction and the COO
        ingest each cost a host round trip: once per edge list, not per forward)"""
        skey = None if sizes is None else np.asarray(sizes, dtype=np.int64).tobytes()
        key = (edge_index.data_ptr(), tuple(edge_index.shape), edge_index._version, int(n), skey)
        hit = _gat_graph_cache.get(key)
        if hit is not None and hit[0]() is edge_index:
            return hit[1]
        keep = edge_index[0] != edge_index[1]
        loop = torch.arange(n, device=edge_index.device)
        ei = torch.cat([edge_index[:, keep], torch.stack([loop, loop])], dim=1)
        if sizes is None:
            g = GraphBatch.from_edge_index(ei, n, ghosts=False)
        else:
            sizes = np.asarray(sizes, dtype=np.int64)
            g = GraphBatch.from_edge_index(ei, n, sizes=sizes, nmax=int(max(1, sizes.max())), ghosts=False)
        g.transpose_map()
        g.loop_edge_index = ei                                # (kept alive: tests rebuild the oracle's edge order from it)
        if len(_gat_graph_cache) > 16:
            _gat_graph_cache.clear()
        _gat_graph_cache[key] = (weakref.ref(edge_index), g)
        return g

    def forward(self, x, edge_index, wp=None, apply_elu=False):
        """wp: this layer's packed projection from pyg_gat.pack_layers (a model packs all of its layers in one launch); apply_elu:
        ELU folded into the fused launch (a model's activation between layers)"""
        from . import pyg_gat as pgat
        from . import pyg_sage as ps
        n = x.size(0)
        g = edge_index if isinstance(edge_index, GraphBatch) else self._loop_graph(edge_index, n)
        if pgat.conv_ok(self, x):
            if wp is None:
                wp = pgat.pack_layers([self])[0]
            bias = self.bias if (self.bias is None or self.bias.data_ptr() % 16 == 0) else self.bias.clone()
            return pgat.gat_conv(ps._rows16(x), wp, bias, g, self.heads, self.out_channels, self.negative_slope,
                                 mean_heads=not self.concat, apply_elu=apply_elu)
        h = mp.linear_oi(x, self.lin_l.weight)
        mult = None
        if self.training and self.dropout > 0.0:
            # F.dropout(alpha, p) on the normalised coefficients (one per edge of the self-looped list and head)
            keep = torch.empty(max(g.nnz, 1), self.heads, dtype=torch.float32, device=x.device).bernoulli_(1.0 - self.dropout)
            mult = keep * (1.0 / (1.0 - self.dropout))
            self.last_drop_mult = mult
        # entry (i = target row, j = source col): score = att_r.h_i + att_l.h_j, softmax over the row
        pre = att.attention_aggregate(h, self.att_r.view(self.heads, -1), self.att_l.view(self.heads, -1), g, self.heads,
                                      self.negative_slope, by_column=False, uniform_isolated=False, drop_mult=mult)
        out = pre if self.concat else att.elu_heads(pre, self.heads, mean_heads=True, apply_elu=False)
        out = bias_add(out, self.bias)
        return att.elu_heads(out, 1, mean_heads=False, apply_elu=True) if apply_elu else out


class SAGPooling(nn.Module):
    """PyG SAGPooling: score = tanh(GNN(x)), top-k on the score, x[perm]*score[perm]."""

    def __init__(self, in_channels, ratio=0.5, GNN=GraphConv, min_score=None, multiplier=1, nonlinearity=torch.tanh, **kwargs):
        super().__init__()
        self.min_score = min_score
        self.in_channels, self.ratio, self.multiplier, self.nonlinearity = in_channels, ratio, multiplier, nonlinearity
        self.gnn = GNN(in_channels, 1, **kwargs)

    def forward(self, x, edge_index, edge_attr=None, batch=None, attn=None):
        if batch is None:
            batch = edge_index.new_zeros(x.size(0))
        attn = x if attn is None else attn
        raw = self.gnn(attn, edge_index).view(-1)
        if self.min_score is not None:
            # PyG's threshold mode: the score is the per-graph softmax of the GNN output, kept nodes are those above min_score
            B = int(batch.max().item()) + 1
            mx = torch.full((B,), float("-inf"), device=raw.device).scatter_reduce(0, batch, raw.detach(), "amax")
            e = torch.exp(raw - mx[batch])
            score = e / torch.zeros(B, device=raw.device).index_add(0, batch, e)[batch]
            perm = topk(score, self.ratio, batch, self.min_score)
            xo = x[perm] * score[perm].view(-1, 1)
            if self.multiplier != 1:
                xo = self.multiplier * xo
            ei, edge_attr = filter_adj(edge_index, edge_attr, perm, num_nodes=raw.numel())
            return xo, ei, edge_attr, batch[perm], perm, score[perm]
        perm = topk(raw, self.ratio, batch)                           # tanh is monotone: same selection as PyG
        if self.nonlinearity is torch.tanh:
            xo = gather_gate(x, raw, perm, use_tanh=True)
            score_perm = torch.tanh(raw[perm])
        else:
            score = self.nonlinearity(raw)
            xo = x[perm] * score[perm].view(-1, 1)
            score_perm = score[perm]
        if self.multiplier != 1:
            xo = self.multiplier * xo
        ei, edge_attr = filter_adj(edge_index, edge_attr, perm, num_nodes=raw.numel())
        return xo, ei, edge_attr, batch[perm], perm, score_perm


class TopKPooling(nn.Module):
    """PyG TopKPooling (imported beside GraphConv and never called, Code/sag/network.py:3): score = tanh(x . p / ||p||), the
    ceil(ratio n) best nodes of every graph, x[perm] * score[perm].  Same kernels as SAGPooling with a projection as the scorer."""

    def __init__(self, in_channels, ratio=0.5, min_score=None, multiplier=1, nonlinearity=torch.tanh):
        super().__init__()
        self.in_channels, self.ratio, self.min_score = in_channels, ratio, min_score
        self.multiplier, self.nonlinearity = multiplier, nonlinearity
        self.weight = nn.Parameter(torch.empty(1, in_channels, device=_default_device()))
        self.reset_parameters()

    def reset_parameters(self):
        bound = 1.0 / math.sqrt(self.in_channels)                      # PyG's uniform(size, tensor)
        with torch.no_grad():
            self.weight.uniform_(-bound, bound)

    def forward(self, x, edge_index, edge_attr=None, batch=None, attn=None):
        if batch is None:
            batch = edge_index.new_zeros(x.size(0))
        attn = x if attn is None else attn
        attn = attn.unsqueeze(-1) if attn.dim() == 1 else attn
        if self.min_score is not None:
            # PyG's threshold mode: per-graph softmax of the raw projection, nodes above min_score
            raw = linear(attn, self.weight.t()).view(-1)
            B = int(batch.max().item()) + 1
            mx = torch.full((B,), float("-inf"), device=raw.device).scatter_reduce(0, batch, raw.detach(), "amax")
            e = torch.exp(raw - mx[batch])
            score = e / torch.zeros(B, device=raw.device).index_add(0, batch, e)[batch]
            perm = topk(score, self.ratio, batch, self.min_score)
            xo = x[perm] * score[perm].view(-1, 1)
            score_perm = score[perm]
        else:
            raw = linear(attn, (self.weight / self.weight.norm(p=2, dim=-1)).t()).view(-1)
            if self.nonlinearity is torch.tanh:
                perm = topk(raw, self.ratio, batch)                    # tanh is monotone: same selection as PyG
                xo = gather_gate(x, raw, perm, use_tanh=True)
                score_perm = torch.tanh(raw[perm])
            else:
                score = self.nonlinearity(raw)
                perm = topk(score, self.ratio, batch)
                xo = x[perm] * score[perm].view(-1, 1)
                score_perm = score[perm]
        if self.multiplier != 1:
            xo = self.multiplier * xo
        ei, edge_attr = filter_adj(edge_index, edge_attr, perm, num_nodes=raw.numel())
        return xo, ei, edge_attr, batch[perm], perm, score_perm


class _SoftmaxEntropy(torch.autograd.Function):
    """(s, h) = (softmax(logits, -1) * mask, sum over the rows of -sum_k s log(s + eps)): dense_diff_pool's assignment and the numerator of
    its entropy loss in one launch each way (tsgnn_row_softmax_ent_{fwd,bwd}_f32)"""

    @staticmethod
    def forward(ctx, logits, mask, eps):
        x = logits.contiguous()
        rows, K = x.shape
        y = torch.empty_like(x)
        hpart = torch.empty((rows + 3) // 4, dtype=torch.float32, device=x.device)
        nat.call("row_softmax_ent_fwd_f32", x, x.stride(0), rows, K, mask, float(eps), y, y.stride(0), hpart)
        ctx.save_for_backward(y, mask)
        ctx.eps = float(eps)
        return y, hpart.sum()

    @staticmethod
    def backward(ctx, ds, gh):
        y, mask = ctx.saved_tensors
        ds = ds.contiguous() if ds is not None else None
        gh = gh.contiguous().view(1) if gh is not None else None
        dx = torch.empty_like(y)
        nat.call("row_softmax_ent_bwd_f32", y, y.stride(0), ds, ds.stride(0) if ds is not None else 0, mask, gh, 1.0, ctx.eps,
                 y.size(0), y.size(1), dx, dx.stride(0))
        return dx, None, None


_LINK_PARTS = 512        # blocks sharing the fp64 reduction of the link loss (config 5: 8 K adjacency floats each)


class _LinkLoss(torch.autograd.Function):
    """dense_diff_pool's link loss ||adj - s s^T||_F / adj.numel() from ao = s^T adj s and G = s^T s without the [B, N, N] product:
    d2 = ||adj||^2 - 2 tr(ao) + ||G||^2 accumulated in fp64, two launches forward and one backward (tsgnn_diffpool_link_{fwd,bwd}_f32)"""

    @staticmethod
    def forward(ctx, adj, ao, G):
        adj, ao, G = adj.contiguous(), ao.contiguous(), G.contiguous()
        part = torch.empty(_LINK_PARTS, dtype=torch.float64, device=adj.device)
        link = torch.empty((), dtype=torch.float32, device=adj.device)
        coef = torch.empty(1, dtype=torch.float64, device=adj.device)
        nat.call("diffpool_link_fwd_f32", adj, adj.numel(), ao, G, G.size(0), G.size(1), part, _LINK_PARTS, link, coef)
        ctx.save_for_backward(adj, G, coef)
        return link

    @staticmethod
    def backward(ctx, g):
        adj, G, coef = ctx.saved_tensors
        dG, dao = torch.empty_like(G), torch.empty_like(G)
        dadj = torch.empty_like(adj) if ctx.needs_input_grad[0] else None
        nat.call("diffpool_link_bwd_f32", g.contiguous(), coef, G, G.size(0), G.size(1), adj, adj.numel(), dG, dao, dadj)
        return dadj, dao, dG


def dense_diff_pool(x, adj, s, mask=None, eps=1e-15):
    """PyG dense_diff_pool: (s^T x, s^T adj s, link loss, entropy loss) with s = softmax(s, -1) [* mask].

    The contractions run on fp32 MFMA (diffpool.diffpool_contract_dense).  The link loss ||adj - s s^T||_F / numel never forms the
    [B, N, N] product s s^T (config 5: 16 x 512 x 512 x 64 x 2 = 0.54 GFLOP and three 16 MB tensors for one scalar):
        ||adj - s s^T||^2 = ||adj||^2 - 2 tr(s^T adj s) + ||s^T s||^2        (<adj, s s^T> = tr(s^T adj s);  ||s s^T||_F = ||s^T s||_F)
    with tr(s^T adj s) read off the pooled adjacency that is computed anyway and G = s^T s a [B, K, K] product; its gradient reaches s
    (and adj) through those two products' own backward.  Softmax, mask and the entropy term are one launch each way.

    The three terms are accumulated in fp64 (_LinkLoss), but tr(s^T adj s) and G are fp32 products and the terms cancel when s s^T
    reproduces adj, so the link loss is good to an absolute bound, not a relative one:
        |link - ||adj - s s^T||_F / numel|  <=  8 sqrt(eps32 (||adj||^2 + 2 |tr(s^T adj s)| + ||s^T s||^2)) / numel,   eps32 = 2^-23.
    Where the computed d2 = ||adj - s s^T||^2 is <= 0 the link loss is 0 and passes no gradient (torch.norm's choice at 0, where
    sqrt' is inf); elsewhere its gradient is 0.5 / sqrt(d2) times d2's.  The choice is made on the device: no host sync, capture-safe."""
    from .diffpool import bmm, diffpool_contract_dense
    x = x.unsqueeze(0) if x.dim() == 2 else x
    adj = adj.unsqueeze(0) if adj.dim() == 2 else adj
    s = s.unsqueeze(0) if s.dim() == 2 else s
    B, N, K = s.shape
    m = mask.reshape(B * N).to(torch.float32).contiguous() if mask is not None else None
    s, h = _SoftmaxEntropy.apply(s.reshape(B * N, K), m, eps)
    s = s.reshape(B, N, K)
    if mask is not None:
        x = x * mask.view(B, N, 1).to(x.dtype)
    out, out_adj = diffpool_contract_dense(s, x, adj)
    G = bmm(s, s, trans_a=True)                                                   # s^T s  [B, K, K]
    link = _LinkLoss.apply(adj, out_adj, G)
    ent = h / (B * N)
    return out, out_adj, link, ent


# ----------------------------------------------------------------------------- graph classifiers on the PyG-named layers
class SageNet(nn.Module):
    """BASELINE configs 1-2 as worded ("MUTAG SAGEConv 2-layer h=64", "PROTEINS SAGEConv 3-layer h=128"): the shape of the reference's one
    PyG network (Code/sag/network.py:9-53 — conv + ReLU per layer, [gmp || gap] of every layer summed, lin1 / lin2 / lin3, log_softmax)
    with SAGEConv layers and no pooling.  ``fused=True``: the conv stack is ONE autograd node (pyg_sage._SageStack: one launch per
    layer forward, readouts in the layers' epilogues) and the head one launch each way; ``fused=False`` composes the drop-in modules."""

    def __init__(self, num_features, nhid, num_classes, num_layers=3, dropout_ratio=0.0, fused=True):
        super().__init__()
        self.num_features, self.nhid, self.num_classes, self.num_layers = num_features, nhid, num_classes, num_layers
        self.dropout_ratio, self.fused = dropout_ratio, fused
        self.convs = nn.ModuleList([SAGEConv(num_features if l == 0 else nhid, nhid) for l in range(num_layers)])
        dev = _default_device()
        self.lin1 = nn.Linear(nhid * 2, nhid).to(dev)
        self.lin2 = nn.Linear(nhid, nhid // 2).to(dev)
        self.lin3 = nn.Linear(nhid // 2, num_classes).to(dev)

    def graph(self, data):
        x = data.x
        if isinstance(data.edge_index, GraphBatch):
            return data.edge_index
        batch = getattr(data, "batch", None)
        return graph_of(data.edge_index, x.size(0), check_symmetry=True, sizes=segment_sizes(batch, x.size(0)))

    def head(self, x):
        if mp.mlp3_ok(x, self.lin1, self.lin2, self.lin3):
            return mp.mlp3_log_softmax(x, self.lin1, self.lin2, self.lin3, self.dropout_ratio, self.training)
        x = relu(mp.linear_oi(x, self.lin1.weight, self.lin1.bias))
        x = torch.nn.functional.dropout(x, p=self.dropout_ratio, training=self.training)
        x = relu(mp.linear_oi(x, self.lin2.weight, self.lin2.bias))
        return torch.nn.functional.log_softmax(mp.linear_oi(x, self.lin3.weight, self.lin3.bias), dim=-1)

    def forward(self, data):
        from . import pyg_sage as ps
        g = self.graph(data)
        x = data.x
        if self.fused and ps.stack_ok(g, list(self.convs), x):
            return self.head(ps.sage_stack(x, g, list(self.convs)))
        batch = getattr(data, "batch", None)
        if batch is None:
            batch = torch.zeros(x.size(0), dtype=torch.int64, device=x.device)
        out = None
        for conv in self.convs:
            x = relu(conv(x, g))
            r = torch.cat([global_max_pool(x, batch), global_mean_pool(x, batch)], dim=1)
            out = r if out is None else out + r
        return self.head(out)


class GatNet(nn.Module):
    """BASELINE config 3 as worded ("DD GATConv 2-layer 4-head h=64 batch=32"): GATConv(F -> heads x nhid, concat) + ELU, ...,
    GATConv(heads x nhid -> nhid, mean over heads), global_max_pool, Linear, log_softmax — the layer shapes of the reference's
    DGATEncoderGraph (encoders_GAT.py:175-198: concat layers, a mean layer, max over nodes, Linear) on PyG's per-target GATConv."""

    def __init__(self, num_features, nhid, num_classes, heads=4, num_layers=2, dropout=0.0):
        super().__init__()
        self.heads, self.nhid = heads, nhid
        convs = []
        for l in range(num_layers):
            last = l == num_layers - 1
            convs.append(GATConv(num_features if l == 0 else heads * nhid, nhid, heads=heads, concat=not last, dropout=dropout))
        self.convs = nn.ModuleList(convs)
        self.lin = nn.Linear(nhid, num_classes).to(_default_device())

    def graph(self, data):
        if isinstance(data.edge_index, GraphBatch):
            return data.edge_index
        return GATConv._loop_graph(data.edge_index, data.x.size(0), sizes=segment_sizes(getattr(data, "batch", None), data.x.size(0)))

    def features(self, data):
        from . import pyg_gat as pgat
        g = self.graph(data)
        x = data.x
        wps = pgat.pack_layers(list(self.convs)) if all(pgat.conv_ok(c, x) for c in self.convs) else [None] * len(self.convs)
        for l, conv in enumerate(self.convs):
            x = conv(x, g, wp=wps[l], apply_elu=l < len(self.convs) - 1)
        r = mp.readout_max(x, g) if g.row_graph is not None and g.n_ghost == 0 else global_max_pool(x, getattr(data, "batch", None))
        return r

    def logits(self, data):
        """lin(readout): the head as ONE launch each way (the two-Linear head kernels with W2 = I: 1 * v + 0 * u is exact), so that a
        cross-entropy on it can be folded into the head's backward (mp.cross_entropy under FlatTrainer(defer_loss=True))"""
        r = self.features(data)
        C = self.lin.out_features
        if mp.HEAD_TAIL is not None and r.is_cuda and r.size(1) % 4 == 0 and r.size(1) <= 2048 and r.size(0) <= 1024 \
                and self.lin.weight.data_ptr() % 16 == 0:
            eye = _eye_cache.get((C, r.device))
            if eye is None:
                eye = _eye_cache[(C, r.device)] = torch.eye(C, dtype=torch.float32, device=r.device)
            y = mp._Head2.apply(r, self.lin.weight, self.lin.bias, eye, None)[1]
            y._tsgnn_defer_ce = True
            return y
        return mp.linear_oi(r, self.lin.weight, self.lin.bias)

    def forward(self, data):
        return torch.nn.functional.log_softmax(self.logits(data), dim=-1)

    def loss(self, data, label):
        """nll_loss(log_softmax(lin(readout))) = cross_entropy(lin(readout)): the fused softmax + CE kernel (folded into the head's
        backward under FlatTrainer(defer_loss=True))"""
        return mp.cross_entropy(self.logits(data), label)


class SagePoolNet(nn.Module):
    """BASELINE config 4 as worded ("IMDB-BINARY SAGPool (ratio 0.5) + SAGEConv h=128 batch=128"): Code/sag/network.py:9-53 with its
    GCNConv layers replaced by SAGEConv and its pooling by PyG's SAGPooling (GraphConv scorer) — conv + ReLU, pool, [gmp || gap] per
    level, summed; lin1-3; log_softmax.

    ``fused=True`` (default): the three levels run as ONE sync-free autograd node, sag_stack_sage._SagSageStack with the GraphConv
    scorer (two per-graph launches per level each way, no host round trip: the step can be captured in a hipGraph / GraphedStep), when
    every one of these holds (``fused_route``):
      - nhid % 4 == 0 and the per-graph kernels take nhid (sag_stack.supported);
      - every SAGEConv has a lin_l bias, root_weight and no normalize;
      - every SAGPooling has ratio = pooling_ratio, a GraphConv(aggr="add") scorer with a lin_l bias, min_score None, multiplier 1,
        nonlinearity torch.tanh;
      - the edge list is unit-weight and symmetric, and no graph has more than tsgnn_sag_pool_graph_max_nodes() nodes.
    Anything else, and ``fused=False``, composes the drop-in operators level by level (top-k / filter_adj size their outputs from the
    data: three host round trips per level, like PyG).  ``last_perms``: per level, int64 rows of that level, grouped by graph, descending
    score within a graph, on both paths (the fused path converts its int32 buffers when read)."""

    def __init__(self, num_features, nhid, num_classes, pooling_ratio=0.5, dropout_ratio=0.0, fused=True):
        super().__init__()
        self.nhid, self.pooling_ratio, self.dropout_ratio, self.fused = nhid, pooling_ratio, dropout_ratio, fused
        self.convs = nn.ModuleList([SAGEConv(num_features if l == 0 else nhid, nhid) for l in range(3)])
        self.pools = nn.ModuleList([SAGPooling(nhid, ratio=pooling_ratio) for _ in range(3)])
        dev = _default_device()
        self.lin1 = nn.Linear(nhid * 2, nhid).to(dev)
        self.lin2 = nn.Linear(nhid, nhid // 2).to(dev)
        self.lin3 = nn.Linear(nhid // 2, num_classes).to(dev)
        self.last_perms = None

    @property
    def last_perms(self):
        if self._perms_fused is not None:
            return [p.long() for p in self._perms_fused]
        return self._perms

    @last_perms.setter
    def last_perms(self, v):
        self._perms, self._perms_fused = v, None

    def _modules_fusable(self):
        from . import sag_stack
        convs_ok = all(c.lin_l.bias is not None and c.root_weight and not c.normalize for c in self.convs)
        pools_ok = all(isinstance(p.gnn, GraphConv) and p.gnn.aggr == "add" and p.gnn.lin_l.bias is not None and p.min_score is None
                       and p.multiplier == 1 and p.nonlinearity is torch.tanh and p.ratio == self.pooling_ratio for p in self.pools)
        return self.fused and self.nhid % 4 == 0 and sag_stack.supported(self.nhid) and convs_ok and pools_ok

    def fused_route(self, data):
        """(graph, plan) when forward(data) takes the one-node stack, else None (see the class docstring).  Host work on the first call
        for an edge list / batch only (symmetry check, graph sizes), as the composed path's."""
        if not self._modules_fusable():
            return None
        from . import sag_stack
        x, edge_index = data.x, data.edge_index
        if x.dim() != 2 or x.size(1) != self.convs[0].in_channels:
            return None
        g = edge_index if isinstance(edge_index, GraphBatch) else graph_of(edge_index, x.size(0), check_symmetry=True)
        if g.val is not None or not g.symmetric:
            return None
        sizes = segment_sizes(getattr(data, "batch", None), x.size(0))
        if int(sizes.max()) > int(nat.lib().tsgnn_sag_pool_graph_max_nodes()):
            return None
        return g, sag_stack.SagPlan.get(sizes, self.pooling_ratio, x.device, depth=3)

    def forward(self, data):
        route = self.fused_route(data)
        if route is not None:
            from . import sag_stack_sage
            g, plan = route
            params, perms = [], []
            for conv, pool in zip(self.convs, self.pools):
                params += [conv.lin_l.weight, conv.lin_l.bias, conv.lin_r.weight, pool.gnn.lin_l.weight, pool.gnn.lin_l.bias,
                           pool.gnn.lin_r.weight]
            out = sag_stack_sage.sag_sage_stack(data.x, g, plan, params, scorer="graphconv", perms_out=perms)
            self._perms, self._perms_fused = None, perms
        else:
            out = self._levels_composed(data)
        if mp.mlp3_ok(out, self.lin1, self.lin2, self.lin3):
            return mp.mlp3_log_softmax(out, self.lin1, self.lin2, self.lin3, self.dropout_ratio, self.training)
        h = relu(mp.linear_oi(out, self.lin1.weight, self.lin1.bias))
        h = torch.nn.functional.dropout(h, p=self.dropout_ratio, training=self.training)
        h = relu(mp.linear_oi(h, self.lin2.weight, self.lin2.bias))
        return torch.nn.functional.log_softmax(mp.linear_oi(h, self.lin3.weight, self.lin3.bias), dim=-1)

    def _levels_composed(self, data):
        x, edge_index = data.x, data.edge_index
        batch = getattr(data, "batch", None)
        if batch is None:
            batch = torch.zeros(x.size(0), dtype=torch.int64, device=x.device)
        out, perms = None, []
        for conv, pool in zip(self.convs, self.pools):
            x = relu(conv(x, edge_index))
            x, edge_index, _, batch, perm, _ = pool(x, edge_index, None, batch)
            perms.append(perm)
            r = torch.cat([global_max_pool(x, batch), global_mean_pool(x, batch)], dim=1)
            out = r if out is None else out + r
        self.last_perms = perms
        return out
