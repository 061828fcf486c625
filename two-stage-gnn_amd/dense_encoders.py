"""Drop-in modules for the reference's dense-batched encoders (Code/sage+gat+diffpool/encoders.py).

Same class names, constructor signatures, parameter names/shapes (``weight[Fin,Fout]``, ``bias[Fout]``,
``conv_first`` / ``conv_block`` / ``conv_last`` / ``pred_model`` …, so ``state_dict``s interchange) and call
signatures as the reference, so its scaffolding (train.py:253-260,121; tripletnet.py:36-38) can construct
and call them unchanged.  Internally nothing is dense: the adjacency becomes a CSR ``GraphBatch`` and every
tensor op on the message-passing path is a HIP kernel behind include/tsgnn.h.

Accepted inputs of ``forward(x, adj, batch_num_nodes)``:
  * the reference's tensors ``x[B,Nmax,F]``, ``adj[B,Nmax,Nmax]`` (dense -> CSR conversion on the GPU), or
  * a prebuilt ``GraphBatch`` as ``adj`` with ``x`` either padded ``[B,Nmax,F]`` or already in rows.
"""
import os
import weakref

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from . import message_passing as mp
from .graph import GraphBatch


def _default_device():
    return torch.device("cuda", torch.cuda.current_device()) if torch.cuda.is_available() else torch.device("cpu")


# dense adj tensor -> GraphBatch cache (the three conv layers of an encoder share one conversion)
_csr_cache = {}


def _batch_from_dense(adj, sizes, layout):
    key = (adj.data_ptr(), tuple(adj.shape), adj._version, layout,
           None if sizes is None else tuple(int(s) for s in np.asarray(sizes).reshape(-1)))
    hit = _csr_cache.get(key)
    if hit is not None and hit[0]() is adj:
        return hit[1]
    g = GraphBatch.from_dense(adj.detach(), sizes=sizes, layout=layout)
    if len(_csr_cache) > 8:
        _csr_cache.clear()
    _csr_cache[key] = (weakref.ref(adj), g)
    return g


FUSED_HEAD = True              # the two chained nn.Linear after the readout as one HIP launch (+1 backward)
FUSED_DENSE_STACK = True    # pooled DiffPool levels: the whole GCN stack as one autograd node (dense_stack.py)
# DiffPool: the readout of embeddings that a contraction reads too is made inside the contraction's node (no backward pass of its own);
# off: by a node of its own that passes the embeddings through, so that one backward pass sums both gradients (mp._ReadoutMax)
READOUT_IN_CONTRACT = os.environ.get("TSGNN_READOUT_IN_CONTRACT", "1") != "0"
SOFTMAX_IN_CONTRACT = os.environ.get("TSGNN_SOFTMAX_IN_CONTRACT", "1") != "0"   # pooled levels: the assignment softmax inside the contraction's launches
READOUT_COLUMNS = os.environ.get("TSGNN_READOUT_COLUMNS", "1") != "0"   # DiffPool: the levels' readouts written into one buffer (no cat)
FUSED_STACK = True             # GcnEncoderGraph: run the conv stack as one fused autograd node when it qualifies
PER_GRAPH_STACK = os.environ.get("TSGNN_PER_GRAPH_STACK", "1") != "0"   # ... also with per-graph statistics (the triplet step)
PER_GRAPH_DENSE = os.environ.get("TSGNN_PER_GRAPH_DENSE", "1") != "0"   # pooled DiffPool levels under per-graph statistics: one launch per layer (dense_stack_pg.py)
DENSE_ADJ_MAX_NODES = 128      # at or below this many nodes per graph a dense batched MFMA product is used


def _stack(first, block, last):
    """a conv stack as a list, input layer first (the encoders keep the reference's conv_first / conv_block / conv_last attributes)"""
    return [first, *block, last]


def per_graph_node_ok(g, convs):
    """may the fused GraphSage node (sage_stack) run the stack ``convs`` under per-graph statistics on batch ``g``?"""
    # Its row-local launches take a batch whose rows know their graph and which carries every ghost-slot row.  The width bound is the
    # one of tsgnn_row_post_bwd_f32 / tsgnn_row_post_nodes_bwd_f32 (csrc/bn_readout.hip refuses F > 256); sage_stack.eligible, which
    # every caller asks as well, stops at 128 columns, so the bound never decides.  (The PER_GRAPH_STACK switch is for the encoders to
    # consult: a stream's batch either has the shape or not.)
    return g.row_graph is not None and g.n_ghost == g.nmax and convs[0].output_dim <= 256


class _Readouts:
    """the max readouts of an encoder's layers or levels, asked for one by one (``of``) in the order of their concatenation"""
    # (READOUT_COLUMNS: they land in their column blocks of ONE buffer: no torch.cat launch, no slice copies backwards)

    def __init__(self, B, width, device, concat):
        self.concat = concat
        self.cols = mp.ReadoutColumns(B, width, device) if (concat and READOUT_COLUMNS) else None
        self.out = []

    def of(self, x, g, shared=False, ghost_unused=False):
        """the readout of the rows ``x`` on batch ``g`` -> (x, request): the one place that picks the readout's route"""
        # shared: a DiffPool contraction reads x next.  Then the contraction makes the readout, as a third output of its node, and adds
        # the readout's gradient inside the launch that produces the embeddings' gradient (diffpool._ContractRows / _ContractDense):
        # request = (into,), the column block to hand it, and the caller appends what comes back to `out`.  READOUT_IN_CONTRACT off:
        # a pass-through node makes it here, the contraction reads the x returned.  Not shared: a plain readout_max.  request is None
        # wherever the readout is made here.
        into = self.cols and self.cols.take(x.size(1))
        if shared and READOUT_IN_CONTRACT:
            return x, (into,)
        if shared:
            ro, x = mp.readout_max_pass(x, g, ghost_unused=ghost_unused, into=into)
        else:
            ro = mp.readout_max(x, g, into=into)
        self.out.append(ro)
        return x, None

    def joined(self):
        if not self.concat:
            return self.out[-1]
        return self.cols.join(self.out) if self.cols is not None else torch.cat(self.out, dim=1)


class _DenseBmm(torch.autograd.Function):
    """y[b] = adj[b] @ x[b] (+x) for small / differentiable dense adjacencies (pooled DiffPool levels,
    encoders.py:375-380): batched fp32 MFMA, gradients to BOTH operands."""

    @staticmethod
    def forward(ctx, adj, x, add_self):
        adj = adj.contiguous()
        x = x.contiguous()
        B, N, Fd = x.shape
        y = x.clone() if add_self else torch.empty_like(x)
        mp.gemm(adj, N, 1, x, Fd, 1, y, Fd, 1, N, Fd, N, batch=B, stride_a=N * N, stride_b=N * Fd, stride_c=N * Fd,
                accumulate=add_self)
        ctx.save_for_backward(adj, x)
        ctx.add_self = add_self
        return y

    @staticmethod
    def backward(ctx, dy):
        adj, x = ctx.saved_tensors
        dy = dy.contiguous()
        B, N, Fd = x.shape
        dadj = dx = None
        if ctx.needs_input_grad[0]:      # dA[b] = dY[b] x[b]^T
            dadj = torch.empty_like(adj)
            mp.gemm(dy, Fd, 1, x, 1, Fd, dadj, N, 1, N, N, Fd, batch=B, stride_a=N * Fd, stride_b=N * Fd, stride_c=N * N)
        if ctx.needs_input_grad[1]:      # dx[b] = A[b]^T dY[b] (+dY)
            dx = dy.clone() if ctx.add_self else torch.empty_like(x)
            mp.gemm(adj, 1, N, dy, Fd, 1, dx, Fd, 1, N, Fd, N, batch=B, stride_a=N * N, stride_b=N * Fd, stride_c=N * Fd,
                    accumulate=ctx.add_self)
        return dadj, dx, None


class GraphConv(nn.Module):
    """Drop-in for encoders.py:13-42: y = normalize((adj@x [+x]) @ weight + bias)."""

    def __init__(self, input_dim, output_dim, add_self=False, normalize_embedding=False, dropout=0.0, bias=True):
        super().__init__()
        self.add_self = add_self
        self.dropout = dropout
        if dropout > 0.001:
            self.dropout_layer = nn.Dropout(p=dropout)
        self.normalize_embedding = normalize_embedding
        self.input_dim = input_dim
        self.output_dim = output_dim
        dev = _default_device()
        self.weight = nn.Parameter(torch.empty(input_dim, output_dim, device=dev))
        self.bias = nn.Parameter(torch.empty(output_dim, device=dev)) if bias else None
        # the reference leaves the storage uninitialised until its encoder re-initialises it
        # (encoders.py:88-92); give a stand-alone layer the same Xavier/zero init
        nn.init.xavier_uniform_(self.weight.data, gain=nn.init.calculate_gain("relu"))
        if self.bias is not None:
            nn.init.constant_(self.bias.data, 0.0)

    # rows in, rows out (the encoders' fast path)
    def forward_rows(self, x, g):
        if self.dropout > 0.001:
            x = self.dropout_layer(x)
        z = mp.aggregate(x, g, add_self=self.add_self)
        return mp.linear_l2norm(z, self.weight, self.bias, normalize=self.normalize_embedding)

    def forward(self, x, adj):
        if isinstance(adj, GraphBatch):
            if x.dim() == 2:
                return self.forward_rows(x, adj)
            return mp.unpack_rows(self.forward_rows(mp.pack_rows(x, adj), adj), adj)
        if x.dim() != 3 or adj.dim() != 3:
            raise ValueError("GraphConv expects x[B,N,F] and adj[B,N,N]")
        B, N, Fin = x.shape
        if adj.requires_grad or N <= DENSE_ADJ_MAX_NODES:
            if self.dropout > 0.001:
                x = self.dropout_layer(x)
            y = _DenseBmm.apply(adj.float(), x.float(), self.add_self)
            v = mp.linear_l2norm(y.reshape(B * N, Fin), self.weight, self.bias, normalize=self.normalize_embedding)
            return v.reshape(B, N, self.output_dim)
        g = _batch_from_dense(adj, None, "padded")
        return self.forward_rows(x.contiguous().float().reshape(B * N, Fin), g).reshape(B, N, self.output_dim)


class GcnEncoderGraph(nn.Module):
    """Drop-in for encoders.py:45-229 (the repo's "GraphSage"/base encoder)."""

    def __init__(self, input_dim, hidden_dim, embedding_dim, label_dim, num_layers, pred_hidden_dims=[],
                 concat=True, bn=True, dropout=0.0, args=None, final_dim="output_dim"):
        super().__init__()
        self.concat = concat
        add_self = not concat
        self.bn = bn
        self.num_layers = num_layers
        self.num_aggs = 1
        self.final_dim = final_dim
        self.bias = True
        if args is not None:
            self.bias = args.bias
        self.conv_first, self.conv_block, self.conv_last = self.build_conv_layers(
            input_dim, hidden_dim, embedding_dim, num_layers, add_self, normalize=True, dropout=dropout)
        self.act = nn.ReLU()
        self.label_dim = label_dim
        self.pred_input_dim = hidden_dim * (num_layers - 1) + embedding_dim if concat else embedding_dim
        self.pre_pred_model = self.build_pred_layers(self.pred_input_dim, pred_hidden_dims, embedding_dim,
                                                     num_aggs=self.num_aggs)
        self.pred_model = self.build_pred_layers(embedding_dim, pred_hidden_dims, label_dim, num_aggs=self.num_aggs)
        self.map_model = self.build_pred_layers(self.pred_input_dim, pred_hidden_dims, embedding_dim,
                                                num_aggs=self.num_aggs)
        self.map2_model = self.build_pred_layers(pred_input_dim=embedding_dim, pred_hidden_dims=[], label_dim=2)
        # True: each graph of a batch is normalised with the statistics it would have at B = 1 (triplet settings)
        self.per_graph_bn = False
        self._init_convs()
        self.to(_default_device())

    def _init_convs(self):
        for m in self.modules():
            if isinstance(m, GraphConv):
                nn.init.xavier_uniform_(m.weight.data, gain=nn.init.calculate_gain("relu"))
                if m.bias is not None:
                    nn.init.constant_(m.bias.data, 0.0)

    def build_conv_layers(self, input_dim, hidden_dim, embedding_dim, num_layers, add_self, normalize=False,
                          dropout=0.0):
        conv_first = GraphConv(input_dim=input_dim, output_dim=hidden_dim, add_self=add_self,
                               normalize_embedding=normalize, bias=self.bias)
        conv_block = nn.ModuleList(
            [GraphConv(input_dim=hidden_dim, output_dim=hidden_dim, add_self=add_self, normalize_embedding=normalize,
                       dropout=dropout, bias=self.bias) for _ in range(num_layers - 2)])
        conv_last = GraphConv(input_dim=hidden_dim, output_dim=embedding_dim, add_self=add_self,
                              normalize_embedding=normalize, bias=self.bias)
        return conv_first, conv_block, conv_last

    def build_pred_layers(self, pred_input_dim, pred_hidden_dims, label_dim, num_aggs=1):
        pred_input_dim = pred_input_dim * num_aggs
        if len(pred_hidden_dims) == 0:
            return nn.Linear(pred_input_dim, label_dim)
        layers = []
        for pred_dim in pred_hidden_dims:
            layers.append(nn.Linear(pred_input_dim, pred_dim))
            layers.append(self.act)
            pred_input_dim = pred_dim
        layers.append(nn.Linear(pred_dim, label_dim))
        return nn.Sequential(*layers)

    def construct_mask(self, max_nodes, batch_num_nodes):
        """[B, max_nodes, 1] prefix mask (encoders.py:121-132), built without a python loop."""
        n = torch.as_tensor(np.asarray(batch_num_nodes, dtype=np.int64), device=_default_device())
        return (torch.arange(max_nodes, device=n.device)[None, :] < n[:, None]).float().unsqueeze(2)

    def apply_bn(self, x):
        """Per-node-slot batch norm of a padded [B,N,F] tensor (encoders.py:134-138)."""
        B, N, Fd = x.shape
        g = GraphBatch.uniform(B, N, x.device)
        return mp.bn_slots(x.contiguous().float().reshape(B * N, Fd), g, relu=False, bn=True).reshape(B, N, Fd)

    # ------------------------------------------------------------------ graph batch plumbing
    @staticmethod
    def make_batch(x, adj, batch_num_nodes):
        """-> (rows, GraphBatch).  With node counts: packed rows + ghost-slot rows; without: padded rows."""
        if isinstance(adj, GraphBatch):
            g = adj
        elif batch_num_nodes is not None:
            g = _batch_from_dense(adj, np.asarray(batch_num_nodes).reshape(-1), "packed")
        else:
            g = _batch_from_dense(adj, None, "padded")
        if x.dim() == 3:
            F_in = x.size(2)
            ld = (F_in + 3) // 4 * 4 if g.layout == "packed" else None      # 16-B rows for the float4 gather
            x = mp.pack_rows(x, g, ld)
        return x, g

    def _post(self, v, g):
        """ReLU then (optionally) slot batch-norm: encoders.py:179-181."""
        return mp.bn_slots(v, g, relu=True, bn=self.bn, per_graph=self.per_graph_bn)

    def conv_stack(self, level=0):
        """the conv stack as a list; ``level`` >= 1, in the encoders that pool: the embedding stack after the level-th pooling"""
        if level == 0:
            return _stack(self.conv_first, self.conv_block, self.conv_last)
        i = level - 1
        return _stack(self.conv_first_after_pool[i], self.conv_block_after_pool[i], self.conv_last_after_pool[i])

    def gcn_forward_rows(self, x, g, conv_first, conv_block, conv_last, mask_ghost=False, per_graph_stack=False):
        """gcn_forward (encoders.py:140-167) on rows, with the reference's signature; see ``_gcn_rows``"""
        return self._gcn_rows(x, g, _stack(conv_first, conv_block, conv_last), mask_ghost, per_graph_stack)

    def _gcn_rows(self, x, g, convs, mask_ghost=False, per_graph_stack=False):
        """per-layer outputs of the stack ``convs`` concatenated on the feature axis"""
        # mask_ghost = multiply by the embedding mask (zeroes every ghost row).  per_graph_stack: the caller allows the fused node under
        # per-graph statistics too.
        # the fused node: slot statistics, or — where the caller allows it — the per-graph statistics of the triplet step (masked
        # output on a batch with its full set of ghost-slot rows: the row-local launches tsgnn_row_ln_fwd_f32 /
        # tsgnn_row_post_nodes_bwd_f32 in place of the slot ones)
        per_graph = bool(self.per_graph_bn)
        allowed = (mask_ghost or not g.n_ghost) if not per_graph else \
            (per_graph_stack and PER_GRAPH_STACK and mask_ghost and per_graph_node_ok(g, convs))
        if FUSED_STACK and allowed:
            from . import sage_stack
            if sage_stack.eligible(g, convs, self.bn, x):
                with sage_stack.per_graph_stats(per_graph):
                    return sage_stack.sage_stack_nodes(x, g, convs, mask_ghost)     # one autograd node, layers write into the cat
        x_all = []
        for conv in convs[:-1]:
            x = self._post(conv.forward_rows(x, g), g)
            x_all.append(x)
        x_all.append(convs[-1].forward_rows(x, g))
        t = torch.cat(x_all, dim=1)
        if mask_ghost and g.n_ghost:
            t = mp.mask_ghost_rows(t, g)
        return t

    def readouts_rows(self, x, g):
        """encoders.py:177-205 up to the concatenated max readout."""
        from . import sage_stack
        convs = self.conv_stack()
        if self.concat and FUSED_STACK and sage_stack.eligible(g, convs, self.bn, x) and \
                (not self.per_graph_bn or (PER_GRAPH_STACK and per_graph_node_ok(g, convs))):
            # (per-graph statistics, the triplet step: the same node with the row-local batch-norm launches, sage_stack.per_graph_stats)
            with sage_stack.per_graph_stats(self.per_graph_bn):
                return sage_stack.sage_stack_readouts(x, g, convs)
        ro = _Readouts(g.B, self.pred_input_dim, x.device, self.concat)
        for conv in convs[:-1]:
            x = self._post(conv.forward_rows(x, g), g)
            ro.of(x, g)
        ro.of(convs[-1].forward_rows(x, g), g)
        return ro.joined()

    def _head(self):
        """final_dim -> (lin1, lin2, swap): the two chained nn.Linear after the readout; swap: (lin2's output, lin1's) is returned"""
        if self.final_dim == "pretrain":          # 2stg+
            return self.map_model, self.map2_model, True
        if self.final_dim != "output_dim":        # original
            return self.pre_pred_model, self.pred_model, False
        return None                               # 2stg: the first output IS the readout

    def _ordered(self, vec, y):
        """(lin1's output, lin2's) in the order ``final_dim`` returns them"""
        return (y, vec) if self._head()[2] else (vec, y)

    def _head_linears(self):
        """the two chained nn.Linear after the readout (None where ``forward`` applies none: 2stg, and triplet.tripletnet's _defer_map)"""
        head = None if getattr(self, "_defer_map", False) else self._head()
        return head and head[:2]

    def _heads(self, output):
        head, defer = self._head(), getattr(self, "_defer_map", False)
        if head is None:             # (triplet.tripletnet applies map_model itself: embeddings + distances, one launch)
            return output, (None if defer else self.map_model(output))
        if defer and self.final_dim == "pretrain":
            return None, output      # (tripletnet reads the embedding only; it applies map_model to `output` itself)
        lin1, lin2, _ = head
        if FUSED_HEAD and mp.head2_ok(output, lin1, lin2):
            return self._ordered(*mp.head2(output, lin1, lin2))
        vec = lin1(output)
        return self._ordered(vec, lin2(vec))

    def forward(self, x, adj, batch_num_nodes=None, **kwargs):
        x, g = self.make_batch(x, adj, batch_num_nodes)
        head = self._head()
        if FUSED_HEAD and type(self) is GcnEncoderGraph and head is not None:
            from . import sage_stack
            convs, (lin1, lin2, _) = self.conv_stack(), head
            if self.concat and FUSED_STACK and not self.per_graph_bn and sage_stack.eligible(g, convs, self.bn, x) \
                    and sage_stack.head_ok(g, convs, lin1, lin2):
                # stack + readout tail + head: one autograd node
                return self._ordered(*sage_stack.sage_stack_head(x, g, convs, lin1, lin2))
        return self._heads(self.readouts_rows(x, g))

    def loss(self, pred, label, type="softmax"):
        if type == "softmax":
            return mp.cross_entropy(pred, label)
        if type == "margin":
            onehot = torch.zeros(pred.size(0), self.label_dim, dtype=torch.long, device=pred.device)
            onehot.scatter_(1, label.view(-1, 1), 1)
            return torch.nn.MultiLabelMarginLoss()(pred, onehot)
        raise ValueError(type)


class SoftPoolingGcnEncoder(GcnEncoderGraph):
    """Drop-in for encoders.py:236-441 (DiffPool).  Level 0 runs on the CSR rows of the input graphs; the
    assignment contraction X' = S^T Z, A' = S^T A S (encoders.py:374-375) is SpMM + ragged batched fp32-MFMA
    GEMMs; pooled levels (dense, differentiable adjacency) use strided batched MFMA GEMMs."""

    def __init__(self, max_num_nodes, input_dim, hidden_dim, embedding_dim, label_dim, num_layers, assign_hidden_dim,
                 assign_ratio=0.25, assign_num_layers=-1, num_pooling=1, pred_hidden_dims=[], concat=True, bn=True,
                 dropout=0.0, linkpred=True, assign_input_dim=-1, args=None, final_dim="output_dim"):
        # the reference forwards neither bn nor dropout to the base ctor (encoders.py:249-250): bn stays True
        super().__init__(input_dim, hidden_dim, embedding_dim, label_dim, num_layers, pred_hidden_dims=pred_hidden_dims,
                         concat=concat, args=args)
        add_self = not concat
        self.num_pooling = num_pooling
        self.linkpred = linkpred
        self.assign_ent = True
        self.final_dim = final_dim
        self.conv_first_after_pool = nn.ModuleList()
        self.conv_block_after_pool = nn.ModuleList()
        self.conv_last_after_pool = nn.ModuleList()
        for _ in range(num_pooling):
            c1, cb, cl = self.build_conv_layers(self.pred_input_dim, hidden_dim, embedding_dim, num_layers, add_self,
                                                normalize=True, dropout=dropout)
            self.conv_first_after_pool.append(c1)
            self.conv_block_after_pool.append(cb)
            self.conv_last_after_pool.append(cl)
        if assign_num_layers == -1:
            assign_num_layers = num_layers
        if assign_input_dim == -1:
            assign_input_dim = input_dim
        self.assign_conv_first_modules = nn.ModuleList()
        self.assign_conv_block_modules = nn.ModuleList()
        self.assign_conv_last_modules = nn.ModuleList()
        self.assign_pred_modules = nn.ModuleList()
        assign_dim = int(max_num_nodes * assign_ratio)
        for _ in range(num_pooling):
            a1, ab, al = self.build_conv_layers(assign_input_dim, assign_hidden_dim, assign_dim, assign_num_layers, add_self,
                                                normalize=True)
            assign_pred_input_dim = assign_hidden_dim * (num_layers - 1) + assign_dim if concat else assign_dim
            self.assign_pred_modules.append(self.build_pred_layers(assign_pred_input_dim, [], assign_dim, num_aggs=1))
            assign_input_dim = self.pred_input_dim
            assign_dim = int(assign_dim * assign_ratio)
            self.assign_conv_first_modules.append(a1)
            self.assign_conv_block_modules.append(ab)
            self.assign_conv_last_modules.append(al)
        self.pre_pred_model = self.build_pred_layers(self.pred_input_dim * (num_pooling + 1), pred_hidden_dims, embedding_dim,
                                                     num_aggs=self.num_aggs)
        self.pred_model = self.build_pred_layers(embedding_dim, pred_hidden_dims, label_dim, num_aggs=self.num_aggs)
        self.map_model = self.build_pred_layers(self.pred_input_dim * (num_pooling + 1), pred_hidden_dims, embedding_dim,
                                                num_aggs=self.num_aggs)
        self.map2_model = self.build_pred_layers(pred_input_dim=embedding_dim, pred_hidden_dims=[], label_dim=2)
        self._init_convs()
        self.to(_default_device())

    def assign_stack(self, level):
        """the assignment conv stack of ``level`` (0: the input graphs) as a list; its embedding stack is ``conv_stack(level)``"""
        return _stack(self.assign_conv_first_modules[level], self.assign_conv_block_modules[level], self.assign_conv_last_modules[level])

    def assign_linear(self, level):
        """the nn.Linear from the level's assignment stack output to its cluster logits"""
        return self.assign_pred_modules[level]

    def gcn_forward_dense(self, x, adj, conv_first, conv_block, conv_last):
        """gcn_forward on dense pooled tensors x[B,K,F], adj[B,K,K] (encoders.py:378-380; mask is None there) -> (cat, uniform batch)"""
        return self._gcn_dense(x, adj, _stack(conv_first, conv_block, conv_last))

    def _gcn_dense(self, x, adj, convs):
        B, K, _ = x.shape
        g = GraphBatch.uniform(B, K, x.device)
        if self.per_graph_bn and self.bn and PER_GRAPH_DENSE:
            # per-graph statistics (the triplet step, stage two): every post-op is row-local, a layer is one launch of independent tiles
            from . import dense_stack_pg
            if dense_stack_pg.eligible(x, adj, convs):
                return dense_stack_pg.dense_gcn_stack_pg(x, adj, convs), g
        if FUSED_DENSE_STACK:
            from . import dense_stack
            if dense_stack.eligible(x, adj, g, convs, self.bn, self.per_graph_bn):
                return dense_stack.dense_gcn_stack(x, adj, g, convs), g       # one autograd node, layers write into the cat

        def hidden(conv, x):
            # transform + normalise + ReLU + slot BN as one node (one launch for the BN forward, one for the backward of
            # BN + ReLU + normalise) when the fused slot kernels take the shape; else the composed ops
            if (self.bn and not self.per_graph_bn and conv.normalize_embedding and conv.dropout <= 0.001
                    and mp.linear_norm_bn_ok(g, conv.output_dim)):
                y = _DenseBmm.apply(adj.float(), x.float(), conv.add_self)
                return mp.linear_norm_bn(y.reshape(B * K, -1), conv.weight, conv.bias, g).reshape(B, K, -1)
            v = conv(x, adj).reshape(B * K, -1)
            return mp.bn_slots(v, g, relu=True, bn=self.bn, per_graph=self.per_graph_bn).reshape(B, K, -1)
        x_all = []
        for conv in convs[:-1]:
            x = hidden(conv, x)
            x_all.append(x)
        x_all.append(convs[-1](x, adj))
        return torch.cat(x_all, dim=2), g

    def _level0_pair_ok(self, x, x_a, g, masked):
        """both first-level stacks take the fused stack path (_gcn_rows) and may share launches"""
        from . import sage_stack
        if not (FUSED_STACK and sage_stack.PAIR_LAUNCHES and not self.per_graph_bn and (masked or not g.n_ghost)):
            return False
        return all(torch.is_tensor(xx) and xx.dim() == 2 and sage_stack.eligible(g, convs, self.bn, xx)
                   for xx, convs in ((x, self.conv_stack()), (x_a, self.assign_stack(0))))

    # ------------------------------------------------------------------ the stages of forward
    def _inputs(self, x, adj, batch_num_nodes, x_a):
        """1. -> (rows of x, rows of the assignment input x_a, batch, masked): packed rows (+ghost reps) if masked, else padded"""
        same_input = x_a is x
        x, g = self.make_batch(x, adj, batch_num_nodes)
        if same_input:
            x_a = x
        elif x_a.dim() == 3:
            x_a = mp.pack_rows(x_a, g, (x_a.size(2) + 3) // 4 * 4 if g.layout == "packed" else None)
        return x, x_a, g, batch_num_nodes is not None

    def _level0_stacks(self, x, x_a, g, masked):
        """2. -> (embeddings, the first assignment stack's output: None without pooling), rows on the input batch"""
        if self.num_pooling > 0 and self._level0_pair_ok(x, x_a, g, masked):
            # the embedding and the first assignment stack run on the same graph: one autograd node whose launches are shared
            # pairwise (sage_stack._SageStackPair) — each kernel of one stack alone fills about half of the CUs
            from . import sage_stack
            return sage_stack.sage_stack_nodes_pair(x, x_a, g, self.conv_stack(), self.assign_stack(0), masked)
        emb = self._gcn_rows(x, g, self.conv_stack(), mask_ghost=masked, per_graph_stack=True)
        if self.num_pooling == 0:
            return emb, None
        return emb, self._gcn_rows(x_a, g, self.assign_stack(0), mask_ghost=masked, per_graph_stack=True)

    def _pool_rows(self, a, emb, g, masked, ro):
        """3. at level 0: S = softmax(linear(a)) on the input batch's rows, X' = S^T Z, A' = S^T A S -> (X', A'); Z's readout -> ro"""
        from . import diffpool as dp
        ghost = bool(masked and g.n_ghost)
        # masked: the ghost rows of `emb` are constants (zeros), their gradient is discarded by the stack's backward
        emb, request = ro.of(emb, g, shared=True, ghost_unused=ghost)
        lin = self.assign_linear(0)
        s = dp.row_softmax(mp.linear_oi(a, lin.weight, lin.bias), g.n_rows if ghost else None)   # encoders.py:369, :371 (ghost rows -> 0)
        self.assign_tensor = s
        self._link_graph, self._link_masked = g, masked
        res = dp.diffpool_contract_rows(s, emb, g, readout=request and (ghost, *request, ghost))   # :374-375 (+ :353, the readout)
        ro.out.extend(res[2:])
        return res[0], res[1]

    def _pool_dense(self, level, x, adj, emb, a, ro):
        """3. at a pooled level >= 1 with inputs (x, adj) and embeddings emb [B, K, C]; a: the assignment stack's output, if made"""
        from . import diffpool as dp
        B, K, C = emb.shape
        rows, g = self._level_rows(emb)
        rows, request = ro.of(rows, g, shared=True)
        if a is None:
            a, _ = self._gcn_dense(x, adj, self.assign_stack(level))
        lin = self.assign_linear(level)
        logits = mp.linear_oi(a.reshape(B * K, -1), lin.weight, lin.bias)
        # SOFTMAX_IN_CONTRACT: nn.Softmax(dim=-1) (:369) on the operand the contraction stages anyway, its backward in the backward
        # launch; S comes back as the last output
        s = (logits if SOFTMAX_IN_CONTRACT else dp.row_softmax(logits)).reshape(B, K, -1)
        res = dp.diffpool_contract_dense(s, rows.reshape(B, K, C), adj, readout=request and (g, *request), softmax=SOFTMAX_IN_CONTRACT)
        self.assign_tensor = res[-1] if SOFTMAX_IN_CONTRACT else s
        if request is not None:
            ro.out.append(res[2])
        return res[0], res[1]

    def _pooled_stacks(self, level, x, adj):
        """3. the embedding stack of ``level`` >= 1 on (x, adj) -> (embeddings [B, K, C], assignment stack's output or None, adj)"""
        # (the assignment stack's output where one launch serves both stacks; adj: what the level's contraction is to read)
        convs = self.conv_stack(level)
        if level < self.num_pooling and FUSED_DENSE_STACK and self.bn and not self.per_graph_bn:
            # the embedding stack and the level's assignment stack read the same (x, adjacency): one launch forward and one
            # backward for both (dense_stack.py)
            from . import dense_stack
            stacks = [convs, self.assign_stack(level)]
            if dense_stack.ONE_LAUNCH and dense_stack.one_launch_ok(x, adj, stacks):
                # (the contraction reads the adjacency through this node's pass-through: one gradient sum, inside the stacks'
                # backward launch)
                return dense_stack.dense_gcn_stacks(x, adj, stacks, adj_pass=True)
        return self._gcn_dense(x, adj, convs)[0], None, adj

    @staticmethod
    def _level_rows(emb):
        """a pooled level's embeddings [B, K, C] -> (rows [B * K, C], their uniform batch)"""
        B, K, C = emb.shape
        return emb.reshape(B * K, C), GraphBatch.uniform(B, K, emb.device)

    def _levels_head(self, ro, rows, g):
        """4. + 5. the last level's readout (its embeddings: ``rows`` on ``g``) and the head on the levels' readouts"""
        lins = self._head_linears()
        if (self.num_pooling > 0 and self.concat and lins is not None and FUSED_HEAD and g.n_ghost == 0
                and mp.head2_tail_ok(ro.cols, rows, g.nmax, *lins)):
            # the LAST level's readout fills its column block inside the head's own launches (mp._Head2Tail)
            return self._ordered(*mp.head2_tail(ro.cols, ro.out, rows, g.nmax, *lins))
        ro.of(rows, g)
        return self._heads(ro.joined())

    def forward(self, x, adj, batch_num_nodes, **kwargs):
        x, x_a, g, masked = self._inputs(x, adj, batch_num_nodes, kwargs.get("assign_x", x))
        emb, a = self._level0_stacks(x, x_a, g, masked)
        ro = _Readouts(g.B, emb.size(1) * (self.num_pooling + 1), emb.device, self.concat)
        if self.num_pooling == 0:
            return self._levels_head(ro, emb, g)
        x_l, adj_l = self._pool_rows(a, emb, g, masked, ro)
        for level in range(1, self.num_pooling + 1):
            emb, a, adj_l = self._pooled_stacks(level, x_l, adj_l)
            if level < self.num_pooling:
                x_l, adj_l = self._pool_dense(level, x_l, adj_l, emb, a, ro)
        return self._levels_head(ro, *self._level_rows(emb))

    linkpred_clamp = 1.0        # the reference clamps pred_adj with an UNINITIALISED tensor (encoders.py:424); see DESIGN.md

    def loss(self, pred, label, adj=None, batch_num_nodes=None, adj_hop=1):
        """CE (+ the link-prediction side loss of encoders.py:416-440 when ``linkpred``).  ``adj`` / ``batch_num_nodes`` are
        accepted for signature compatibility; the adjacency and the mask used are those of the forward's batch."""
        loss = super().loss(pred, label)
        if self.linkpred:
            from . import diffpool as dp
            if self.num_pooling != 1:
                # trap T7: the reference multiplies the LAST level's assignment with the ORIGINAL adjacency (:418,428)
                raise RuntimeError("link-prediction loss with num_pooling >= 2: the last assignment tensor [B, %d, .] does not "
                                   "match the input adjacency (the reference fails with a shape error here too)"
                                   % self.assign_tensor.size(-2))
            self.link_loss = dp.link_pred_loss(self.assign_tensor, self._link_graph, self.linkpred_clamp,
                                               masked=self._link_masked, adj_hop=adj_hop)
            return loss + self.link_loss
        return loss
