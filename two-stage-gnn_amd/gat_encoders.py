"""Drop-in modules for the reference's dense GAT (Code/sage+gat+diffpool/encoders_GAT.py:11-209).

Same class names / ctor signatures / parameter names (``w[Fin,Fout]``, ``a[2*Fout,1]``, heads registered as
``attention_{i}``) so state_dicts interchange; the O(N^2 F) pair tensor and dense attention matrix are
replaced by per-edge kernels (attention.py).  Bug-compatible with the reference where it is runnable:
  * softmax over dim=1 = per source column (T3), all-masked columns uniform 1/N;
  * ``input[0]``: every graph of a batch uses graph 0's features (T4) — meaningful at B=1 only;
  * DGATLayer's ctor in the reference dies on an undefined name (encoders_GAT.py:65); the loop it guards
    would re-initialise nothing, so it is simply omitted here.
``DGATEncoderGraph(..., per_graph_features=True)`` (extension, default off) gives every graph of a batch its OWN
features: one batched forward then equals B independent B = 1 reference forwards (the reference's GAT batch size,
train.py:480) in outputs and summed gradients, and the per-edge kernels run once on the block-diagonal batch.  With
``batch_num_nodes`` that batch is packed: n_b real rows per graph plus ONE representative of its Nmax - n_b padded rows
(``GraphBatch.from_dense_ghost1``) — padded rows have no edges and there are no per-slot statistics in this model, so
they are identical in every layer; as all-masked softmax columns they add (Nmax - n_b) / Nmax * h_ghost to every row
of their graph, which is the only place their multiplicity enters (forward weight and backward scale).
"""
import weakref

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from . import attention as att
from . import gat_fused as gf
from . import _native as nat
from . import message_passing as mp
from .dense_encoders import GraphConv, _batch_from_dense, _default_device
from .graph import GraphBatch


_ghost1_cache = {}
_eye_cache = {}
FUSED_HEAD = True


def _padded_batch(adj):
    return adj if isinstance(adj, GraphBatch) else _batch_from_dense(adj, None, "padded")


def _rows_of_graph0(x, g):
    """the reference uses input[0] for every graph (encoders_GAT.py:32): rows of graph 0, repeated."""
    if x.dim() == 3:
        x0 = x[0]
    else:
        x0 = x[: g.nmax]
    return x0.contiguous().float()


class DGATHead(nn.Module):
    per_graph_features = False          # False: encoders_GAT.py:32's input[0] for every graph (T4)

    def __init__(self, input_dim, output_dim, add_self=False, dropout=0.0, neg_input_slope=0.2, concat=True):
        super().__init__()
        self.dropout = dropout
        self.input_dim = input_dim
        self.output_dim = output_dim
        self.leakyRELU_neg_input_slope = neg_input_slope
        self.concat = concat
        dev = _default_device()
        self.w = nn.Parameter(torch.zeros(input_dim, output_dim, device=dev))
        nn.init.xavier_uniform_(self.w.data, gain=1.414)
        self.a = nn.Parameter(torch.zeros(2 * output_dim, 1, device=dev))
        nn.init.xavier_uniform_(self.a.data, gain=1.414)

    def forward(self, input, adj):
        return _gat_heads_forward([self], input, adj, concat_heads=True, elu=self.concat)


class _CatHeadWeights(torch.autograd.Function):
    """[W_0 | W_1 | ...] of a layer's heads.  The autograd of torch.cat hands every head a strided column slice that
    AccumulateGrad then clones one by one; here the backward splits the fused gradient into ONE [H, Fin, Fo] buffer (a single
    launch) and returns its contiguous per-head slices."""

    @staticmethod
    def forward(ctx, *ws):
        ctx.shape = (len(ws), ws[0].size(0), ws[0].size(1))
        return torch.cat(ws, dim=1) if len(ws) > 1 else ws[0].contiguous()

    @staticmethod
    def backward(ctx, dW):
        H, Fin, Fo = ctx.shape
        if H == 1:
            return (dW,)
        g = dW.reshape(Fin, H, Fo).permute(1, 0, 2).contiguous()          # one copy kernel for all heads
        return tuple(g[h] for h in range(H))


class _StackHeadVectors(torch.autograd.Function):
    """a_h [2*Fo, 1] of every head -> (a_row [H, Fo], a_col [H, Fo]) (encoders_GAT.py:34-36: a1 . h_i + a2 . h_j), with a
    backward that builds all heads' gradients in one launch."""

    @staticmethod
    def forward(ctx, *as_):
        H, Fo = len(as_), as_[0].size(0) // 2
        if H > 1:
            A = torch.cat(as_, dim=1).reshape(2, Fo, H).permute(0, 2, 1).contiguous()          # [2, H, Fo]: both halves contiguous
        else:
            A = as_[0].reshape(2, 1, Fo)
        ctx.shape = (H, Fo)
        return A[0], A[1]

    @staticmethod
    def backward(ctx, da_row, da_col):
        H, Fo = ctx.shape
        z = None
        if da_row is None or da_col is None:
            z = torch.zeros(H, Fo, dtype=torch.float32, device=(da_row if da_row is not None else da_col).device)
        G = torch.cat([da_row if da_row is not None else z, da_col if da_col is not None else z], dim=1)   # [H, 2*Fo]
        return tuple(G[h].reshape(2 * Fo, 1) for h in range(H))


class _PackHeads(torch.autograd.Function):
    """(w_0.., a_0..) of a layer's heads -> (W [Fin, H*Fo], a_row [H, Fo], a_col [H, Fo]) in ONE launch, and all 2H parameter
    gradients from ONE launch backward (cat / permute / copy per tensor kind otherwise: five launches per layer and step)."""

    @staticmethod
    def forward(ctx, *params):
        H = len(params) // 2
        ws, as_ = params[:H], params[H:]
        Fin, Fo = ws[0].size(0), ws[0].size(1)
        dev = ws[0].device
        W = torch.empty(Fin, H * Fo, dtype=torch.float32, device=dev)
        A = torch.empty(2, H, Fo, dtype=torch.float32, device=dev)
        pad = [None] * (8 - H)
        nat.call("pack_heads_f32", *[w.contiguous() for w in ws], *pad, *[a.contiguous() for a in as_], *pad, H, Fin, Fo, W, A)
        ctx.shape = (H, Fin, Fo)
        return W, A[0], A[1]

    @staticmethod
    def backward(ctx, dW, da_row, da_col):
        H, Fin, Fo = ctx.shape
        ref = next(t for t in (dW, da_row, da_col) if t is not None)
        gw = torch.empty(H, Fin, Fo, dtype=torch.float32, device=ref.device)
        ga = torch.empty(H, 2 * Fo, dtype=torch.float32, device=ref.device)
        nat.call("unpack_heads_f32", dW.contiguous() if dW is not None else None,
                 da_row.contiguous() if da_row is not None else None, da_col.contiguous() if da_col is not None else None,
                 H, Fin, Fo, gw, ga)
        return tuple(gw[h] for h in range(H)) + tuple(ga[h].reshape(2 * Fo, 1) for h in range(H))


PACK_HEADS = True


def _own_features(heads, g):
    ragged = getattr(g, "row_mult", None) is not None
    return ragged or (heads[0].per_graph_features and g.B > 1)


def _fused_layer_ok(heads, g, rows):
    """this layer runs on the fused kernels (gat_fused.py): supported head shape, every graph reads its own rows, the batch's
    edge-less columns can be listed"""
    if not gf.heads_ok(heads) or not (g.B == 1 or _own_features(heads, g)):
        return False
    drop_on = heads[0].dropout > 0 and heads[0].training
    return gf.batch_ok(g, rows, len(heads), drop_on)


def _gat_heads_forward(heads, x, adj, concat_heads, elu, wp=None, readout=False):
    """all heads of a layer in one pass: h = x0 [W_0|W_1|...], one edge-softmax / aggregation launch set.
    wp: this layer's packed operand when the caller packed several layers in one launch (gat_fused.pack_layers).
    readout: the caller only wants the max readout of the output over each graph's rows (the last layer, :189); returned as
    (tensor, True) when the fused layer made it inside its own node, (node output, False) otherwise."""
    g = _padded_batch(adj)
    B, N = g.B, g.nmax
    H = len(heads)
    Fo = heads[0].output_dim
    slope = heads[0].leakyRELU_neg_input_slope
    ragged = getattr(g, "row_mult", None) is not None          # packed rows + one ghost representative per graph
    if ragged and not heads[0].per_graph_features and B > 1:
        raise ValueError("the packed GAT batch needs per_graph_features=True (or B = 1)")
    own = ragged or (heads[0].per_graph_features and B > 1)
    if ragged:
        x0 = x.contiguous().float()                            # [rows, Fin]
    else:
        x0 = x.reshape(B * N, -1).contiguous().float() if own else _rows_of_graph0(x, g)  # [N, Fin] ([B*N, Fin] per-graph)
    if x0.size(1) % 4 and not x0.requires_grad:
        x0 = F.pad(x0, (0, 4 - x0.size(1) % 4))                            # 16-byte rows: the MFMA row-panel product applies
    p = heads[0].dropout
    drop_on = p > 0 and heads[0].training
    if (x0.stride(0) % 4 == 0 and x0.data_ptr() % 16 == 0 and x0.size(1) >= heads[0].input_dim
            and _fused_layer_ok(heads, g, x0.size(0))):
        if wp is None:
            (wp,) = gf.pack_layers([heads])
        if readout and gf.readout_ok(g, x0.size(0)):
            return gf.gat_layer(x0, wp, g, H, Fo, slope, mean_heads=not concat_heads, apply_elu=elu, drop_p=p if drop_on else 0.0,
                                readout=True), True
        y = gf.gat_layer(x0, wp, g, H, Fo, slope, mean_heads=not concat_heads, apply_elu=elu, drop_p=p if drop_on else 0.0)
        y = y if ragged else y.reshape(B, N, -1)
        return (y, False) if readout else y
    if drop_on:
        raise NotImplementedError("attention dropout > 0 needs the fused layer kernels (gat_fused.py): supported head shape, "
                                  "per-graph features (or B = 1), un-packed rows")
    if PACK_HEADS and 1 < H <= 8 and heads[0].w.is_cuda:
        W, a_row, a_col = _PackHeads.apply(*[hd.w for hd in heads], *[hd.a for hd in heads])
    else:
        W = _CatHeadWeights.apply(*[hd.w for hd in heads])                  # [Fin, H*Fo]
        a_row, a_col = _StackHeadVectors.apply(*[hd.a for hd in heads])    # a1 . h_i (row index i), a2 . h_j (column index j)
    h = mp.linear_l2norm(x0, W, None, normalize=False)                      # [N, H*Fo]
    if B > 1 and not own:
        h = h.unsqueeze(0).expand(B, N, H * Fo).reshape(B * N, H * Fo)       # T4: graph 0's features everywhere
    pre = att.attention_aggregate(h, a_row, a_col, g, H, slope, by_column=True, uniform_isolated=True)
    out = att.elu_heads(pre, H, mean_heads=not concat_heads, apply_elu=elu)
    out = out if ragged else out.reshape(B, N, -1)
    return (out, False) if readout else out


class DGATLayer(nn.Module):
    def __init__(self, input_dim, output_dim, dropout=0.0, neg_input_slope=0.2, n_heads=4, concat=True):
        super().__init__()
        self.dropout = dropout
        self.concat = concat
        self.n_heads = n_heads
        self.attentions = [DGATHead(input_dim, output_dim, dropout=dropout, neg_input_slope=neg_input_slope,
                                    concat=self.concat) for _ in range(n_heads)]
        for i, attention in enumerate(self.attentions):
            self.add_module("attention_{}".format(i), attention)

    def forward(self, x, adj, wp=None, readout=False):
        if self.dropout > 0 and self.training:
            x = F.dropout(x, self.dropout, training=True)
        # concat: per-head ELU then concatenation (:75); otherwise mean over heads then ELU (:78-83)
        return _gat_heads_forward(self.attentions, x, adj, concat_heads=self.concat, elu=True, wp=wp, readout=readout)


class DGATEncoderGraph(nn.Module):
    def __init__(self, input_dim, hidden_dim, embedding_dim, label_dim, args, num_layers=2, num_heads=[2, 2],
                 pred_hidden_dims=[], neg_input_slopes=[0.2, 0.2], dropouts=[0.0, 0.0], final_dim="output_dim", concat=True,
                 per_graph_features=False):
        super().__init__()
        self.dropout = dropouts
        self.bias = True
        self.num_layers = num_layers
        self.num_aggs = 1
        self.final_dim = final_dim
        self.label_dim = label_dim
        self.conv_first, self.conv_block, self.conv_last = self.build_conv_layers(
            input_dim, hidden_dim, embedding_dim, num_layers, num_heads, neg_input_slopes, dropouts)
        self.pred_input_dim = embedding_dim
        self.pred_model = self.build_pred_layers(self.pred_input_dim, label_dim, num_aggs=self.num_aggs)
        self.map_model = self.build_pred_layers(self.pred_input_dim, embedding_dim, num_aggs=self.num_aggs)
        self.map2_model = torch.nn.Identity()
        for m in self.modules():
            if isinstance(m, DGATHead):
                m.per_graph_features = bool(per_graph_features)
        self.to(_default_device())

    def build_conv_layers(self, input_dim, hidden_dim, embedding_dim, num_layers, num_heads, neg_input_slopes, dropouts):
        conv_first = DGATLayer(input_dim=input_dim, output_dim=hidden_dim, n_heads=num_heads[0], dropout=dropouts[0], concat=True)
        if num_layers >= 3:
            conv_block = nn.ModuleList(
                [DGATLayer(input_dim=hidden_dim * num_heads[i - 1], output_dim=hidden_dim, n_heads=num_heads[i],
                           dropout=dropouts[i], concat=True) for i in range(1, num_layers - 1)])
        else:
            conv_block = None
        conv_last = DGATLayer(input_dim=hidden_dim * num_heads[-1], output_dim=embedding_dim, n_heads=num_heads[-1],
                              dropout=dropouts[-1], concat=False)
        return conv_first, conv_block, conv_last

    def build_assign_conv_layers(self, input_dim, hidden_dim, embedding_dim, num_layers, add_self, normalize=False, dropout=0.0):
        conv_first = GraphConv(input_dim=input_dim, output_dim=hidden_dim, add_self=add_self, normalize_embedding=normalize)
        conv_block = nn.ModuleList([GraphConv(input_dim=hidden_dim, output_dim=hidden_dim, add_self=add_self,
                                              normalize_embedding=normalize, dropout=dropout) for _ in range(num_layers - 2)])
        conv_last = GraphConv(input_dim=hidden_dim, output_dim=embedding_dim, add_self=add_self, normalize_embedding=normalize)
        return conv_first, conv_block, conv_last

    def build_pred_layers(self, pred_input_dim, label_dim, num_aggs=1):
        return nn.Linear(pred_input_dim * num_aggs, label_dim)

    def gcn_forward(self, x, adj, conv_first, conv_block, conv_last, readout=False):
        """readout: returns (tensor, made) — the max readout of the last layer's output when its fused node made it (made = True),
        the node output otherwise"""
        g = _padded_batch(adj)
        layers = [conv_first] + (list(conv_block) if conv_block is not None else []) + [conv_last]
        wps = [None] * len(layers)
        rows = x.size(0) if x.dim() == 2 else (x.size(0) * x.size(1) if _own_features(conv_first.attentions, g) else x.size(1))
        if len(layers) <= 4 and all(isinstance(l, DGATLayer) and _fused_layer_ok(l.attentions, g, rows) for l in layers):
            wps = gf.pack_layers([l.attentions for l in layers])        # the parameters of every layer: one launch each way
        made = False
        for k, (layer, wp) in enumerate(zip(layers, wps)):
            if readout and k == len(layers) - 1 and isinstance(layer, DGATLayer):
                x, made = layer(x, g, wp=wp, readout=True)
            else:
                x = layer(x, g, wp=wp) if isinstance(layer, DGATLayer) else layer(x, g)
        return (x, made) if readout else x

    def packed_batch(self, x, adj, batch_num_nodes):
        """(rows, GraphBatch) of the packed block-diagonal batch (per_graph_features mode): dense adj [B,Nmax,Nmax] -> CSR
        over n_b + 1 rows per graph, cached per adj tensor; x [B,Nmax,F] -> those rows."""
        sizes = np.asarray(batch_num_nodes, dtype=np.int64).reshape(-1)
        key = (adj.data_ptr(), tuple(adj.shape), adj._version, tuple(int(v) for v in sizes))
        hit = _ghost1_cache.get(key)
        if hit is not None and hit[0]() is adj:
            g = hit[1]
        else:
            g = GraphBatch.from_dense_ghost1(adj.detach(), sizes)
            g.transpose_map()
            if len(_ghost1_cache) > 8:
                _ghost1_cache.clear()
            _ghost1_cache[key] = (weakref.ref(adj), g)
        F_in = x.size(2)
        return mp.pack_rows(x, g, (F_in + 3) // 4 * 4), g

    def forward(self, x, adj, batch_num_nodes=None, **kwargs):
        drop_on = self.training and any(hd.dropout > 0 for hd in self.modules() if isinstance(hd, DGATHead))
        # packed rows + one representative of each graph's padded rows: every graph must read its OWN features — the
        # per_graph_features extension, or B = 1 (the reference's GAT batch size, train.py:480), where input[0] IS the graph's own
        if (self.conv_first.attentions[0].per_graph_features or (torch.is_tensor(adj) and adj.size(0) == 1)) \
                and batch_num_nodes is not None and not isinstance(adj, GraphBatch) \
                and not drop_on:                          # (attention dropout makes a graph's padded rows differ: no packing)
            x, adj = self.packed_batch(x, adj, batch_num_nodes)
        g = _padded_batch(adj)
        x, made = self.gcn_forward(x, g, self.conv_first, self.conv_block, self.conv_last, readout=True)   # [B,N,E] ([rows,E] packed)
        if not made:                                           # (else: the last layer's node made the readout itself)
            if x.dim() == 3:
                x = x.reshape(g.B * g.nmax, x.size(2))
            x = mp.readout_max(x, g)                                                        # max over ALL padded rows (:189)
        return x, self.head(x)

    def head(self, x):
        """readouts [B, E] -> the second output of forward (encoders_GAT.py:191-198)"""
        lin1 = self.pred_model if self.final_dim != "output_dim" else self.map_model
        if mp.head2_ok(x, lin1, self.map2_model):
            return mp.head2(x, lin1, self.map2_model)[1]                                # both nn.Linear: one launch each way
        if FUSED_HEAD and isinstance(self.map2_model, torch.nn.Identity) and isinstance(lin1, nn.Linear) and x.is_cuda \
                and x.size(1) % 4 == 0 and x.size(0) <= 1024 and lin1.out_features <= 256 and lin1.weight.data_ptr() % 16 == 0:
            # map2_model is Identity (:117): the two-Linear head kernels with W2 = I (1 * v + 0 * u is exact) — one launch each way,
            # the cross-entropy folded into the backward, instead of three library GEMMs + a bias reduction
            C = lin1.out_features
            eye = _eye_cache.get((C, x.device))
            if eye is None:
                eye = _eye_cache[(C, x.device)] = torch.eye(C, dtype=torch.float32, device=x.device)
            y = mp._Head2.apply(x, lin1.weight, lin1.bias, eye, None)[1]
            y._tsgnn_defer_ce = True          # (under FlatTrainer(defer_loss=True) / mp.deferred_loss(): mp._SoftmaxCE)
            return y
        return self.map2_model(lin1(x))

    def loss(self, pred, label, type="softmax"):
        if type == "softmax":
            return mp.cross_entropy(pred, label)
        if type == "margin":
            onehot = torch.zeros(pred.size(0), self.label_dim, dtype=torch.long, device=pred.device)
            onehot.scatter_(1, label.view(-1, 1), 1)
            return torch.nn.MultiLabelMarginLoss()(pred, onehot)
        raise ValueError(type)
