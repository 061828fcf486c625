"""Drop-in modules for the reference's EigenGCN encoder (Code/eigengcn/encoders.py:248-417): ``WavePoolingGcnEncoder`` and ``Pool``.

Same class names, constructor signatures and ``state_dict`` keys (``conv_first.*``, ``conv_block.N.*``, ``conv_last.*``,
``conv_first_after_pool.i.*``, ``conv_block_after_pool.i.N.*``, ``conv_last_after_pool.i.*``, ``pred_model.*``).  The level stacks
run on the rows of a ``GraphBatch`` (dense_encoders.GcnEncoderGraph.gcn_forward_rows: the fused stack node where it qualifies); each
pooling X' = P^T Z is one launch that also writes the max readout of Z (eigen_pool.py, csrc/eigen_pool.hip).

``forward(x, adj, adj_pooled_list, batch_num_nodes, batch_num_nodes_list, pool_matrices_dic)`` takes the reference's padded tensors
(converted on the GPU, cached), or a prebuilt ``eigen_pool.EigenBatch`` as ``adj`` with the pooled arguments None (no host
synchronisation in forward or backward: the step can be captured and replayed).
"""
import numpy as np
import torch
import torch.nn as nn

from . import dense_encoders as E
from . import eigen_pool as ep
from . import message_passing as mp


class WavePoolingGcnEncoder(E.GcnEncoderGraph):
    def __init__(self, max_num_nodes, input_dim, hidden_dim, embedding_dim, label_dim, num_layers, num_pool_matrix=2,
                 num_pool_final_matrix=0, pool_sizes=[4], pred_hidden_dims=[50], concat=True, bn=True, dropout=0.0, mask=1,
                 args=None, device="cpu"):
        # the reference forwards neither bn nor dropout to its base constructor (encoders.py:258-259)
        super().__init__(input_dim, hidden_dim, embedding_dim, label_dim, num_layers, pred_hidden_dims=pred_hidden_dims,
                         concat=concat, args=args)
        # the eigengcn base (encoders.py:69-75) has one prediction MLP and an identity map: drop the other encoder's extra heads
        del self.pre_pred_model, self.map2_model
        self.map_model = nn.Identity()
        add_self = not concat
        if not 1 <= num_pool_matrix <= ep.N_POOL or not 0 <= num_pool_final_matrix <= ep.N_FINAL:
            raise ValueError("num_pool_matrix must lie in [1, 5] and num_pool_final_matrix in [0, 4] (the coarsening builds 5 and 4)")
        self.max_num_nodes = max_num_nodes
        self.embedding_dim = embedding_dim
        self.mask = mask
        self.pool_sizes = pool_sizes
        self.num_pool_matrix = num_pool_matrix
        self.num_pool_final_matrix = num_pool_final_matrix
        self.con_final = getattr(args, "con_final", 1)
        self.conv_first_after_pool = nn.ModuleList()
        self.conv_block_after_pool = nn.ModuleList()
        self.conv_last_after_pool = nn.ModuleList()
        for _ in range(len(pool_sizes)):
            c1, cb, cl = self.build_conv_layers(self.pred_input_dim * num_pool_matrix, hidden_dim, embedding_dim, num_layers,
                                                add_self, normalize=True, dropout=dropout)
            self.conv_first_after_pool.append(c1)
            self.conv_block_after_pool.append(cb)
            self.conv_last_after_pool.append(cl)
        L, P = len(pool_sizes), self.pred_input_dim
        if num_pool_final_matrix > 0:                          # encoders.py:283-311
            if concat:
                head_in = P * (L + 1 if self.con_final else L) + P * num_pool_final_matrix
            else:
                head_in = P * num_pool_final_matrix
        else:
            head_in = P * (L + 1) if concat else P
        self.pred_model = self.build_pred_layers(head_in, pred_hidden_dims, label_dim, num_aggs=self.num_aggs)
        self._init_convs()
        self.to(E._default_device())

    def _stack(self, x, g, convs, masked, per_graph_stack=False):
        emb = self._gcn_rows(x, g, convs, mask_ghost=masked, per_graph_stack=per_graph_stack)
        return emb if self.concat else emb[:, emb.size(1) - self.embedding_dim:]

    def forward(self, x, adj, adj_pooled_list=None, batch_num_nodes=None, batch_num_nodes_list=None, pool_matrices_dic=None,
                readout_only=False, **kwargs):
        """``readout_only``: return the concatenated readouts, the input of ``pred_model`` (eigen_triplet.tripletnet applies
        ``pred_model`` itself, together with both distances)"""
        L, J, Jf = len(self.pool_sizes), self.num_pool_matrix, self.num_pool_final_matrix
        if isinstance(adj, ep.EigenBatch):
            eb = adj
        else:
            eb = ep.batch_from_dense(adj, batch_num_nodes, adj_pooled_list, batch_num_nodes_list, pool_matrices_dic, J, Jf, L)
        if len(eb.levels) != L or (Jf > 0) != (eb.final_coef is not None) or any(lv.J != J for lv in eb.levels) or \
                (Jf and eb.final_coef.size(1) != Jf):
            raise ValueError("the EigenBatch was built for another number of levels / pooling matrices")
        g = eb.g0
        if x.dim() == 3:
            x = mp.pack_rows(x, g, (x.size(2) + 3) // 4 * 4)
        # level 0: always masked; under per-graph statistics (eigen_triplet) it may still run as the fused node
        emb = self._stack(x, g, self.conv_stack(), True, per_graph_stack=True)
        C = emb.size(1)
        head_in = self.pred_model[0].in_features if isinstance(self.pred_model, nn.Sequential) else self.pred_model.in_features
        cols = mp.ReadoutColumns(g.B, head_in, emb.device) if self.concat else None
        out_all = []
        ghost_mode = 1                                         # the ghost rows of a masked embedding are zero
        for i in range(L):
            want_ro = i == 0 or bool(self.con_final) or Jf == 0
            into = cols.take(C) if (cols is not None and want_ro) else None
            if want_ro:
                xp, ro = ep.eigen_pool(emb, g, eb.levels[i], ghost_mode, True, into)
                out_all.append(ro)
            else:
                xp = ep.eigen_pool(emb, g, eb.levels[i], ghost_mode)
            g = eb.levels[i].g
            emb = self._stack(xp, g, self.conv_stack(i + 1), bool(self.mask))
            ghost_mode = 1 if self.mask else 2
        want_ro = L == 0 or bool(self.con_final) or Jf == 0
        if Jf > 0:
            into = cols.take(C) if (cols is not None and want_ro) else None
            into_f = cols.take(Jf * C) if cols is not None else None
            if want_ro:
                fo, ro = ep.eigen_pool_final(emb, g, eb.final_coef, ghost_mode, True, into, into_f)
                out_all.append(ro)
            else:
                fo = ep.eigen_pool_final(emb, g, eb.final_coef, ghost_mode, False, None, into_f)
            out_all.append(fo)
        elif L == 0 or want_ro:
            out_all.append(mp.readout_max(emb, g, into=cols.take(C) if cols is not None else None))
        if self.concat:
            output = cols.join(out_all) if cols is not None else torch.cat(out_all, dim=1)
        else:
            output = out_all[-1]
        if readout_only:
            return output
        return self.pred_model(output)

    def loss(self, pred, label):
        return mp.cross_entropy(pred, label)


class Pool(nn.Module):
    """encoders.py:397-417: x_pooled = cat_j (P_j^T x) for the padded x [B, N, C] and pool_matrices [J][B, N, N]."""

    def __init__(self, num_pool, pool_matrices, device="cpu"):
        super().__init__()
        self.pool_matrices = pool_matrices
        self.num_pool = num_pool
        self.device = device

    def forward(self, x):
        from .graph import GraphBatch
        B, N, C = x.shape
        dev = E._default_device()
        key = tuple((m.data_ptr(), m._version, tuple(m.shape)) for m in list(self.pool_matrices)[:self.num_pool])
        lvl = getattr(self, "_lvl", None)
        if lvl is None or lvl[0] != key:
            # every padded row is a row, the N columns of each graph its clusters: a uniform batch pooled into itself
            g = GraphBatch.uniform(B, N, dev)
            P = ep._pool_operand(self.pool_matrices, self.num_pool, B, N, dev, "Pool")
            bad = torch.zeros(1, dtype=torch.int32, device=dev)
            lv = ep.level_from_dense(P, g, g, bad)
            if int(bad.item()):
                raise ValueError("Pool: a pooling matrix has an entry outside its graph")
            self._lvl = lvl = (key, lv, g)
        z = x.to(dev, torch.float32).contiguous().reshape(B * N, C)
        return ep.eigen_pool(z, lvl[2], lvl[1], 0).reshape(B, N, self.num_pool * C)
