"""BASELINE config 4 as worded — "IMDB-BINARY SAGPool (ratio 0.5) + SAGEConv h=128" — as ONE sync-free autograd node: the three
conv -> SAGPool -> readout levels of Code/sag/network.py:33-44 with the network's GCNConv layers replaced by PyG SAGEConv
(lin_l(mean_j x_j) + lin_r(x_i)); the pooling layer is the reference's own SAGPool (Code/sag/layers.py:7-25: GCNConv(C -> 1) scorer, top-k,
tanh gate, filter_adj), i.e. the per-graph kernels of sag_stack.py unchanged.

What changes against sag_stack._SagStack is the conv of a level:
    agg  = mean aggregation over the level's (filtered) CSR        tsgnn_propagate_mean_f32 (1 / deg from the row lengths: no coefficient arrays)
    y    = [agg || x] . [W_l | W_r]^T + b                           ONE row-panel product on the concatenation (K = 2 * ceil4(F_in)): the
                                                                    aggregation writes the left half of the buffer, the previous level's gated
                                                                    gather wrote the right half in place (its output stride is a parameter)
and, backward, the slabs of dW_l = agg^T dy and dW_r = x^T dy in one launch (tsgnn_sage_wgrad_pair_f32), d[agg || x] = dy . [W_l | W_r],
dx = A_mean^T dagg + dself in one launch (tsgnn_propagate_mean_f32, transpose form, self half added from its own columns); ONE reduction
at the end of the backward sums every level's slabs into nn.Linear's layout AND the score layers' per-graph partial rows, straight into
the flat gradient bucket with |grad|^2 shares when a FlatTrainer is listening.  The [W_l | W_r] images of all levels: one launch
(tsgnn_copy2d_multi_f32), which also places the input features in the level-0 concatenation (every forward: a resident input refilled
between graph replays is followed).  Launches per step: 1 + 3 x 3 forward, 3 + 4 + 4 + 1 backward (the GCN network of sag_stack.py: 6 and
10).  Symmetric edge lists (every TU dataset); other inputs take the composed operators (pyg.SagePoolNet).  PARITY UNPINNED for the SAGEConv
half; the SAGPool half follows layers.py:14-25.

scorer = "graphconv": PyG SAGPooling's score layer instead, GraphConv(C -> 1) = gnn.lin_l(sum_j x_j) + gnn.lin_r(x_i) on x = relu(y)
(pyg.SagePoolNet, BASELINE config 4 as PyG words it): the same two per-graph launches in their GraphConv form
(tsgnn_sag_pool_graph_gc_f32 / _gc_bwd_f32), no gcn_norm coefficients, and partial rows of 2H + 4 floats that the closing reduction
splits into gnn.lin_l.weight / .bias and gnn.lin_r.weight."""
import numpy as np
import torch

from . import _native as nat
from . import message_passing as mp
from . import pyg_sage as ps
from . import sag_stack as ss

_f32 = mp._f32
_i32 = ss._i32


def _ceil4(k):
    return (int(k) + 3) // 4 * 4


def _prop_mean(rowptr, rowend, col, transpose, x, ldx, xself, ldxs, y, ldy, n, feat):
    nat.call("propagate_mean_f32", rowptr, rowend, col, int(transpose), x, int(ldx), xself, int(ldxs), y, int(ldy), int(n), int(feat))


def _wcats(pairs, device, x=None, cat0=None):
    """[W_l | W_r] of every level in nn.Linear's [out, in] layout, both halves padded to Kp = ceil4(K) columns: [H, 2 Kp] each, ONE launch.
    x, cat0: the input features go to the right half of level 0's concatenation [N, 2 Kp0] (zero-padded) in the same launch"""
    outs, words = [], [2 * len(pairs) + (x is not None)]
    for wl, wr in pairs:
        H, K = int(wl.size(0)), int(wl.size(1))
        Kp = _ceil4(K)
        o = _f32(H, 2 * Kp, device=device)
        for t, w in enumerate((wl, wr)):
            words += [w.data_ptr(), int(w.stride(0)), H, K, o.data_ptr() + 4 * t * Kp, int(o.stride(0)), Kp]
        outs.append(o)
    if x is not None:
        Kp0 = cat0.size(1) // 2
        words += [x.data_ptr(), int(x.stride(0)), int(x.size(0)), int(x.size(1)), cat0.data_ptr() + 4 * Kp0, int(cat0.stride(0)), Kp0]
    d = np.asarray(words, dtype=np.int64)
    nat.call("copy2d_multi_f32", d.ctypes.data)
    return outs


SCORERS = {"gcn": 5, "graphconv": 6}             # parameters per level


def _cat0(x, N, Kp0):
    """level 0's concatenation buffer [N, 2 Kp0], allocated once per resident input tensor (kept on it, as segment_sizes keeps the
    graph sizes on ``batch``); its contents are written by every forward, never cached: the left half by the aggregation, the right
    half from x by the weight-image launch.  Zeros at allocation: the padding columns of the left half are never written."""
    hit = getattr(x, "_tsgnn_sage_cat0", None)
    if hit is not None and hit[0] == (N, Kp0) and hit[1].device == x.device:
        return hit[1]
    cat = torch.zeros(N, 2 * Kp0, dtype=torch.float32, device=x.device)
    x._tsgnn_sage_cat0 = ((N, Kp0), cat)
    return cat


class _SagSageStack(torch.autograd.Function):
    """forward(x, g, plan, scorer, perms_out, *[W_l, b_l, W_r, score parameters] per level) -> readout [B, 2H].  score parameters:
    (weight [1, H], bias [1]) for scorer "gcn", (gnn.lin_l.weight, gnn.lin_l.bias, gnn.lin_r.weight) for "graphconv".  perms_out
    (a list or None): gets each level's perm (int32 [K_l], rows of the level, grouped by graph, descending score)"""

    @staticmethod
    def forward(ctx, x, g, plan, scorer, perms_out, *params):
        depth = plan.depth
        if scorer not in SCORERS:
            raise ValueError("scorer: one of %s" % sorted(SCORERS))
        P = SCORERS[scorer]
        gc = scorer == "graphconv"
        if len(params) != P * depth:
            raise ValueError("expected (lin_l.weight, lin_l.bias, lin_r.weight, %s) per level"
                             % ("gnn.lin_l.weight, gnn.lin_l.bias, gnn.lin_r.weight" if gc else "score weight, score bias"))
        if plan.levels[0].N != g.total_rows or x.size(0) != g.total_rows:
            raise ValueError("plan, graph and features disagree on the number of nodes")
        if g.val is not None or not g.symmetric:
            raise NotImplementedError("the one-node SAGPool + SAGEConv stack takes unit-weight symmetric edge lists")
        dev = x.device
        H = int(params[0].size(0))
        B = plan.levels[0].B
        rowptr, col, rowend = g.rowptr, g.col, None
        dinv, self_w = (None, None) if gc else ss.gcn_coef(g)   # GCN coefficients: the SCORE layer of the pool (layers.py:18)
        nnz_bound = max(int(col.numel()), 1)
        read = _f32(B, 2 * H, device=dev)
        pool_graph_max = int(nat.lib().tsgnn_sag_pool_graph_max_nodes())
        if plan.levels[0].max_seg > pool_graph_max:
            raise NotImplementedError("graphs of more than %d nodes: use the composed operators" % pool_graph_max)
        # level 0's concatenation buffer [N, 2 Kp]: the features go to its right half in the weight images' launch
        K0 = int(x.size(1))
        Kp0 = _ceil4(K0)
        xs = x if (x.dtype == torch.float32 and x.stride(1) == 1) else x.float().contiguous()
        cat = _cat0(x, plan.levels[0].N, Kp0)
        wcats = _wcats([(params[P * l].contiguous(), params[P * l + 2].contiguous()) for l in range(depth)], dev, x=xs, cat0=cat)
        saved = []
        K, Kp = K0, Kp0
        for l in range(depth):
            L, Ln = plan.levels[l], plan.levels[l + 1]
            N, Kn = L.N, Ln.N
            wl, bl, wr, ws, bs = params[P * l: P * l + 5]
            wrt = ss._al16(params[P * l + 5].contiguous().view(-1)) if gc else None
            wcat = wcats[l]
            wsv = ss._al16(ws.contiguous().view(-1))
            bl = ss._al16(bl.contiguous())
            # agg -> the left half of the concatenation, then ONE product for both weights
            _prop_mean(rowptr, rowend, col, 0, cat[:, Kp:], cat.stride(0), None, 0, cat, cat.stride(0), N, K)
            y = _f32(N, H, device=dev)
            nat.call("rowgemm_f32", cat, cat.stride(0), wcat, wcat.stride(0), 1, bl, y, y.stride(0), None, N, 2 * Kp, H, 0, 0)
            # the level's tail (score, top-k, gated gather, readout, filter): one workgroup per graph; the kept rows land in the right half of
            # the NEXT level's concatenation
            cat_n = _f32(max(Kn, 1), 2 * H, device=dev)
            xp = cat_n[:, H:]
            perm, new_id = _i32(max(Kn, 1), device=dev), _i32(max(N, 1), device=dev)
            cnt = _i32(max(Kn, 1), device=dev)
            arg = _i32(B, H, device=dev)
            score = _f32(N, device=dev)
            last = l + 1 == depth
            rp_n = re_n = col_n = dinv_n = self_w_n = None
            if not last:
                rp_n, re_n, col_n = _i32(Kn, device=dev), _i32(Kn, device=dev), _i32(nnz_bound, device=dev)
                if not gc:
                    dinv_n, self_w_n = _f32(Kn, device=dev), _f32(Kn, device=dev)
            if gc:
                nat.call("sag_pool_graph_gc_f32", y, y.stride(0), rowptr, rowend, col, wsv, wrt, bs, L.gp, Ln.gp, B, L.max_seg, H,
                         score, perm, new_id, xp, xp.stride(0), cnt, read, read.stride(0), arg, int(l > 0), rp_n, re_n, col_n)
            else:
                nat.call("sag_pool_graph_f32", y, y.stride(0), rowptr, rowend, col, dinv, self_w, wsv, bs, L.gp, Ln.gp, B, L.max_seg, H,
                         score, perm, new_id, xp, xp.stride(0), cnt, read, read.stride(0), arg, int(l > 0),
                         rp_n, re_n, col_n, dinv_n, self_w_n, None, 0)
            if perms_out is not None:
                perms_out.append(perm[:Kn])
            saved.append((cat, y, score, new_id, arg, rowptr, col, rowend, dinv, self_w, wcat, wsv, wrt, K, Kp))
            if not last:
                rowptr, col, rowend, dinv, self_w = rp_n, col_n, re_n, dinv_n, self_w_n
            cat, K, Kp = cat_n, H, H
        ctx.plan, ctx.saved_levels, ctx.H, ctx.P = plan, saved, H, P
        ctx.x_needs_grad = x.requires_grad
        ctx.params = params
        return read

    @staticmethod
    def backward(ctx, dread):
        plan, H, P = ctx.plan, ctx.H, ctx.P
        gc = P == 6
        depth = plan.depth
        dread = dread.contiguous()
        dev = dread.device
        grads = [None] * (P * depth)
        red = mp.WgradSets()
        dxp = None
        dx = None
        for l in range(depth - 1, -1, -1):
            L, Ln = plan.levels[l], plan.levels[l + 1]
            N = L.N
            cat, y, score, new_id, arg, rowptr, col, rowend, dinv, self_w, wcat, wsv, wrt, K, Kp = ctx.saved_levels[l]
            wl, bl, wr, ws, bs = ctx.params[P * l: P * l + 5]
            dyb = _f32(N, H, device=dev)
            part = _f32(L.B * ((2 * H if gc else H) + 4), device=dev)
            if gc:
                nat.call("sag_pool_graph_gc_bwd_f32", y, y.stride(0), score, new_id, L.gp, Ln.gp, arg, dxp,
                         dxp.stride(0) if dxp is not None else 0, dread, dread.stride(0), rowptr, rowend, col, wsv, wrt,
                         L.B, L.max_seg, H, dyb, dyb.stride(0), part)
            else:
                nat.call("sag_pool_graph_bwd_f32", y, y.stride(0), score, new_id, L.gp, Ln.gp, arg, dxp,
                         dxp.stride(0) if dxp is not None else 0, dread, dread.stride(0), rowptr, rowend, col, dinv, self_w, wsv,
                         L.B, L.max_seg, H, dyb, dyb.stride(0), part, None, None, None, 0, None, None, None, None, None)
            # the slabs of dW_l = agg^T dy (+ db) and dW_r = x^T dy: one launch; their sum waits for the end of the backward
            sl = ps.wgrad_slabs(cat, cat[:, Kp:], K, dyb)
            if sl is None:
                raise RuntimeError("SAGPool + SAGEConv stack: weight-gradient shape %d x %d is not taken by the slab kernel" % (K, H))
            dwl, dbl, dwr = red.grad(wl, (H, K)), red.grad(bl, (H,)), red.grad(wr, (H, K))
            dws, dbs = red.grad(ws, tuple(ws.shape)), red.grad(bs, (1,))
            red.add(mp.wgrad_set(sl[0][0], sl[0][1], K, H, dwl, dbl))
            red.add(mp.wgrad_set(sl[1][0], sl[1][1], K, H, dwr))
            if gc:
                # partial rows [dw_rel | db | 3 unused | dw_root]: dw_root from column H + 4 of the same set
                wroot = ctx.params[P * l + 5]
                dwt = red.grad(wroot, tuple(wroot.shape))
                red.add(mp.wgrad_set(part, L.B, 0, 2 * H + 4, dwt, dws, n_db=H, tail=dbs, lddw=H + 4))
            else:
                dwt = None
                red.add(mp.wgrad_set(part, L.B, 0, H + 4, None, dws, n_db=H, tail=dbs))
            grads[P * l: P * l + P] = [red.autograd_grad(t) for t in (dwl, dbl, dwr, dws, dbs, dwt)[:P]]
            if l > 0 or ctx.x_needs_grad:
                dcat = _f32(N, 2 * Kp, device=dev)
                nat.call("rowgemm_f32", dyb, dyb.stride(0), wcat, wcat.stride(0), 0, None, dcat, dcat.stride(0), None, N, H, 2 * Kp, 0, 0)
                # dx = A_mean^T dagg + dself   (symmetric edge list: rows of A^T = rows of A; the 1 / deg moves to the gathered rows)
                dxin = _f32(N, Kp, device=dev)
                _prop_mean(rowptr, rowend, col, 1, dcat, dcat.stride(0), dcat[:, Kp:], dcat.stride(0), dxin, dxin.stride(0), N, K)
                if l > 0:
                    dxp = dxin
                else:
                    dx = dxin[:, :K]
        red.close()
        return (dx, None, None, None, None, *grads)


def sag_sage_stack(x, g, plan, params, scorer="gcn", perms_out=None):
    """readout[B, 2H] = sum over the levels of [gmp || gap] (network.py:36-46) with SAGEConv layers.  params: per level
    (lin_l.weight [H, in], lin_l.bias [H], lin_r.weight [H, in]) and the score layer's: scorer "gcn" (the reference's SAGPool,
    layers.py:18) score weight [H, 1], score bias [1]; scorer "graphconv" (PyG SAGPooling) gnn.lin_l.weight [1, H], gnn.lin_l.bias [1],
    gnn.lin_r.weight [1, H].  perms_out (list, nullable): receives each level's perm buffer (int32, see _SagSageStack)."""
    return _SagSageStack.apply(x, g, plan, scorer, perms_out, *params)
