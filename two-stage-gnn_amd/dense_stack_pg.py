"""GCN stack of a pooled DiffPool level under PER-GRAPH statistics (the triplet step, two_stage.embed_dataset / evaluate) as ONE
autograd node on the launches of csrc/dense_stack_pg.hip.

With per-graph statistics the batch-norm of a pooled level is a layer norm of every row (message_passing._RowLn), so nothing but
the product with the adjacency couples rows: a layer is one launch of independent 16-row tiles, and the launch boundary between
two layers is the only synchronisation (no device-wide barriers, unlike dense_stack.py's one-launch form for slot statistics).
Forward: L launches.  Backward: L launches (each forms the input gradient of the layer above as its prologue, accumulates its rows
of the adjacency gradient and leaves its weight-gradient slab) + one for the stack's input gradient + ONE fixed-order reduction of
all layers' slabs.  The layers write straight into the concatenation; its gradient is read in place through leading dimensions.
"""
import torch

from . import _native as nat
from . import message_passing as mp


def _f32(*shape, device):
    return torch.empty(*shape, dtype=torch.float32, device=device)


def convs_ok(convs):
    """what the launches compute: SUM aggregation without the self term, the L2 normalisation, no dropout"""
    return len(convs) >= 1 and not any(c.add_self or not c.normalize_embedding or c.dropout > 0.001 for c in convs)


def eligible(x, adj, convs):
    """the checks of dense_stack.eligible (no add_self, normalize_embedding, dropout <= 0.001, fp32, 16-byte alignment) + the library's
    envelope (tsgnn_dense_pg_supported) for every layer"""
    if not convs_ok(convs) or not (torch.is_tensor(x) and torch.is_tensor(adj)) or not x.is_cuda or not adj.is_cuda:
        return False
    if x.dim() != 3 or adj.dim() != 3 or x.dtype != torch.float32 or adj.dtype != torch.float32:
        return False
    B, K, fin = (int(s) for s in x.shape)
    if tuple(adj.shape) != (B, K, K) or x.data_ptr() % 16 or not x.is_contiguous():
        return False
    lib = nat.lib()
    for c in convs:
        w = c.weight
        if w.dtype != torch.float32 or not w.is_cuda or w.data_ptr() % 16 or not w.is_contiguous() or w.size(0) != fin:
            return False
        if not lib.tsgnn_dense_pg_supported(B, K, fin, int(c.output_dim)):
            return False
        fin = int(c.output_dim)
    return True


class _DenseGcnStackPg(torch.autograd.Function):
    """forward(x[B, K, F], adj[B, K, K], *[weight, bias] per layer) -> [B, K, sum(widths)]"""

    @staticmethod
    def forward(ctx, x, adj, *params):
        B, K, fin0 = (int(s) for s in x.shape)
        R = B * K
        dev = x.device
        ws = [w.contiguous() for w in params[0::2]]
        bs = list(params[1::2])
        L = len(ws)
        widths = [int(w.size(1)) for w in ws]
        offs = [sum(widths[:l]) for l in range(L)]
        total = sum(widths)
        adj = adj.contiguous()
        x2 = x.contiguous().reshape(R, fin0)
        out = _f32(R, total, device=dev)
        keep = any(ctx.needs_input_grad)             # a forward-only call allocates nothing for the backward
        aggs, vs, rinvs, stats = [], [], [], []
        xin, ldx, fin = x2, fin0, fin0
        for l in range(L):
            n = widths[l]
            hidden = l < L - 1
            agg = _f32(R, fin, device=dev) if keep else None
            rinv = _f32(R, device=dev) if keep else None
            v = _f32(R, n, device=dev) if (keep and hidden) else None
            st = _f32(2, R, device=dev) if (keep and hidden) else None
            dst = out[:, offs[l]:offs[l] + n]
            nat.call("dense_pg_layer_fwd_f32", xin, ldx, adj, ws[l], ws[l].stride(0), bs[l], B, K, fin, n, int(hidden), agg, v, rinv,
                     None if st is None else st[0], None if st is None else st[1], dst, total)
            aggs.append(agg); rinvs.append(rinv); vs.append(v); stats.append(st)
            xin, ldx, fin = dst, total, n
        if keep:
            ctx.dims = (B, K, fin0, widths, offs, total)
            ctx.params = params
            ctx.save_for_backward(x2, adj, out, *ws, *aggs, *rinvs, *vs[:-1], *stats[:-1])
        return out.view(B, K, total)

    @staticmethod
    def backward(ctx, dout):
        B, K, fin0, widths, offs, total = ctx.dims
        L = len(widths)
        R = B * K
        sv = ctx.saved_tensors
        x2, adj, out = sv[0], sv[1], sv[2]
        ws = sv[3:3 + L]
        aggs = sv[3 + L:3 + 2 * L]
        rinvs = sv[3 + 2 * L:3 + 3 * L]
        vs = sv[3 + 3 * L:3 + 3 * L + (L - 1)]
        stats = sv[3 + 3 * L + (L - 1):]
        dev = out.device
        dout = mp._check(dout.reshape(R, total))
        need_x, need_adj = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        want = [bool(ctx.needs_input_grad[2 + i]) and ctx.params[i] is not None for i in range(2 * L)]
        fins = [fin0] + widths[:-1]
        shapes = []
        for l in range(L):
            shapes += [(fins[l], widths[l]), (widths[l],)]
        # straight into the trainer's flat gradient bucket when one is installed (FlatTrainer): no AccumulateGrad copy
        bufs, grads = mp._sinks_or_new([p if w_ else None for p, w_ in zip(ctx.params, want)], shapes, dev)
        nslab = B * ((K + 15) // 16)
        dadj = _f32(B, K, K, device=dev) if need_adj else None
        red = mp.WgradSets()                                     # ONE reduction for all layers' slabs, at the end
        dagg_next = None
        first = True
        for l in range(L - 1, -1, -1):
            fin, n = fins[l], widths[l]
            hidden = l < L - 1
            xin, ldx = (x2, fin0) if l == 0 else (out[:, offs[l - 1]:offs[l - 1] + fin], total)
            v, ldv = (vs[l], n) if hidden else (out[:, offs[l]:offs[l] + n], total)
            dw, db = bufs[2 * l], bufs[2 * l + 1]
            slab = _f32(nslab * (fin + 1) * n, device=dev) if (dw is not None or db is not None) else None
            dagg = _f32(R, fin, device=dev) if (l > 0 or need_x) else None
            if slab is None and dagg is None and not need_adj:
                continue
            nat.call("dense_pg_layer_bwd_f32", adj, ws[l], ws[l].stride(0), aggs[l], v, ldv, rinvs[l],
                     stats[l][0] if hidden else None, stats[l][1] if hidden else None, xin if need_adj else None, ldx,
                     dout[:, offs[l]:offs[l] + n], dout.stride(0), dagg_next, B, K, fin, n, int(hidden), dagg, slab, dadj, int(not first))
            first = False
            if slab is not None:
                red.add(mp.wgrad_set(slab, nslab, fin, n, dw if dw is not None else _f32(fin, n, device=dev), db, kn=1, lddw=n))
            dagg_next = dagg
        dx = None
        if need_x:
            dx = _f32(R, fin0, device=dev)
            nat.call("dense_pg_dx_f32", adj, dagg_next, B, K, fin0, dx, fin0)
            dx = dx.view(B, K, fin0)
        red.close()
        return (dx, dadj) + tuple(grads)


def dense_gcn_stack_pg(x, adj, convs):
    """concatenated layer outputs [B, K, sum(widths)] of conv_first / conv_block / conv_last on the pooled level (x, adj), every
    graph with the statistics it would have alone in its batch"""
    params = []
    for c in convs:
        params += [c.weight, c.bias]
    return _DenseGcnStackPg.apply(x, adj, *params)
