"""Reference of the per-node-slot operations of the GraphSage stack (ReLU + slot batch-norm, its backward fused with the max-readout
scatter and the row L2-normalise backward, the max readout), written from the dense formulation ``x[B, Nmax, F]`` of
oracle/dense_ref.py on the packed row layout the kernels use.  TEST INFRASTRUCTURE: plain torch on the CPU, no project kernel;
float64 by default, ``dtype=torch.float32`` runs the SAME code in single precision (the yardstick of the kernels' rounding).

Rows: ``[0, n_real)`` real nodes graph after graph (rows ``[graph_ptr[B], n_real)`` belong to no graph: a capacity-padded batch),
``[n_real, n_real + n_ghost)`` one ghost row per node slot, ``n_ghost`` in ``{0, nmax}``.

Candidate ``(b, n)`` — what the reference's dense tensor holds at ``[b, n, :]``:
  * the real row ``graph_ptr[b] + n``             if ``n < sizes[b]``;
  * the ghost row ``n_real + n``                  otherwise, if the layout has ghost rows (one COPY of that row per such graph);
  * absent                                         otherwise (the padded layout materialises every row it has).
"""
import numpy as np
import torch

BN_EPS = 1e-5
CLAMPED = 0.999e12          # rinv at or above this marks a row whose norm was clamped to 1e-12: no projection in its backward


class Layout:
    """idx [B, nmax] (row of candidate (b, n), -1: absent), present / ghost masks, slot_count, graph_ptr"""

    def __init__(self, sizes, nmax, n_ghost, n_real=None):
        sizes = np.asarray(sizes, dtype=np.int64).reshape(-1)
        assert n_ghost in (0, nmax) and (sizes >= 0).all() and (sizes <= nmax).all()
        self.sizes, self.nmax, self.n_ghost, self.B = sizes, int(nmax), int(n_ghost), int(sizes.size)
        gp = np.zeros(self.B + 1, dtype=np.int64)
        np.cumsum(sizes, out=gp[1:])
        self.graph_ptr = gp
        self.n_real = int(gp[-1]) if n_real is None else int(n_real)
        assert self.n_real >= gp[-1]
        self.rows = self.n_real + self.n_ghost
        n = np.arange(self.nmax)[None, :]
        real = n < sizes[:, None]
        idx = np.where(real, gp[:-1, None] + n, (self.n_real + n) if n_ghost else -1)
        self.idx = torch.from_numpy(idx)
        self.present = self.idx >= 0
        self.real = torch.from_numpy(real)
        self.ghost = self.present & ~self.real
        self.slot_count = real.sum(0)                                        # graphs that HAVE slot n
        # first ghost copy of every slot (B: none)
        g = self.ghost.numpy()
        self.first_ghost = np.where(g.any(0), g.argmax(0), self.B)
        self.unused_ghost_rows = [self.n_real + k for k in range(self.n_ghost) if self.slot_count[k] == self.B]
        self.pad_rows = list(range(int(gp[-1]), self.n_real))

    def row_graph(self, pad_value=None):
        """graph of every real row; padding rows get ``pad_value`` (default B)"""
        rg = np.full(self.n_real, self.B if pad_value is None else pad_value, dtype=np.int32)
        rg[: self.graph_ptr[-1]] = np.repeat(np.arange(self.B), self.sizes)
        return rg


def _dense(v, L):
    return v[L.idx.clamp(min=0)]                                             # absent candidates: masked by the callers


def _slot_bn_dense(v, L, relu, bn):
    """(mean [nmax], rstd [nmax], y_dense [B, nmax, F]); differentiable in v"""
    F = v.size(1)
    m = L.present[:, :, None].to(v.dtype)
    h = _dense(v, L)
    if relu:
        h = torch.relu(h)
    h = h * m
    cnt = m.sum(dim=(0, 2)) * F                                              # B*F with ghosts, slot_count[n]*F without
    safe = cnt.clamp(min=1.0)
    mean = torch.where(cnt > 0, h.sum(dim=(0, 2)) / safe, torch.zeros_like(cnt))
    d = (h - mean[None, :, None]) * m
    var = torch.where(cnt > 0, (d * d).sum(dim=(0, 2)) / safe, torch.zeros_like(cnt))
    rstd = 1.0 / torch.sqrt(var + BN_EPS)
    y = d * rstd[None, :, None] if bn else h
    return mean, rstd, y


def _to_rows(y_dense, L):
    """every candidate's value at its row; all ghost copies of a row are equal; rows nobody is a candidate of stay 0"""
    y = torch.zeros(L.rows, y_dense.size(2), dtype=y_dense.dtype)
    y[L.idx[L.present]] = y_dense[L.present]
    return y


def slot_bn(v, L, relu=True, bn=True, dtype=torch.float64):
    """-> mean [nmax], rstd [nmax], y [rows, F]: y = (relu(v) - mean[slot]) * rsqrt(var[slot] + 1e-5), statistics per slot over the
    present candidates x F (biased variance); a slot without candidates has mean 0, rstd 1/sqrt(1e-5)"""
    mean, rstd, y = _slot_bn_dense(v.to(dtype), L, relu, bn)
    return mean, rstd, _to_rows(y, L)


def _dv(v, L, dy_dense, relu, bn):
    """gradient of sum(y_dense * dy_dense) with respect to the rows of v (ghost copies sum into their one row)"""
    v = v.detach().clone().requires_grad_(True)
    y = _slot_bn_dense(v, L, relu, bn)[2]
    loss = (y * dy_dense * L.present[:, :, None].to(v.dtype)).sum()
    if not loss.requires_grad:
        return torch.zeros_like(v)
    return torch.autograd.grad(loss, v)[0]


def l2_bwd(v, rinv, dv):
    """du = rinv (dv - v <v, dv>); <v, dv> is taken as 0 where the norm was clamped"""
    dot = (v * dv).sum(dim=1, keepdim=True)
    dot = torch.where(rinv[:, None] >= CLAMPED, torch.zeros_like(dot), dot)
    return rinv[:, None] * (dv - v * dot)


def rows_to_dense_grad(dy_rows, L):
    """a gradient given per ROW as the dense dy: real candidates take their row's, the FIRST ghost copy of a slot takes the ghost
    row's (the other copies 0: the row's gradient counts once)"""
    F = dy_rows.size(1)
    out = torch.zeros(L.B, L.nmax, F, dtype=dy_rows.dtype)
    out[L.real] = dy_rows[L.idx[L.real]]
    for n in range(L.nmax if L.n_ghost else 0):
        b = int(L.first_ghost[n])
        if b < L.B:
            out[b, n] = dy_rows[L.n_real + n]
    return out


def slot_bn_bwd(v, L, dy_rows, relu=True, bn=True, dtype=torch.float64):
    """dv [rows, F] of y = slot_bn(v) for a gradient dy given per row"""
    return _dv(v.to(dtype), L, rows_to_dense_grad(dy_rows.to(dtype), L), relu, bn)


def post_dy_dense(L, F, dxs, dxs2, dout, arg, dtype):
    """dy_dense[b, n] = dxs[row] + dxs2[row] (real candidates only) + dout[b, f] where arg[b, f] == row(b, n)"""
    dy = torch.zeros(L.B, L.nmax, F, dtype=dtype)
    for t in (dxs, dxs2):
        if t is not None:
            dy[L.real] += t.to(dtype)[L.idx[L.real]]
    if arg is not None:
        hit = (arg.long()[:, None, :] == L.idx[:, :, None]) & L.present[:, :, None]
        dy = dy + hit.to(dtype) * dout.to(dtype)[:, None, :]
    return dy


def slot_post_bwd(v, rinv, L, dxs=None, dxs2=None, dout=None, arg=None, relu=True, bn=True, dtype=torch.float64):
    """du [rows, F]: backward of [max-readout scatter + dxs + dxs2] -> slot BN -> ReLU -> row L2 normalise.  Rows that are nobody's
    candidate (capacity padding, unused ghost rows) get 0."""
    v = v.to(dtype)
    dv = _dv(v, L, post_dy_dense(L, v.size(1), dxs, dxs2, dout, arg, dtype), relu, bn)
    return l2_bwd(v, rinv.to(dtype), dv)


def readout_l2_bwd(v, rinv, dout, arg, row_graph, n_ghost_rows, dtype=torch.float64):
    """the same with relu = bn = 0 and no dxs, row-parallel: dy[r, f] = sum of dout[b, f] over the graphs b with arg[b, f] == r
    (a real row can only be won by its own graph); padding rows (row_graph >= B) are 0"""
    v, rinv, dout = v.to(dtype), rinv.to(dtype), dout.to(dtype)
    B, F = dout.shape
    n_real = len(row_graph)
    rows = n_real + int(n_ghost_rows)
    dy = torch.zeros(rows, F, dtype=dtype)
    rg = torch.as_tensor(np.asarray(row_graph), dtype=torch.long)
    a = arg.long().reshape(B, F)
    for b in range(B):                                                       # graph order
        for f in torch.nonzero(a[b] >= 0).flatten().tolist():
            r = int(a[b, f])
            assert r < rows and (r >= n_real or int(rg[r]) == b)
            dy[r, f] += dout[b, f]
    return l2_bwd(v[:rows], rinv[:rows], dy)


def readout_max(x, L):
    """(out [B, F], arg int32 [B, F]): max over the candidates of each graph, the smallest row id among equal values (so a real
    row beats a ghost row); a graph without candidates: out 0, arg -1"""
    F = x.size(1)
    d = _dense(x, L)
    neg = torch.full_like(d, -float("inf"))
    d = torch.where(L.present[:, :, None], d, neg)
    out = d.max(dim=1)[0]
    big = torch.iinfo(torch.int64).max
    rid = torch.where((d == out[:, None, :]) & L.present[:, :, None], L.idx[:, :, None].expand(-1, -1, F),
                      torch.full((1, 1, 1), big, dtype=torch.int64))
    arg = rid.min(dim=1)[0]
    none = arg == big
    return torch.where(none, torch.zeros_like(out), out), torch.where(none, torch.full_like(arg, -1), arg).to(torch.int32)


def wgrad_slab_sum(z, du, n_real, K_in):
    """[K_in + 1, F]: rows [0, K_in) = Z^T dU over the real rows, row K_in = the column sums of dU over real AND ghost rows"""
    return torch.cat([z[:n_real, :K_in].t() @ du[:n_real], du.sum(dim=0, keepdim=True)], dim=0)
