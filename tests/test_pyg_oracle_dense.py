"""oracle/pyg_ref.gat_conv / sage_conv / graph_conv (the fp64 yardstick of the GPU layer tests) against dense restatements of the
same layers: an n x n edge-multiplicity matrix instead of scatter / index_add over the edge list.  CPU only."""
import pytest
import torch
import torch.nn.functional as F

from oracle import pyg_ref as P


def _multiplicity(ei, n, gat=False):
    """M[i, j] = number of edges j -> i (targets = row 1).  gat: GATConv's edge list (self loops dropped, one added per node)"""
    if gat:
        ei = ei[:, ei[0] != ei[1]]
    M = torch.zeros(n, n, dtype=torch.float64)
    M.index_put_((ei[1], ei[0]), torch.ones(ei.size(1), dtype=torch.float64), accumulate=True)
    if gat:
        M += torch.eye(n, dtype=torch.float64)
    return M


def _dense_gat(x, M, w, att_l, att_r, bias, heads, concat, slope):
    n = x.size(0)
    C = w.size(0) // heads
    h = (x @ w.t()).view(n, heads, C)
    s_src = (h * att_l.view(1, heads, C)).sum(-1)                  # [n, H]: node as source j
    s_dst = (h * att_r.view(1, heads, C)).sum(-1)                  # node as target i
    e = F.leaky_relu(s_dst.t().unsqueeze(2) + s_src.t().unsqueeze(1), slope)          # [H, i, j]
    e = e.masked_fill(M.unsqueeze(0) == 0, -float("inf"))
    p = M.unsqueeze(0) * torch.exp(e - e.max(dim=2, keepdim=True).values)
    alpha = p / p.sum(dim=2, keepdim=True)
    out = torch.einsum("hij,jhc->ihc", alpha, h)
    out = out.reshape(n, heads * C) if concat else out.mean(dim=1)
    return out + bias if bias is not None else out


def _graphs(seed, n):
    """a directed list with duplicates, self loops and a node without in-edges"""
    g = torch.Generator().manual_seed(seed)
    src, dst = torch.randint(0, n, (4 * n,), generator=g), torch.randint(0, n - 1, (4 * n,), generator=g)
    ei = torch.stack([src, dst])
    loops = torch.arange(0, n, 5)
    return torch.cat([ei, ei[:, :7], torch.stack([loops, loops])], dim=1)


def _grads_both(f_a, f_b, tensors, gy):
    ta = [t.clone().requires_grad_(True) if t is not None else None for t in tensors]
    tb = [t.clone().requires_grad_(True) if t is not None else None for t in tensors]
    ya, yb = f_a(*ta), f_b(*tb)
    la = [t for t in ta if t is not None]
    lb = [t for t in tb if t is not None]
    return ya, yb, torch.autograd.grad((ya * gy).sum(), la), torch.autograd.grad((yb * gy).sum(), lb)


@pytest.mark.parametrize("heads,C,concat,slope,bias", [(1, 4, True, 0.2, True), (4, 8, False, 0.2, True), (8, 4, True, 0.05, False),
                                                       (2, 16, False, 0.2, False)])
def test_gat_conv_oracle_matches_dense(heads, C, concat, slope, bias):
    n, fin = 23, 6
    ei = _graphs(1 + heads, n)
    g = torch.Generator().manual_seed(heads * 10 + C)
    x = torch.randn(n, fin, generator=g, dtype=torch.float64)
    w = torch.randn(heads * C, fin, generator=g, dtype=torch.float64)
    al = 0.5 * torch.randn(1, heads, C, generator=g, dtype=torch.float64)
    ar = 0.5 * torch.randn(1, heads, C, generator=g, dtype=torch.float64)
    b = torch.randn(heads * C if concat else C, generator=g, dtype=torch.float64) if bias else None
    M = _multiplicity(ei, n, gat=True)
    assert M.max() >= 2 and int((M.diagonal() == 1).sum()) == n            # duplicates; exactly one loop per node
    gy = torch.randn(n, heads * C if concat else C, generator=g, dtype=torch.float64)
    ya, yb, ga, gb = _grads_both(lambda *t: P.gat_conv(t[0], ei, t[1], t[2], t[3], t[4], heads, concat=concat, slope=slope),
                                 lambda *t: _dense_gat(t[0], M, t[1], t[2], t[3], t[4], heads, concat, slope), [x, w, al, ar, b], gy)
    torch.testing.assert_close(ya, yb, rtol=1e-12, atol=1e-12)
    for a, c in zip(ga, gb):
        torch.testing.assert_close(a, c, rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("aggr", ["mean", "add"])
@pytest.mark.parametrize("K,N,bias", [(1, 3, True), (5, 4, False), (33, 31, True)])
def test_sage_conv_oracle_matches_dense(aggr, K, N, bias):
    """SAGEConv: D^-1 A X W_l^T + b + X W_r^T (D = max(in-degree, 1)); GraphConv: A X W_l^T + b + X W_r^T"""
    n = 29
    ei = _graphs(7 + K, n)
    g = torch.Generator().manual_seed(K * 100 + N)
    x = torch.randn(n, K, generator=g, dtype=torch.float64)
    wl, wr = torch.randn(N, K, generator=g, dtype=torch.float64), torch.randn(N, K, generator=g, dtype=torch.float64)
    b = torch.randn(N, generator=g, dtype=torch.float64) if bias else None
    A = _multiplicity(ei, n)
    assert A.max() >= 2 and A.diagonal().sum() > 0 and A.sum(1).min() == 0
    Dinv = 1.0 / A.sum(1).clamp(min=1) if aggr == "mean" else torch.ones(n, dtype=torch.float64)
    gy = torch.randn(n, N, generator=g, dtype=torch.float64)
    fn = P.sage_conv if aggr == "mean" else P.graph_conv

    def dense(xx, wwl, wwr, bb):
        y = (Dinv.unsqueeze(1) * (A @ xx)) @ wwl.t() + xx @ wwr.t()
        return y + bb if bb is not None else y

    ya, yb, ga, gb = _grads_both(lambda xx, wwl, wwr, bb: fn(xx, ei, wwl, bb, wwr), dense, [x, wl, wr, b], gy)
    torch.testing.assert_close(ya, yb, rtol=1e-12, atol=1e-12)
    for a, c in zip(ga, gb):
        torch.testing.assert_close(a, c, rtol=1e-12, atol=1e-12)
