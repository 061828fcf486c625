"""The pooled-level GCN layer under per-graph statistics (csrc/dense_stack_pg.hip) in plain torch, dtype-parametric: run it in float64
for the reference and in float32 on the CPU for the yardstick (fp32_yardstick.py).  Backward comes through autograd.
TEST INFRASTRUCTURE: no project kernel."""
import torch

NORM_EPS = 1e-12        # F.normalize
BN_EPS = 1e-5


def layer_fwd(x, adj, w, bias, hidden):
    """x[B, K, fin], adj[B, K, K], w[fin, n], bias[n] or None -> (agg, v, rinv, mean, rstd, y); mean / rstd are None on the last layer
    (hidden=False: encoders.py:165, no ReLU, no batch norm).  The batch norm of a graph alone in its batch is a layer norm of every
    row over its features (biased variance, eps 1e-5)."""
    agg = torch.matmul(adj, x)
    u = torch.matmul(agg, w)
    if bias is not None:
        u = u + bias
    rinv = 1.0 / torch.sqrt((u * u).sum(dim=2, keepdim=True)).clamp_min(NORM_EPS)
    v = u * rinv
    if not hidden:
        return agg, v, rinv.squeeze(2), None, None, v
    r = torch.relu(v)
    mean = r.mean(dim=2, keepdim=True)
    var = ((r - mean) ** 2).mean(dim=2, keepdim=True)
    rstd = 1.0 / torch.sqrt(var + BN_EPS)
    return agg, v, rinv.squeeze(2), mean.squeeze(2), rstd.squeeze(2), (r - mean) * rstd


def stack_fwd(x, adj, params):
    """params: [(w, bias or None)] of conv_first / conv_block / conv_last -> the concatenated layer outputs [B, K, sum(widths)]"""
    ys = []
    for l, (w, b) in enumerate(params):
        x = layer_fwd(x, adj, w, b, l < len(params) - 1)[5]
        ys.append(x)
    return torch.cat(ys, dim=2)


def inputs(seed, B, K, fin, n, bias=True, dtype=torch.float64):
    """one layer's operands: a dense, positive, non-symmetric adjacency (what S^T A S is), features and weights scaled so that no row of
    u is short (the test asserts |u| >= 1e-3)"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, K, fin, generator=g, dtype=torch.float64)
    adj = torch.rand(B, K, K, generator=g, dtype=torch.float64) * 0.9 + 0.1
    w = torch.randn(fin, n, generator=g, dtype=torch.float64) / fin ** 0.5
    b = torch.randn(n, generator=g, dtype=torch.float64) * 0.3 if bias else None
    cast = lambda t: None if t is None else t.float().to(dtype)       # every dtype sees the same fp32-representable values
    return cast(x), cast(adj), cast(w), cast(b)
