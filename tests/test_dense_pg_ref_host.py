"""tests/dense_pg_ref.py (the reference of the per-graph pooled-level kernels) against the pinned oracle: in float64 the stack equals
oracle/dense_ref.gcn_forward on every graph ALONE (B = 1, bn=True, concat=True), values and gradients.  No GPU."""
import pytest
import torch

import dense_pg_ref as PG
from oracle import dense_ref as R


def _case(seed, B, K, widths, bias):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, K, widths[0], generator=g, dtype=torch.float64)
    adj = torch.rand(B, K, K, generator=g, dtype=torch.float64) * 0.9 + 0.1
    params = []
    for fin, n in zip(widths[:-1], widths[1:]):
        params.append((torch.randn(fin, n, generator=g, dtype=torch.float64) / fin ** 0.5,
                       torch.randn(n, generator=g, dtype=torch.float64) * 0.3 if bias else None))
    return x, adj, params


def _oracle(x, adj, params):
    p, L = {}, len(params)
    for l, (w, b) in enumerate(params):
        name = "cf" if l == 0 else ("cl" if l == L - 1 else "cb.%d" % (l - 1))
        p[name + ".weight"] = w
        if b is not None:
            p[name + ".bias"] = b
    return torch.cat([R.gcn_forward(p, ("cf", "cb", "cl"), x[b:b + 1], adj[b:b + 1], None, bn=True, concat=True) for b in range(x.size(0))])


@pytest.mark.parametrize("B,K,widths,bias", [(1, 4, (4, 4, 4), True), (3, 20, (12, 8, 8, 12), True), (2, 36, (20, 16, 100), False),
                                             (3, 100, (24, 8, 8, 8, 4), True)])
def test_reference_equals_the_oracle_on_each_graph_alone(B, K, widths, bias):
    x, adj, params = _case(B * 100 + K, B, K, widths, bias)
    leaves = [x, adj] + [t for wb in params for t in wb if t is not None]
    grads = []
    for f in (PG.stack_fwd, _oracle):
        for t in leaves:
            t.requires_grad_(True)
            t.grad = None
        y = f(x, adj, params)
        gen = torch.Generator().manual_seed(3)
        (y * torch.randn(y.shape, generator=gen, dtype=torch.float64)).sum().backward()
        grads.append((y.detach(), [t.grad.clone() for t in leaves]))
    (y_ref, g_ref), (y_or, g_or) = grads
    assert y_ref.shape == (B, K, sum(widths[1:]))
    assert (y_ref - y_or).abs().max().item() <= 1e-12
    for a, b in zip(g_ref, g_or):
        assert (a - b).abs().max().item() <= 1e-12 * max(1.0, b.abs().max().item())


def test_layer_outputs_are_consistent():
    x, adj, w, b = PG.inputs(5, 2, 20, 12, 8)
    agg, v, rinv, mean, rstd, y = PG.layer_fwd(x, adj, w, b, True)
    u = agg @ w + b
    assert torch.allclose(v, u * rinv.unsqueeze(2)) and torch.allclose(v.norm(dim=2), torch.ones(2, 20, dtype=torch.float64))
    assert torch.allclose(y, (torch.relu(v) - mean.unsqueeze(2)) * rstd.unsqueeze(2))
    assert y.mean(dim=2).abs().max().item() < 1e-12
    last = PG.layer_fwd(x, adj, w, None, False)
    assert last[3] is None and last[4] is None and last[5] is last[1]
