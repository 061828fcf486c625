"""pyg.dense_diff_pool and its assignment kernels against float64 restatements, at the edges where they can go wrong: the softmax /
entropy kernels across the 64-lane wave loop, with shifted, near one-hot and masked rows and strided operands; the operator at
BASELINE config 5 (the batched-products contraction) and at a size that takes csrc/contract.hip; and the closed-form link loss where
||adj||^2 - 2 tr(s^T adj s) + ||s^T s||^2 cancels.  Every tolerance is relative to the fp64 result's scale: max|hip - ref| <= tol *
scale.  The references run on the CPU."""
import math

import pytest
import torch

from oracle import pyg_ref as P
from util_graphs import dense_batch

pytestmark = pytest.mark.gpu

EPS32 = 2.0 ** -23
SENTINEL = 7.25           # fills what a kernel must not write (padding columns of strided outputs)


def _err(got, ref, scale=None):
    """max|got - ref| / scale (default: max|ref|) in float64, on the CPU"""
    got, ref = got.detach().cpu().double(), ref.detach().cpu().double()
    scale = ref.abs().max().item() if scale is None else float(scale)
    return (got - ref).abs().max().item() / max(scale, 1e-300)


def _grads(loss, inputs, retain=True):
    gs = torch.autograd.grad(loss, inputs, retain_graph=retain, allow_unused=True)
    return [g if g is not None else torch.zeros_like(t) for g, t in zip(gs, inputs)]


# ----------------------------------------------------------------------------- a. assignment softmax + entropy kernels
def _logits(kind, rows, K, seed):
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn(rows, K, generator=gen)
    if kind == "shifted":                     # the max subtraction: exp(x) alone overflows
        return 50.0 * x + 1e4
    if kind == "onehot":                      # near one-hot rows: gaps of 20 (s ~ 2e-9), 35 (s ~ eps), 90 (fp32 denormal), 120 (s -> 0)
        hot = torch.randint(0, K, (rows,), generator=gen)
        gap = torch.tensor([20.0, 35.0, 90.0, 120.0, 0.0])[torch.arange(rows) % 5]
        return 0.5 * x + gap[:, None] * torch.nn.functional.one_hot(hot, K)
    return 3.0 * x


def _row_mask(kind, rows, seed):
    """None, or 0/1 per row with the rows of block 1 (rows 4-7) all masked and a random quarter of the others"""
    if kind == "shifted":
        return None
    gen = torch.Generator().manual_seed(seed + 1)
    m = (torch.rand(rows, generator=gen) > 0.25).float()
    m[4:8] = 0.0
    return m


def _softmax_ent_ref(x, mask, eps, ds, g):
    """fp64: s = softmax(x) * mask, the per-row entropy terms h = -sum_k s log(s + eps), and d(<s, ds> + g sum(h)) / dx, with the
    scales the kernels' rounding is measured against"""
    xd = x.double().requires_grad_(True)
    s = torch.softmax(xd, -1)
    if mask is not None:
        s = s * mask.double()[:, None]
    lg = torch.log(s + eps)
    h = -(s * lg).sum(-1)
    dx, = torch.autograd.grad((s * ds.double()).sum() + g * h.sum(), xd)
    s, lg = s.detach(), lg.detach()
    # the gradient arriving at the softmax, and the size of the terms its backward s * (dv - <s, dv>) subtracts
    m = mask.double()[:, None] if mask is not None else 1.0
    dv = (ds.double() - g * (lg + s / (s + eps))) * m
    dx_scale = (s * (dv.abs() + (s * dv.abs()).sum(-1, keepdim=True))).max().item()
    h_scale = (s * (lg.abs() + 1.0)).sum(-1)                  # log's absolute rounding is ~eps32 even where log(s + eps) ~ 0
    return s, h, dx, dx_scale, h_scale


def softmax_ent_kernel_errors(K, kind, rows=37, seed=0):
    """tsgnn_row_softmax_ent_{fwd,bwd}_f32 through nat.call with four different row strides (ldx = K + 3, ldy = K + 1,
    ldds = K + 2, lddx = K + 5; NaN in the input padding, a sentinel in the output padding) -> {what: error / scale}"""
    from two_stage_gnn_amd import _native as nat
    eps, g_ent, g_scale = 1e-15, 0.7, 0.25
    x = _logits(kind, rows, K, seed)
    mask = _row_mask(kind, rows, seed)
    ds = torch.randn(rows, K, generator=torch.Generator().manual_seed(seed + 2))
    s_ref, h_ref, dx_ref, dx_scale, h_scale = _softmax_ent_ref(x, mask, eps, ds, g_ent * g_scale)
    ldx, ldy, ldds, lddx = K + 3, K + 1, K + 2, K + 5
    xb = torch.full((rows, ldx), float("nan")); xb[:, :K] = x
    dsb = torch.full((rows, ldds), float("nan")); dsb[:, :K] = ds
    xb, dsb = xb.cuda(), dsb.cuda()
    m = mask.cuda() if mask is not None else None
    nblk = (rows + 3) // 4
    y = torch.full((rows, ldy), SENTINEL, device="cuda")
    hpart = torch.full((nblk,), SENTINEL, device="cuda")
    dx = torch.full((rows, lddx), SENTINEL, device="cuda")
    nat.call("row_softmax_ent_fwd_f32", xb, ldx, rows, K, m, eps, y, ldy, hpart)
    nat.call("row_softmax_ent_bwd_f32", y, ldy, dsb, ldds, m, torch.tensor([g_ent], device="cuda"), g_scale, eps, rows, K, dx, lddx)
    y, hpart, dx = y.cpu(), hpart.cpu(), dx.cpu()
    assert torch.isfinite(y[:, :K]).all() and torch.isfinite(hpart).all() and torch.isfinite(dx[:, :K]).all()
    assert (y[:, K:] == SENTINEL).all() and (dx[:, K:] == SENTINEL).all(), "a kernel wrote past column K"
    pad = nblk * 4 - rows
    hblk_ref = torch.cat([h_ref, h_ref.new_zeros(pad)]).view(nblk, 4).sum(-1)
    hblk_scale = torch.cat([h_scale, h_scale.new_zeros(pad)]).view(nblk, 4).sum(-1)
    if mask is not None:
        off = mask == 0
        assert off[4:8].all() and (hpart[1] == 0).item(), "a fully masked block's entropy must be exactly 0"
        assert (y[off, :K] == 0).all() and (dx[off, :K] == 0).all(), "masked rows: s = 0 and dlogits = 0 exactly"
    return {"s": _err(y[:, :K], s_ref, max(s_ref.abs().max().item(), 1e-30)),
            "hpart": _err(hpart, hblk_ref, hblk_scale.max().item()),
            "h": _err(hpart.double().sum(), h_ref.sum(), h_scale.sum().item()),
            "dlogits": _err(dx[:, :K], dx_ref, max(dx_scale, 1e-30))}


SOFTMAX_TOL = {"s": 2e-6, "hpart": 1e-6, "h": 1e-6, "dlogits": 1e-6}


@pytest.mark.parametrize("kind", ["plain", "shifted", "onehot"])
@pytest.mark.parametrize("K", [1, 2, 63, 64, 65, 128, 200])
def test_row_softmax_entropy_kernels(K, kind):
    """below, at and across the 64-lane loop; 37 rows (the last block of four is partial); strided operands; shifted logits
    (mask None), near one-hot rows with underflowing s, fully masked rows and a fully masked block"""
    err = softmax_ent_kernel_errors(K, kind, seed=K)
    bad = {k: v for k, v in err.items() if not v <= SOFTMAX_TOL[k]}
    assert not bad, "K=%d %s: %s" % (K, kind, err)


@pytest.mark.parametrize("K,masked", [(65, True), (64, False), (5, True)])
def test_softmax_entropy_autograd_node(K, masked):
    """pyg._SoftmaxEntropy (the contiguous path dense_diff_pool takes): s, the entropy numerator and d logits of <s, ds> + g h"""
    from two_stage_gnn_amd import pyg
    rows, eps, g = 4 * 13 + 2, 1e-15, 0.3
    x = _logits("plain", rows, K, 5)
    mask = _row_mask("plain", rows, 5) if masked else None
    ds = torch.randn(rows, K, generator=torch.Generator().manual_seed(6))
    s_ref, h_ref, dx_ref, dx_scale, h_scale = _softmax_ent_ref(x, mask, eps, ds, g)
    xg = x.cuda().requires_grad_(True)
    s, h = pyg._SoftmaxEntropy.apply(xg, mask.cuda() if masked else None, eps)
    dx, = torch.autograd.grad((s * ds.cuda()).sum() + g * h, xg)
    assert _err(s, s_ref, 1.0) <= 2e-6
    assert _err(h, h_ref.sum(), h_scale.sum().item()) <= 1e-6
    assert _err(dx, dx_ref, dx_scale) <= 1e-6


# ----------------------------------------------------------------------------- b. dense_diff_pool against fp64
def _diffpool_inputs(seed, B, N, K, F, sizes, p_edge):
    """random symmetric 0/1 adjacency inside each graph's `sizes[b]` nodes (nothing outside), features, logits, row mask"""
    x, adj, sizes = dense_batch(seed, B, N, F, sizes=sizes, p_edge=p_edge)
    s = 2.0 * torch.randn(B, N, K, generator=torch.Generator().manual_seed(seed + 1))
    mask = torch.arange(N)[None, :] < torch.as_tensor(sizes)[:, None]
    return x, adj, s, mask


def diffpool_errors(x, adj, s, mask, adj_grad=False, seed=0):
    """pyg.dense_diff_pool against oracle.pyg_ref.dense_diff_pool on float64 inputs: the four outputs and, separately, the gradients
    of (random projections of out and out_adj), link and ent w.r.t. x, s (and adj) -> {what: error / scale}"""
    from two_stage_gnn_amd import pyg
    B, N, K = s.shape
    gen = torch.Generator().manual_seed(seed + 7)
    gx, ga = torch.randn(B, K, x.size(2), generator=gen), torch.randn(B, K, K, generator=gen)
    names = ["x", "s"] + (["adj"] if adj_grad else [])

    def run(xx, aa, ss, mm, pw):
        ins = [xx.requires_grad_(True), ss.requires_grad_(True)] + ([aa.requires_grad_(True)] if adj_grad else [])
        out, out_adj, link, ent = pw(xx, aa, ss, mm)
        proj = (out * gx.to(out)).sum() + (out_adj * ga.to(out)).sum()
        return [out, out_adj, link, ent], [_grads(t, ins) for t in (proj, link, ent)]

    o_g, g_g = run(x.cuda(), adj.cuda(), s.cuda(), mask.cuda(), pyg.dense_diff_pool)
    o_r, g_r = run(x.double(), adj.double(), s.double(), mask, P.dense_diff_pool)
    err = {name: _err(a, b) for name, a, b in zip(("out", "out_adj", "link", "ent"), o_g, o_r)}
    for term, gg, gr in zip(("proj", "link", "ent"), g_g, g_r):
        for name, a, b in zip(names, gg, gr):
            assert torch.isfinite(a).all(), "d %s / d %s not finite" % (term, name)
            if b.abs().max().item() > 0:
                err["d%s/d%s" % (term, name)] = _err(a, b)
            else:
                assert (a == 0).all(), "d %s / d %s must be 0" % (term, name)
    return err


DIFFPOOL_TOL = {"out": 1e-5, "out_adj": 1e-5, "link": 1e-6, "ent": 1e-6}
DIFFPOOL_GRAD_TOL = 1e-5


def _check_diffpool(err):
    bad = {k: v for k, v in err.items() if not v <= DIFFPOOL_TOL.get(k, DIFFPOOL_GRAD_TOL)}
    assert not bad, str(err)


def test_dense_diff_pool_config5_batched_products(monkeypatch):
    """BASELINE config 5 (B = 16, N = 512, K = 64, F = 64) with graphs of 100-512 nodes: N > 256 takes the batched products, not
    csrc/contract.hip.  The random adjacency keeps d2 far from 0: the link loss holds 1e-6 relative."""
    from two_stage_gnn_amd import _native as nat
    B, N, K, F = 16, 512, 64, 64
    sizes = torch.randint(100, N + 1, (B,), generator=torch.Generator().manual_seed(3))
    sizes[0], sizes[5] = N, 100
    assert not nat.lib().tsgnn_contract_dense_supported(N, K, F)
    trace = []
    monkeypatch.setattr(nat, "trace", trace)
    err = diffpool_errors(*_diffpool_inputs(11, B, N, K, F, sizes.tolist(), 0.05), seed=1)
    assert not [t for t in trace if t[0].startswith("contract_dense")]
    _check_diffpool(err)


def test_dense_diff_pool_fused_contraction(monkeypatch):
    """a size csrc/contract.hip takes (N <= 256; K, F not multiples of 8), ragged graphs down to one node, adj requiring grad"""
    from two_stage_gnn_amd import _native as nat, diffpool as dp
    B, N, K, F = 5, 120, 20, 36
    assert nat.lib().tsgnn_contract_dense_supported(N, K, F)
    monkeypatch.setattr(dp, "FUSED_CONTRACT", True)
    trace = []
    monkeypatch.setattr(nat, "trace", trace)
    err = diffpool_errors(*_diffpool_inputs(12, B, N, K, F, [120, 33, 1, 77, 100], 0.1), adj_grad=True, seed=2)
    ran = {t[0] for t in trace}
    assert {"contract_dense_fwd_ro_f32", "contract_dense_bwd_ro_f32"} <= ran, ran
    _check_diffpool(err)


# ----------------------------------------------------------------------------- c. the link loss where its closed form cancels
# (B, N, K, per-graph clique sizes): one clique per cluster, unequal sizes, masked tails, empty clusters, B N^2 not a multiple of 4,
# N > 256 (batched products)
LAYOUTS = {"equal": (2, 48, 6, [[8] * 6, [8] * 6]),
           "unequal_tail": (2, 48, 8, [[1, 5, 17, 3, 22], [30, 2, 9]]),
           "wide_k": (3, 64, 16, [[40, 7], [13, 13, 13, 1], [64]]),
           "odd_n": (3, 45, 8, [[20, 5, 3], [44], [1, 2, 3, 4, 5, 6, 7]]),
           "batched": (2, 300, 8, [[100, 50, 150], [7, 280]])}


def clique_inputs(layout, logit, seed=0):
    """adj = block-diagonal cliques with self loops, s = logit * one-hot(clique label) (+ nothing else), rows past the last clique
    masked.  s s^T reproduces adj as the logit grows."""
    B, N, K, cliques = LAYOUTS[layout]
    adj, s, mask = torch.zeros(B, N, N), torch.zeros(B, N, K), torch.zeros(B, N, dtype=torch.bool)
    for b, sizes in enumerate(cliques):
        off = 0
        for c, n in enumerate(sizes):
            adj[b, off:off + n, off:off + n] = 1.0
            s[b, off:off + n, c] = logit
            off += n
        mask[b, :off] = True
    x = torch.randn(B, N, 16, generator=torch.Generator().manual_seed(seed))
    return x, adj, s, mask


def link_bound(adj, s, mask):
    """8 sqrt(eps32 (||adj||^2 + 2 |tr(s^T adj s)| + ||s^T s||^2)) / numel from fp64 values: the operator's documented bound"""
    sd = torch.softmax(s.double(), -1) * mask.double()[..., None]
    a = adj.double()
    tr = torch.diagonal(sd.transpose(1, 2) @ a @ sd, dim1=1, dim2=2).sum()
    G = sd.transpose(1, 2) @ sd
    return 8.0 * math.sqrt(EPS32 * ((a * a).sum() + 2.0 * tr.abs() + (G * G).sum()).item()) / adj.numel()


def _link64(x, adj, s, mask):
    sd = s.double().requires_grad_(True)
    link = P.dense_diff_pool(x.double(), adj.double(), sd, mask)[2]
    return link.item(), torch.autograd.grad(link, sd)[0]


@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_link_loss_exact_cancellation(layout):
    """logit 60: s is exactly 1.0 on the clique's cluster and ~1e-26 elsewhere, so the three sums are integers (the off-cluster
    products underflow) and d2 is exactly 0.  The link loss is 0 (within the bound of fp64's 1e-28), every gradient is finite, and
    the link term passes no gradient: the gradients with and without it in the loss are identical."""
    from two_stage_gnn_amd import pyg
    x, adj, s, mask = clique_inputs(layout, 60.0)
    xg, sg = x.cuda().requires_grad_(True), s.cuda().requires_grad_(True)
    out, out_adj, link, ent = pyg.dense_diff_pool(xg, adj.cuda(), sg, mask.cuda())
    assert link.dtype == torch.float32 and link.dim() == 0
    assert abs(link.item() - _link64(x, adj, s, mask)[0]) <= link_bound(adj, s, mask)
    assert link.item() == 0.0, "d2 should cancel exactly here (integer sums)"
    base = 1e-3 * ((out ** 2).sum() + (out_adj ** 2).sum()) + ent
    g_with, g_without = _grads(base + link, [xg, sg]), _grads(base, [xg, sg])
    for a, b in zip(g_with, g_without):
        assert torch.isfinite(a).all()
        assert torch.equal(a, b)
    assert (_grads(link, [sg])[0] == 0).all()
    # the same adjacency 4 bytes past a 16-byte boundary: the reduction's scalar path, the same integer sums
    a_odd = torch.zeros(adj.numel() + 1, device="cuda")[1:].view(adj.shape).copy_(adj.cuda())
    assert pyg.dense_diff_pool(xg, a_odd, sg, mask.cuda())[2].item() == 0.0


@pytest.mark.parametrize("logit", [3.0, 4.0, 5.0, 6.0, 8.0, 12.0])
@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_link_loss_near_cancellation(layout, logit):
    """adj - s s^T small but not 0: |link - link64| within the documented absolute bound; where link64 is at least 10x that bound,
    the link loss's gradient matches fp64 to 1e-3 of its scale"""
    from two_stage_gnn_amd import pyg
    x, adj, s, mask = clique_inputs(layout, logit)
    bound = link_bound(adj, s, mask)
    l64, g64 = _link64(x, adj, s, mask)
    sg = s.cuda().requires_grad_(True)
    link = pyg.dense_diff_pool(x.cuda(), adj.cuda(), sg, mask.cuda())[2]
    assert abs(link.item() - l64) <= bound, (link.item(), l64, bound)
    gs, = _grads(link, [sg])
    assert torch.isfinite(gs).all()
    if l64 >= 10.0 * bound:
        assert _err(gs, g64) <= 1e-3


def test_link_loss_graph_replay_matches_eager():
    """forward + backward of the exact-cancellation input captured in one hipGraph: the replay is finite and bitwise the eager
    result (the guard of the link loss is a device-side select, nothing reads d2 on the host)"""
    from two_stage_gnn_amd import pyg
    x, adj, s, mask = clique_inputs("unequal_tail", 60.0)
    xg, sg = x.cuda().requires_grad_(True), s.cuda().requires_grad_(True)
    ag, mg = adj.cuda(), mask.cuda()

    def step():
        out, out_adj, link, ent = pyg.dense_diff_pool(xg, ag, sg, mg)
        loss = 1e-3 * ((out ** 2).sum() + (out_adj ** 2).sum()) + link + ent
        return [loss, link, ent] + list(torch.autograd.grad(loss, [xg, sg]))

    st = torch.cuda.Stream()
    st.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(st):
        for _ in range(2):
            step()
        torch.cuda.synchronize()
        gr = torch.cuda.CUDAGraph()
        with torch.cuda.graph(gr, stream=st):
            static = step()
        gr.replay()
        torch.cuda.synchronize()
        replayed = [t.clone() for t in static]
        eager = step()
        torch.cuda.synchronize()
    assert replayed[1].item() == 0.0
    for a, b in zip(replayed, eager):
        assert torch.isfinite(a).all()
        assert torch.equal(a, b)
