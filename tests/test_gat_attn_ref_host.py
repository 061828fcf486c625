"""tests/gat_attn_ref.py (the float64 reference of the fused GAT attention kernels) tied to the pinned oracle
oracle/dense_ref.gat_layer, on the CPU, in float64 to 1e-12 * max; and the guarantees of the seeded inputs that
tests/test_gpu_gat_attn_kernels.py feeds to the kernels."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import gat_attn_ref as G
from fp32_yardstick import K_DEFAULT, _yardstick
from oracle import dense_ref as R

TOL = 1e-12
SLOPE = 0.2


def _close(what, got, ref):
    err = (got - ref).abs().max().item()
    assert got.shape == ref.shape and err <= TOL * ref.abs().max().item(), (what, err, ref.abs().max().item())


def _oracle_case(H, Fo, fin=7, N=14, n=11, seed=0):
    """B = 1: n real nodes (node 4 isolated), N - n padded slots; non-symmetric adjacency"""
    gen = torch.Generator().manual_seed(seed)
    adj = torch.zeros(1, N, N, dtype=torch.float64)
    a = (torch.rand(n, n, generator=gen) < 0.3).double() * (1 - torch.eye(n, dtype=torch.float64))
    a[4, :] = 0
    a[:, 4] = 0
    adj[0, :n, :n] = a
    x = torch.randn(1, N, fin, dtype=torch.float64, generator=gen)
    ws = [torch.randn(fin, Fo, dtype=torch.float64, generator=gen) * 0.5 for _ in range(H)]
    as_ = [torch.randn(2 * Fo, 1, dtype=torch.float64, generator=gen) * 0.5 for _ in range(H)]
    mult = [(torch.rand(1, N, N, generator=gen) >= 0.3).double() / 0.7 for _ in range(H)]
    gy = torch.randn(N, H * Fo, dtype=torch.float64, generator=gen)
    return x, adj, [n], ws, as_, mult, gy


@pytest.mark.parametrize("with_mult", [False, True], ids=["nodrop", "att_mult"])
@pytest.mark.parametrize("concat", [True, False], ids=["concat", "mean"])
@pytest.mark.parametrize("H,Fo", [(3, 4), (1, 8), (4, 5)])
def test_reference_equals_pinned_oracle(H, Fo, concat, with_mult):
    """with hp = x . pack(w, a): attn_fwd == oracle.dense_ref.gat_layer, and the gradients with respect to x, w, a — ours through
    attn_bwd, the two products of the projection and unpack — equal the oracle's autograd"""
    x, adj, sizes, ws, as_, mult, gy = _oracle_case(H, Fo, seed=H * 10 + Fo)
    mult = mult if with_mult else None
    Co = H * Fo if concat else Fo
    gy = gy[:, :Co]
    # the oracle
    p = {}
    leaves = [x.clone().requires_grad_(True)]
    for h in range(H):
        p["l.attention_%d.w" % h] = ws[h].clone().requires_grad_(True)
        p["l.attention_%d.a" % h] = as_[h].clone().requires_grad_(True)
        leaves += [p["l.attention_%d.w" % h], p["l.attention_%d.a" % h]]
    yo = R.gat_layer(p, "l", leaves[0], adj, concat, SLOPE, att_mult=mult)
    go = torch.autograd.grad((yo[0] * gy).sum(), leaves)
    # the reference at the kernels' boundary
    L = G.Layout(adj, sizes, "padded")
    wp = G.pack(ws, as_)
    assert wp.shape == (x.size(2), G.packed_width(H, Fo))
    hp = x[0] @ wp
    y = G.attn_fwd(hp, L, H, Fo, SLOPE, not concat, True, mult)
    _close("y", y, yo[0].detach())
    dhp, _ = G.attn_bwd(hp, L, H, Fo, SLOPE, not concat, True, y, dy=gy, mult=mult)
    _close("dx", dhp @ wp.t(), go[0][0])
    gw, ga = G.unpack(x[0].t() @ dhp, ws, as_)
    for h in range(H):
        _close("gw[%d]" % h, gw[h], go[1 + 2 * h])
        _close("ga[%d]" % h, ga[h], go[2 + 2 * h].reshape(-1))


@pytest.mark.parametrize("mean_heads,apply_elu", [(False, True), (True, True), (False, False)])
@pytest.mark.parametrize("name", ["edges", "blocks33"])
def test_ghost_layout_equals_padded_layout(name, mean_heads, apply_elu):
    """one representative row per graph == its Nmax - n_b copies: y on the real rows, the representative's y on every padded slot,
    and the gradients of the copies summed"""
    H, Fh = 3, 8
    Lg, Lp = G.layout(name, "ghost1"), G.layout(name, "padded")
    Ns = G.packed_width(H, Fh)
    hp_g = G.make_hp(Lg, H, Fh, Ns, 77).double()
    hp_p = Lg.expand(hp_g).reshape(Lp.R, Ns)
    y_g = G.attn_fwd(hp_g, Lg, H, Fh, SLOPE, mean_heads, apply_elu)
    y_p = G.attn_fwd(hp_p, Lp, H, Fh, SLOPE, mean_heads, apply_elu)
    _close("y", Lg.expand(y_g).reshape(Lp.R, -1), y_p)
    gen = torch.Generator().manual_seed(5)
    dy_g = torch.randn(y_g.shape, dtype=torch.float64, generator=gen)
    dy_p = torch.zeros_like(y_p).index_copy_(0, Lg.rep_slot, dy_g)
    d_g, S_g = G.attn_bwd(hp_g, Lg, H, Fh, SLOPE, mean_heads, apply_elu, y_g, dy=dy_g)
    d_p, S_p = G.attn_bwd(hp_p, Lp, H, Fh, SLOPE, mean_heads, apply_elu, y_p, dy=dy_p)
    _close("dhp", d_g, torch.zeros_like(d_g).index_add_(0, Lg.slot_row.reshape(-1), d_p))
    _close("S", S_g, S_p.index_select(0, Lg.rep_slot))
    # the readout form is the same gradient
    arg = torch.from_numpy(Lg.graph_ptr[:-1]).unsqueeze(1) + (torch.rand(Lg.B, y_g.size(1), generator=gen) *
                                                                torch.from_numpy(Lg.rows_per_graph).unsqueeze(1)).long()
    dout = torch.randn(Lg.B, y_g.size(1), dtype=torch.float64, generator=gen)
    d_r, _ = G.attn_bwd(hp_g, Lg, H, Fh, SLOPE, mean_heads, apply_elu, y_g, ro_arg=arg.to(torch.int32), ro_dout=dout)
    d_d, _ = G.attn_bwd(hp_g, Lg, H, Fh, SLOPE, mean_heads, apply_elu, y_g, dy=G.readout_dy(Lg, arg, dout))
    assert torch.equal(d_r, d_d) and G.readout_dy(Lg, arg, dout).ne(0).sum().item() > 0


@pytest.mark.parametrize("H,Fin,Fo", [(1, 1, 4), (3, 13, 8), (8, 5, 16)])
def test_unpack_equals_autograd_through_pack(H, Fin, Fo):
    gen = torch.Generator().manual_seed(H + Fin)
    ws = [torch.randn(Fin, Fo, dtype=torch.float64, generator=gen).requires_grad_(True) for _ in range(H)]
    as_ = [torch.randn(2 * Fo, dtype=torch.float64, generator=gen).requires_grad_(True) for _ in range(H)]
    wp = G.pack(ws, as_, Ns=G.packed_width(H, Fo) + 4)
    assert not wp[:, H * Fo + 2 * H:].any()
    dwp = torch.randn(wp.shape, dtype=torch.float64, generator=gen)
    grads = torch.autograd.grad((wp * dwp).sum(), ws + as_)
    gw, ga = G.unpack(dwp, [w.detach() for w in ws], [a.detach() for a in as_])
    for h in range(H):
        _close("gw[%d]" % h, gw[h], grads[h])
        _close("ga[%d]" % h, ga[h], grads[H + h])


def test_col_stats_are_the_softmax_statistics():
    """exp(e - m) / Z over a column's entries == the dense softmax's column; edge-less columns give (0, 0)"""
    H, Fh = 3, 8
    L = G.layout("edges", "padded")
    hp = G.inputs("edges", "padded", H, Fh)[1].double()
    m, rz = G.col_stats(hp, L, H, Fh, SLOPE)
    _, atts = G.attn_dense(hp, L, H, Fh, SLOPE, False, False)
    d = L.expand(hp)
    C = H * Fh
    deg_t = L.mask.sum(dim=1).reshape(-1)
    assert (m[deg_t == 0] == 0).all() and (rz[deg_t == 0] == 0).all() and (rz[deg_t > 0] > 0).all()
    for h in range(H):
        e = F.leaky_relu(d[:, :, C + h].unsqueeze(2) + d[:, :, C + H + h].unsqueeze(1), SLOPE)
        alpha = torch.exp(e - m[:, h].reshape(L.B, 1, L.N)) * rz[:, h].reshape(L.B, 1, L.N) * L.mask
        _close("alpha", alpha, atts[h] * L.mask * (deg_t > 0).reshape(L.B, 1, L.N))


def test_edges_batch_has_the_degrees_it_promises():
    adj, sizes = G.batch("edges")
    assert adj.size(1) == G.EDGES_NMAX <= 96 and sizes.tolist() == [G.EDGES_NMAX, 1, 6, 76, 12]
    assert G.layout("edges", "ghost1").R <= 400 and G.layout("edges", "padded").R <= 400
    row_deg, col_deg = adj.sum(dim=2), adj.sum(dim=1)
    assert not adj[2].any()                                                  # a graph without any edge
    assert adj[1].sum().item() == 1 and adj[1, 0, 0] == 1                    # the 1-node graph
    assert row_deg[4, 5] == 0 and col_deg[4, 5] == 0 and row_deg[4, :12].gt(0).sum() >= 8       # an isolated real node
    hub = adj[G.HUB]
    assert not torch.equal(hub, hub.t())
    assert row_deg[G.HUB, 0] == 70 and col_deg[G.HUB, 75] == 70 and col_deg[G.HUB, 0] == 0 and row_deg[G.HUB, 75] == 0
    assert row_deg[G.HUB, 2:8].tolist() == list(G.HUB_DEGREES) and col_deg[G.HUB, 10:16].tolist() == list(G.HUB_DEGREES)
    # the padded layout's edge-less columns can still be listed by the product (attention._isolated_list: at most 64 per graph on average)
    assert int((col_deg == 0).sum()) <= 64 * adj.size(0)


@pytest.mark.parametrize("B", G.BLOCKS_B)
def test_blocks_batches_mix_empty_and_listed_graphs(B):
    adj, sizes = G.batch("blocks%d" % B)
    assert adj.shape == (B, G.BLOCKS_NMAX, G.BLOCKS_NMAX) and sizes.min() >= 1 and sizes.max() <= G.BLOCKS_NMAX
    col_deg = adj.sum(dim=1)
    listed = (col_deg == 0).sum(dim=1)                                       # padded layout: edge-less columns per graph
    if B > 1:
        assert (listed == 0).any() and (listed > 0).any()                    # an empty list next to listed ones
        assert set(sizes.tolist()) == set(range(1, 7))
        assert any(not adj[b].any() for b in range(B))                       # a graph without any edge
    Lg = G.layout("blocks%d" % B, "ghost1")
    P = max(1, min(8, 256 // B))
    assert (Lg.rows_per_graph < P).any() or P == 1                            # graphs with fewer rows than parts


def test_inputs_keep_their_margin_from_the_kink():
    """min |s_row[i] + s_col[j]| >= 1e-3 over all entries of every input of the GPU module: neither the fp32 sum nor a kernel's
    differently rounded one can take the other branch of LeakyReLU; the extreme inputs really span +-60"""
    keys = G.input_keys()
    assert len(set(keys)) == len(keys) >= 40
    for key in keys:
        L, hp, Ns = G.inputs(*key)
        H, Fh = key[2], key[3]
        C = H * Fh
        assert hp.dtype == torch.float32 and hp.shape == (L.R, Ns) and Ns % 4 == 0 and torch.isfinite(hp).all()
        assert not hp[:, C + 2 * H:].any()
        assert G.score_margin(hp, L, H, Fh) >= G.MARGIN, key
        if key[5]:
            i, j = L.entries()
            t = hp[i, C:C + H] + hp[j, C + H:C + 2 * H]
            assert t.max().item() > 50 and t.min().item() < -50


def test_dropped_softmax_term_is_seen():
    """sensitivity of the tolerance scheme, on the CPU: d s_col[j] = sum_i lrelu'_ij att_ij (datt_ij - S_j) written out by hand
    equals autograd; the same line WITHOUT the  - S_j  term (a mutated copy — the kernels are not touched) misses the reference by
    thousands of yardsticks, far beyond K = 8"""
    H, Fh = 3, 8
    C = H * Fh
    L, hp32, Ns = G.inputs("edges", "ghost1", H, Fh)
    gen = torch.Generator().manual_seed(9)
    dy = torch.randn(L.R, C, generator=gen)
    y32 = G.attn_fwd(hp32, L, H, Fh, SLOPE, False, True)
    d64, S64 = G.attn_bwd(hp32.double(), L, H, Fh, SLOPE, False, True, y32, dy=dy)
    d32, _ = G.attn_bwd(hp32, L, H, Fh, SLOPE, False, True, y32, dy=dy)
    yard = _yardstick(d64[:, C + H:C + 2 * H], d32[:, C + H:C + 2 * H])

    def dscol(mutated):
        hp = hp32.double().requires_grad_(True)
        y, atts = G.attn_dense(hp, L, H, Fh, SLOPE, False, True, None, y32)
        datts = torch.autograd.grad((dy.double() * y).sum(), atts)
        d = L.expand(hp.detach())
        out = []
        for h in range(H):
            t = d[:, :, C + h].unsqueeze(2) + d[:, :, C + H + h].unsqueeze(1)
            lr = torch.where(t > 0, torch.ones_like(t), torch.full_like(t, SLOPE)) * L.mask
            att, datt = atts[h].detach(), datts[h]
            S = (att * datt * L.mask).sum(dim=1, keepdim=True)
            P1, P2 = (lr * att * datt).sum(dim=1), (lr * att).sum(dim=1)
            out.append(P1 if mutated else P1 - S[:, 0] * P2)                       # [B, N] per padded slot
        per_slot = torch.stack(out, dim=2).reshape(L.B * L.N, H)
        return torch.zeros(L.R, H, dtype=torch.float64).index_add_(0, L.slot_row.reshape(-1), per_slot)

    ref = d64[:, C + H:C + 2 * H]
    assert (dscol(False) - ref).abs().max().item() <= 1e-12 * ref.abs().max().item()
    moved = (dscol(True) - ref).abs().max().item() / yard
    print("d s_col without the - S P2 term: %.0f yardsticks" % moved)
    assert moved > 100 * K_DEFAULT
