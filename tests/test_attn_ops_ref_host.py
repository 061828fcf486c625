"""tests/attn_ops_ref.py (the float64 reference of the composed GAT attention kernels, csrc/attention.hip) tied on the CPU to what the
project already trusts — tests/gat_attn_ref.attn_dense, oracle/dense_ref.gat_layer, oracle/pyg_ref.gat_conv and float64 autograd —, the
guarantees of the seeded inputs that tests/test_gpu_attn_ops.py feeds to the kernels, the argument checks of the 18 entry points, and
the entry map of a graph without any edge (attention._inverse_entry_map)."""
import types

import pytest
import torch

import attn_ops_ref as A
import gat_attn_ref as G
from oracle import dense_ref, pyg_ref

TOL = 1e-12
SLOPE = 0.2
EINVAL = -1


def _close(what, got, ref, tol=TOL):
    err = (got - ref).abs().max().item() if ref.numel() else 0.0
    assert got.shape == ref.shape and err <= tol * max(ref.abs().max().item(), 1e-300), (what, err)


# ----------------------------------------------------------------------------- the entry map of a graph without any edge
def test_inverse_entry_map_never_indexes_with_the_placeholder_word():
    """nnz = 0: src_e_t is one placeholder word, whatever it holds; the map is a zero-filled word and nothing is indexed"""
    from two_stage_gnn_amd import attention as att
    g = types.SimpleNamespace(nnz=0)
    inv = att._inverse_entry_map(g, torch.tensor([123456789], dtype=torch.int32))
    assert inv.dtype == torch.int32 and inv.tolist() == [0]
    assert att._inverse_entry_map(g, torch.tensor([5], dtype=torch.int32)) is inv


def test_inverse_entry_map_inverts_a_permutation_and_caches_it():
    from two_stage_gnn_amd import attention as att
    g = types.SimpleNamespace(nnz=5)
    src = torch.tensor([3, 0, 4, 1, 2], dtype=torch.int32)
    inv = att._inverse_entry_map(g, src)
    assert inv.dtype == torch.int32 and inv.tolist() == [1, 3, 4, 0, 2] and src[inv.long()].tolist() == list(range(5))
    assert att._inverse_entry_map(g, torch.zeros(5, dtype=torch.int32)) is inv
    # a buffer longer than nnz (a pooled allocation): only the first nnz words count
    g2 = types.SimpleNamespace(nnz=3)
    assert att._inverse_entry_map(g2, torch.tensor([2, 0, 1, 99], dtype=torch.int32)).tolist() == [1, 2, 0]


# ----------------------------------------------------------------------------- by column == attn_dense == dense_ref.gat_layer
def _uniform(L):
    return (torch.from_numpy(L.row_mult), torch.from_numpy(L.row_graph), torch.from_numpy(L.graph_ptr), L.N)


@pytest.mark.parametrize("mean_heads,apply_elu", [(False, True), (True, True), (False, False)])
@pytest.mark.parametrize("kind", G.KINDS)
def test_by_column_composition_equals_the_dense_reference(kind, mean_heads, apply_elu):
    H, Fh = 3, 8
    C = H * Fh
    L = G.layout("edges", kind)
    rowptr, col = A.layout_csr(L)
    h, a_row, a_col = (t.double() for t in A.layer_inputs(L, H, Fh, 41))
    y = A.compose(h, a_row, a_col, rowptr, col, H, Fh, SLOPE, True, _uniform(L), None, mean_heads, apply_elu)
    s_row, s_col = A.node_scores2(h, a_row, a_col, H, Fh)
    hp = torch.cat([h, s_row, s_col, h.new_zeros(L.R, G.packed_width(H, Fh) - C - 2 * H)], dim=1)
    _close("y", y, G.attn_fwd(hp, L, H, Fh, SLOPE, mean_heads, apply_elu))


@pytest.mark.parametrize("concat", [True, False])
@pytest.mark.parametrize("kind", G.KINDS)
def test_by_column_composition_equals_the_pinned_oracle(kind, concat):
    """B = 1 (the oracle reads graph 0's features for every graph): the 12-node graph of the edges batch, node 5 isolated, 68 padded
    slots; h = x w_h, a_row / a_col = the halves of a_h"""
    H, Fo, fin = 3, 4, 7
    adj, sizes = G.batch("edges")
    L = G.Layout(adj[4:5], sizes[4:5], kind)
    rowptr, col = A.layout_csr(L)
    gen = torch.Generator().manual_seed(3)
    x = torch.randn(L.R, fin, dtype=torch.float64, generator=gen)
    ws = [torch.randn(fin, Fo, dtype=torch.float64, generator=gen) * 0.5 for _ in range(H)]
    as_ = [torch.randn(2 * Fo, 1, dtype=torch.float64, generator=gen) * 0.5 for _ in range(H)]
    p = {}
    for k in range(H):
        p["l.attention_%d.w" % k], p["l.attention_%d.a" % k] = ws[k], as_[k]
    yo = dense_ref.gat_layer(p, "l", L.expand(x), adj[4:5].double(), concat, SLOPE)
    W, Apk = A.pack_heads(ws, [a.reshape(-1) for a in as_])
    y = A.compose(x @ W, Apk[0], Apk[1], rowptr, col, H, Fo, SLOPE, True, _uniform(L), None, not concat, True)
    _close("y", y, L.rows_of(yo))


# ----------------------------------------------------------------------------- per target == pyg_ref.gat_conv
@pytest.mark.parametrize("drop", [False, True])
@pytest.mark.parametrize("concat", [True, False])
def test_per_target_composition_equals_the_pyg_oracle(concat, drop):
    H, Fh, fin = 3, 4, 6
    L = G.layout("edges", "padded")
    rowptr, col, edge_index, entry_of = A.self_looped(L)
    gen = torch.Generator().manual_seed(4)
    x = torch.randn(L.R, fin, dtype=torch.float64, generator=gen)
    w = torch.randn(H * Fh, fin, dtype=torch.float64, generator=gen) * 0.5
    att_l, att_r = torch.randn(H, Fh, dtype=torch.float64, generator=gen), torch.randn(H, Fh, dtype=torch.float64, generator=gen)
    mult_e = ((torch.rand(edge_index.size(1), H, generator=gen) >= 0.3).double() / 0.7) if drop else None
    yo = pyg_ref.gat_conv(x, edge_index, w, att_l, att_r, None, H, concat, SLOPE, mult_e)
    mult = None
    if drop:                                                     # the oracle's multipliers, in the CSR's entry order
        mult = torch.empty_like(mult_e)
        mult[entry_of.long()] = mult_e
    y = A.compose(x @ w.t(), att_r, att_l, rowptr, col, H, Fh, SLOPE, False, None, mult, not concat, False)
    _close("y", y, yo)


# ----------------------------------------------------------------------------- the backward as attention.py issues it == autograd
def _backward_by_ops(h, a_row, a_col, rowptr, col, H, Fh, slope, by_column, uniform, drop_mult, dout):
    """(dh, da_row, da_col) from the reference functions in the order of _AttentionAggregate.backward"""
    R = rowptr.numel() - 1
    s_row, s_col = A.node_scores2(h, a_row, a_col, H, Fh)
    rp_t, col_t, src_e = A.transpose(rowptr, col, R)
    if by_column:
        alpha_t = A.edge_softmax_fwd(rp_t, col_t, 0, s_col, s_row, slope)
        dalpha_g = A.csr_sddmm_heads(rp_t, col_t, 0, h, dout, H, Fh)
        dt_g, ds_col = A.edge_softmax_bwd(rp_t, col_t, 0, s_col, s_row, slope, dalpha_g)
        ds_row = A.csr_row_sum(rowptr, dt_g, A.inverse(src_e))
    else:
        alpha = A.edge_softmax_fwd(rowptr, col, 0, s_row, s_col, slope)
        dalpha = A.csr_sddmm_heads(rowptr, col, 0, dout, h, H, Fh)
        if drop_mult is not None:
            dalpha, alpha = dalpha * drop_mult, alpha * drop_mult
        dt, ds_row = A.edge_softmax_bwd(rowptr, col, 0, s_row, s_col, slope, dalpha)
        ds_col = A.csr_row_sum(rp_t, A.edge_permute(dt, src_e, False))
        alpha_t = A.edge_permute(alpha, src_e, False)
        # scatter is gather's inverse
        assert torch.equal(A.edge_permute(alpha_t, src_e, True), alpha)
    epi = {}
    if uniform is not None:
        mult, row_graph, graph_ptr, N = uniform
        iso = (((rp_t[1:] - rp_t[:-1]) == 0).to(h.dtype) * mult.to(h.dtype)).unsqueeze(1).expand(R, H)
        epi = dict(u=A.segment_wsum(dout, None, H, Fh, graph_ptr), uw=iso, row_seg=row_graph, uscale=1.0 / N)
    dh = A.csr_spmm_heads(rp_t, col_t, 0, alpha_t, dout, H, Fh, w1=ds_row, a1=a_row, w2=ds_col, a2=a_col, **epi)
    da_row, da_col = A.segment_wsum2(h, ds_row, ds_col, H, Fh, None)
    return dh, da_row.view(H, Fh), da_col.view(H, Fh)


@pytest.mark.parametrize("mode", ["column+uniform", "column", "target", "target+drop"])
@pytest.mark.parametrize("kind", G.KINDS)
def test_backward_by_ops_equals_autograd_of_the_composed_forward(kind, mode):
    H, Fh = 2, 8
    L = G.layout("blocks31", kind)
    rowptr, col = A.layout_csr(L)
    by_column = mode.startswith("column")
    uniform = _uniform(L) if mode == "column+uniform" else None
    gen = torch.Generator().manual_seed(6)
    drop = ((torch.rand(col.numel(), H, generator=gen) >= 0.3).double() / 0.7) if mode == "target+drop" else None
    leaves = [t.double().requires_grad_(True) for t in A.layer_inputs(L, H, Fh, 43)]
    out = A.compose(*leaves, rowptr, col, H, Fh, SLOPE, by_column, uniform, drop, False, False)
    dout = torch.randn(out.shape, dtype=torch.float64, generator=gen)
    want = torch.autograd.grad((out * dout).sum(), leaves)
    got = _backward_by_ops(*[t.detach() for t in leaves], rowptr, col, H, Fh, SLOPE, by_column, uniform, drop, dout)
    for what, a, b in zip(("dh", "da_row", "da_col"), got, want):
        _close(what, a, b, 1e-11)


@pytest.mark.parametrize("cell", A.ELU_CELLS)
def test_elu_backward_is_autograd_and_its_closed_form(cell):
    rows, H, Fh, mean, elu, _ = cell
    x = A.elu_inputs(cell).double()
    dy = A.rnd(1, rows, Fh if mean else H * Fh).double()
    dx = A.elu_heads_bwd(x, dy, H, Fh, mean, elu)
    v = x.reshape(rows, H, Fh).sum(dim=1) / H if mean else x
    d = torch.where(v > 0, torch.ones_like(v), torch.exp(v)) if elu else torch.ones_like(v)
    want = (dy * d / H).unsqueeze(1).expand(rows, H, Fh).reshape(rows, H * Fh) if mean else dy * d
    _close("dx", dx, want)


def test_small_ops_against_plain_loops():
    """segment_wsum (mean, empty segment), gather_wsum, broadcast_add, csr_row_sum with an entry map, pack / unpack: written out as
    python loops on a tiny case"""
    H, Fh, C = 2, 3, 6
    x, w = A.rnd(2, 7, C).double(), A.rnd(3, 7, H).double()
    sp = torch.tensor([0, 0, 3, 7], dtype=torch.int32)
    out = A.segment_wsum(x, w, H, Fh, sp, scale=0.5, mean=True)
    for s, (r0, r1) in enumerate([(0, 0), (0, 3), (3, 7)]):
        for c in range(C):
            want = 0.5 * sum(w[r, c // Fh] * x[r, c] for r in range(r0, r1)) / max(r1 - r0, 1)
            assert abs(out[s, c] - want) < 1e-14
    assert not out[0].any()
    _close("one segment", A.segment_wsum(x, None, H, Fh, None), x.sum(dim=0, keepdim=True))
    idx, wl, lp = torch.tensor([4, 1, 1], dtype=torch.int32), torch.tensor([2.0, 3.0, 0.5], dtype=torch.float64), torch.tensor([0, 1, 1, 3])
    _close("gather_wsum", A.gather_wsum(x, idx, wl, lp, C, 2.0), 2.0 * torch.stack([2.0 * x[4], 0 * x[0], 3.5 * x[1]]))
    a, u = A.rnd(4, H, Fh).double(), A.rnd(5, 3, C).double()
    y0 = A.broadcast_add(x, w, H, Fh, a=a, scale=2.0)
    y1 = A.broadcast_add(x, None, H, Fh, u=u, rows_per_seg=3, scale=1.0)
    for r in range(7):
        for c in range(C):
            assert abs(y0[r, c] - (x[r, c] + 2.0 * w[r, c // Fh] * a[c // Fh, c % Fh])) < 1e-14
            assert y1[r, c] == x[r, c] + u[r // 3, c]
    rp, val, ep = torch.tensor([0, 2, 2, 3], dtype=torch.int32), A.rnd(6, 3, H).double(), torch.tensor([2, 0, 1], dtype=torch.int32)
    _close("row_sum", A.csr_row_sum(rp, val, ep), torch.stack([val[2] + val[0], 0 * val[0], val[1]]))
    ws, as_ = [A.rnd(10 + k, 5, 6) for k in range(3)], [A.rnd(20 + k, 12) for k in range(3)]
    W, Ak = A.pack_heads(ws, as_)
    assert W.shape == (5, 18) and Ak.shape == (2, 3, 6)
    assert all(torch.equal(W[:, 6 * k:6 * k + 6], ws[k]) and torch.equal(Ak[0, k], as_[k][:6]) and torch.equal(Ak[1, k], as_[k][6:]) for k in range(3))
    gw, ga = A.unpack_heads(W, Ak[0], Ak[1], 3, 5, 6)
    assert all(torch.equal(gw[k], ws[k]) and torch.equal(ga[k], as_[k]) for k in range(3))
    gw, ga = A.unpack_heads(None, None, Ak[1], 3, 5, 6)
    assert not gw.any() and not ga[:, :6].any() and torch.equal(ga[:, 6:], Ak[1])


# ----------------------------------------------------------------------------- the guarantees of the seeded inputs
def test_graphs_have_the_degrees_they_promise():
    for name, degs in (("softmax", A.SM_DEGREES), ("vec", A.VEC_DEGREES), ("scalar", A.SCALAR_DEGREES), ("sddmm", A.SDDMM_DEGREES)):
        rowptr, col, ncols = A.graph(name)
        deg = (rowptr[1:] - rowptr[:-1]).tolist()
        assert deg[:len(degs)] == list(degs) and rowptr[0] == 0 and rowptr[-1] == col.numel()
        assert 0 <= int(col.min()) and int(col.max()) < ncols
        g = A.row_of(rowptr)
        assert torch.unique(g * ncols + col.long()).numel() == col.numel()                    # no entry twice
    rp_t, col_t, n = A.graph("softmax_t")
    assert (rp_t[1:] - rp_t[:-1]).tolist()[10:17] == list(A.SM_DEGREES) and n == A.SM_ROWS
    assert (A.graph("vec")[0].numel() - 1) % 16 == 1 and (A.graph("scalar")[0].numel() - 1) % 4 == 1
    rows = A.graph("sddmm")[0].numel() - 1
    assert rows % 16 == 1 and rows % 8 == 1 and rows % 4 == 1
    for H in (1, 3, 4):
        assert (A.SM_ROWS * H * 8) % 256 and (2 * A.SM_ROWS * H * 8) % 256
    # transpose() is the transpose, and tile() keeps every copy on graph 0's nodes
    rowptr, col, n = A.graph("softmax")
    rp_t, col_t, src_e = A.transpose(rowptr, col, n)
    g, g_t = A.row_of(rowptr), A.row_of(rp_t)
    assert torch.equal(col_t.long(), g[src_e.long()]) and torch.equal(g_t, col.long()[src_e.long()])
    rp2, col2 = A.tile(rowptr, col, n, 2)
    assert rp2.numel() == 2 * n + 1 and torch.equal(col2.long() % n, torch.cat([col, col]).long()) and int(col2.max()) >= n


def test_softmax_inputs_keep_their_margin_from_the_kink():
    assert len(set(A.SOFTMAX_CELLS)) == len(A.SOFTMAX_CELLS)
    assert {c[1] for c in A.SOFTMAX_CELLS} == {1, 3, 4} and {c[3] for c in A.SOFTMAX_CELLS} == {0.2, 1.0}
    for cell in A.SOFTMAX_CELLS:
        rowptr, col, rows, mod, s_grp, s_oth = A.softmax_inputs(cell)
        assert s_grp.dtype == torch.float32 and torch.isfinite(s_grp).all() and torch.isfinite(s_oth).all()
        assert A.score_margin(rowptr, col, mod, s_grp, s_oth) >= G.MARGIN, cell
        assert (mod == 0) != cell[2] and rows == (2 if cell[2] else 1) * A.SM_ROWS
        if cell[4]:
            t = A.edge_scores(rowptr, col, mod, s_grp, s_oth)
            assert t.max().item() > 50 and t.min().item() < -50


def test_elu_inputs_keep_their_margin_from_zero():
    for cell in A.ELU_CELLS:
        rows, H, Fh, mean, elu, _ = cell
        x, special = A.elu_inputs(cell), A.elu_special_mask(cell)
        assert x.shape == (rows, H * Fh) and A.elu_margin(cell) >= G.MARGIN, cell
        got = x[special].reshape(H, len(A.ELU_SPECIALS))
        assert (got == torch.tensor(A.ELU_SPECIALS)).all() and torch.signbit(got[:, 1]).all() and not torch.signbit(got[:, 0]).any()
    assert any((c[0] * c[1] * c[2]) % 2 for c in A.ELU_CELLS) and any(c[3] and c[1] == 3 for c in A.ELU_CELLS)


@pytest.mark.parametrize("name", ["edges", "blocks31"])
@pytest.mark.parametrize("kind", G.KINDS)
def test_layer_inputs_keep_their_margin_from_the_kink(name, kind):
    L = G.layout(name, kind)
    rowptr, col = A.layout_csr(L)
    assert A.layer_margin(*A.layer_inputs(L, 2, 8, 50), rowptr, col, 2, 8) >= G.MARGIN
    rp, c, edge_index, entry_of = A.self_looped(L)
    assert A.layer_margin(*A.layer_inputs(L, 2, 8, 51, rp, c), rp, c, 2, 8) >= G.MARGIN
    assert torch.equal(c.long()[entry_of.long()], edge_index[0]) and torch.equal(A.row_of(rp)[entry_of.long()], edge_index[1])


# ----------------------------------------------------------------------------- argument checks of the 18 entry points
def test_every_entry_point_checks_its_arguments_before_launching():
    """TSGNN_EINVAL for null pointers, non-positive head counts, negative row counts, strides narrower than the row, and the
    epilogue's / broadcast's inconsistent pairs: all decided on the host, nothing is launched (no GPU here)"""
    from two_stage_gnn_amd import _native as nat
    L = nat.lib()
    P = 1 << 20                                                   # (pointers are only tested for NULL)
    N = None
    bad = [
        ("node_scores_f32", (N, 8, 4, 2, 4, P, 4, P)), ("node_scores_f32", (P, 8, 4, 2, 4, N, 4, P)), ("node_scores_f32", (P, 8, 4, 2, 4, P, 4, N)),
        ("node_scores_f32", (P, 8, -1, 2, 4, P, 4, P)), ("node_scores_f32", (P, 8, 4, 0, 4, P, 4, P)), ("node_scores_f32", (P, 8, 4, 2, 0, P, 4, P)),
        ("node_scores_f32", (P, 7, 4, 2, 4, P, 4, P)),
        ("node_scores2_f32", (P, 8, 4, 2, 4, P, 4, P, N, 4, P)), ("node_scores2_f32", (P, 8, 4, 2, 4, P, 4, P, P, 4, N)),
        ("node_scores2_f32", (P, 8, 4, 2, 4, N, 4, P, P, 4, P)), ("node_scores2_f32", (P, 7, 4, 2, 4, P, 4, P, P, 4, P)),
        ("edge_softmax_fwd_f32", (N, P, 4, 2, P, P, 0, 0.2, P)), ("edge_softmax_fwd_f32", (P, P, 4, 2, N, P, 0, 0.2, P)),
        ("edge_softmax_fwd_f32", (P, P, 4, 2, P, N, 0, 0.2, P)), ("edge_softmax_fwd_f32", (P, P, 4, 2, P, P, 0, 0.2, N)),
        ("edge_softmax_fwd_f32", (P, P, -1, 2, P, P, 0, 0.2, P)), ("edge_softmax_fwd_f32", (P, P, 4, 0, P, P, 0, 0.2, P)),
        ("edge_softmax_fwd_f32", (P, P, 4, 2, P, P, -1, 0.2, P)),
        ("edge_softmax_bwd_f32", (P, P, 4, 2, P, P, 0, 0.2, N, P, P, P)), ("edge_softmax_bwd_f32", (P, P, 4, 2, P, P, 0, 0.2, P, N, P, P)),
        ("edge_softmax_bwd_f32", (P, P, 4, 2, P, P, 0, 0.2, P, P, N, P)), ("edge_softmax_bwd_f32", (P, P, 4, 2, P, P, 0, 0.2, P, P, P, N)),
        ("edge_softmax_bwd_f32", (N, P, 4, 2, P, P, 0, 0.2, P, P, P, P)), ("edge_softmax_bwd_f32", (P, P, 4, 2, P, P, -1, 0.2, P, P, P, P)),
        ("edge_permute_f32", (N, P, 4, 2, 0, P)), ("edge_permute_f32", (P, N, 4, 2, 0, P)), ("edge_permute_f32", (P, P, 4, 2, 1, N)),
        ("edge_permute_f32", (P, P, -1, 2, 0, P)), ("edge_permute_f32", (P, P, 4, 0, 0, P)),
        ("csr_row_sum_f32", (N, P, 4, 2, P)), ("csr_row_sum_f32", (P, N, 4, 2, P)), ("csr_row_sum_f32", (P, P, 4, 2, N)),
        ("csr_row_sum_f32", (P, P, -1, 2, P)), ("csr_row_sum_f32", (P, P, 4, 0, P)),
        ("csr_row_sum_perm_f32", (P, P, N, 4, 2, P)), ("csr_row_sum_perm_f32", (N, P, P, 4, 2, P)), ("csr_row_sum_perm_f32", (P, P, P, 4, 2, N)),
        ("csr_spmm_heads_f32", (N, P, P, 2, 4, P, 8, 0, P, 8, 4)), ("csr_spmm_heads_f32", (P, P, N, 2, 4, P, 8, 0, P, 8, 4)),
        ("csr_spmm_heads_f32", (P, P, P, 2, 4, N, 8, 0, P, 8, 4)), ("csr_spmm_heads_f32", (P, P, P, 2, 4, P, 8, 0, N, 8, 4)),
        ("csr_spmm_heads_f32", (P, P, P, 2, 4, P, 7, 0, P, 8, 4)), ("csr_spmm_heads_f32", (P, P, P, 2, 4, P, 8, 0, P, 7, 4)),
        ("csr_spmm_heads_f32", (P, P, P, 2, 4, P, 8, -1, P, 8, 4)), ("csr_spmm_heads_f32", (P, P, P, 0, 4, P, 8, 0, P, 8, 4)),
        ("csr_spmm_heads_f32", (P, P, P, 2, 4, P, 8, 0, P, 8, -1)),
        ("csr_spmm_heads_epi_f32", (P, P, P, 2, 4, P, 8, 0, P, 8, 4, P, N, 4, N, N, 0, N, 0, N, 1, N, 1.0, N)),      # w1 without a1
        ("csr_spmm_heads_epi_f32", (P, P, P, 2, 4, P, 8, 0, P, 8, 4, N, N, 0, P, N, 4, N, 0, N, 1, N, 1.0, N)),      # w2 without a2
        ("csr_spmm_heads_epi_f32", (P, P, P, 2, 4, P, 8, 0, P, 8, 4, N, N, 0, N, N, 0, P, 8, N, 0, N, 1.0, N)),      # u without a segment map
        ("csr_spmm_heads_epi_f32", (N, P, P, 2, 4, P, 8, 0, P, 8, 4, N, N, 0, N, N, 0, N, 0, N, 1, N, 1.0, N)),
        ("csr_sddmm_heads_f32", (N, P, 2, 4, P, 8, P, 8, 0, P, 4)), ("csr_sddmm_heads_f32", (P, P, 2, 4, N, 8, P, 8, 0, P, 4)),
        ("csr_sddmm_heads_f32", (P, P, 2, 4, P, 8, N, 8, 0, P, 4)), ("csr_sddmm_heads_f32", (P, P, 2, 4, P, 8, P, 8, 0, N, 4)),
        ("csr_sddmm_heads_f32", (P, P, 2, 4, P, 8, P, 8, -1, P, 4)), ("csr_sddmm_heads_f32", (P, P, 2, 0, P, 8, P, 8, 0, P, 4)),
        ("segment_wsum_f32", (N, 8, N, 2, 4, P, 2, 10, 10, 1.0, 0, P, P, 8)), ("segment_wsum_f32", (P, 8, N, 2, 4, P, 2, 10, 10, 1.0, 0, N, P, 8)),
        ("segment_wsum_f32", (P, 8, N, 2, 4, P, 2, 10, 10, 1.0, 0, P, N, 8)), ("segment_wsum_f32", (P, 8, N, 2, 4, N, 2, 10, 10, 1.0, 0, P, P, 8)),
        ("segment_wsum_f32", (P, 7, N, 2, 4, P, 2, 10, 10, 1.0, 0, P, P, 8)), ("segment_wsum_f32", (P, 8, N, 2, 4, P, 2, 10, 10, 1.0, 0, P, P, 7)),
        ("segment_wsum_f32", (P, 8, N, 2, 4, P, 0, 10, 10, 1.0, 0, P, P, 8)), ("segment_wsum_f32", (P, 8, N, 2, 4, P, 2, 10, -1, 1.0, 0, P, P, 8)),
        ("segment_wsum2_f32", (P, 8, N, P, 2, 4, P, 2, 10, 10, 1.0, P, P, P, 8)), ("segment_wsum2_f32", (P, 8, P, N, 2, 4, P, 2, 10, 10, 1.0, P, P, P, 8)),
        ("segment_wsum2_f32", (P, 8, P, P, 2, 4, P, 2, 10, 10, 1.0, P, P, N, 8)), ("segment_wsum2_f32", (P, 8, P, P, 2, 4, N, 2, 10, 10, 1.0, P, P, P, 8)),
        ("segment_wsum2_f32", (P, 8, P, P, 2, 4, P, 2, 10, 10, 1.0, N, P, P, 8)),
        ("gather_wsum_f32", (N, 8, P, P, P, 2, 8, 1.0, P, 8)), ("gather_wsum_f32", (P, 8, N, P, P, 2, 8, 1.0, P, 8)),
        ("gather_wsum_f32", (P, 8, P, N, P, 2, 8, 1.0, P, 8)), ("gather_wsum_f32", (P, 8, P, P, N, 2, 8, 1.0, P, 8)),
        ("gather_wsum_f32", (P, 8, P, P, P, 2, 8, 1.0, N, 8)), ("gather_wsum_f32", (P, 8, P, P, P, 0, 8, 1.0, P, 8)),
        ("gather_wsum_f32", (P, 7, P, P, P, 2, 8, 1.0, P, 8)), ("gather_wsum_f32", (P, 8, P, P, P, 2, 8, 1.0, P, 7)),
        ("broadcast_add_f32", (N, 8, 4, 2, 4, P, P, 4, N, 0, 0, 1.0)), ("broadcast_add_f32", (P, 8, 4, 2, 4, P, P, 4, P, 8, 2, 1.0)),      # both modes
        ("broadcast_add_f32", (P, 8, 4, 2, 4, P, N, 0, N, 0, 0, 1.0)), ("broadcast_add_f32", (P, 8, 4, 2, 4, P, N, 0, P, 8, 0, 1.0)),      # neither; u, no segments
        ("elu_heads_fwd_f32", (N, 4, 2, 4, 0, 1, P)), ("elu_heads_fwd_f32", (P, 4, 2, 4, 0, 1, N)), ("elu_heads_fwd_f32", (P, -1, 2, 4, 0, 1, P)),
        ("elu_heads_fwd_f32", (P, 4, 0, 4, 0, 1, P)),
        ("elu_heads_bwd_f32", (N, P, 4, 2, 4, 0, 1, P)), ("elu_heads_bwd_f32", (P, N, 4, 2, 4, 0, 1, P)), ("elu_heads_bwd_f32", (P, P, 4, 2, 4, 0, 1, N)),
        ("elu_heads_bwd_f32", (P, P, 4, 2, 0, 0, 1, P)),
        ("pack_heads_f32", (P,) * 16 + (9, 5, 6, P, P)), ("pack_heads_f32", (P,) * 16 + (0, 5, 6, P, P)), ("pack_heads_f32", (P,) * 16 + (2, 5, 6, N, P)),
        ("pack_heads_f32", (P, N) + (P,) * 14 + (2, 5, 6, P, P)), ("pack_heads_f32", (P,) * 9 + (N,) + (P,) * 6 + (2, 5, 6, P, P)),
        ("unpack_heads_f32", (P, P, P, 0, 5, 6, P, P)), ("unpack_heads_f32", (P, P, P, 2, 5, 6, N, P)), ("unpack_heads_f32", (P, P, P, 2, 5, 6, P, N)),
        ("unpack_heads_f32", (P, P, P, 2, 0, 6, P, P)),
    ]
    assert len({n for n, _ in bad}) == 18
    for name, args in bad:
        assert getattr(L, "tsgnn_" + name)(*args, None) == EINVAL, (name, args)
    assert L.tsgnn_pack_heads_max() == 8
    # calls that return before any launch: no rows, no entries
    assert L.tsgnn_node_scores_f32(P, 8, 0, 2, 4, P, 4, P, None) == 0 and L.tsgnn_edge_permute_f32(P, P, 0, 2, 0, P, None) == 0
    assert L.tsgnn_csr_spmm_heads_f32(P, P, P, 2, 4, P, 8, 0, P, 8, 0, None) == 0 and L.tsgnn_elu_heads_fwd_f32(P, 0, 2, 4, 0, 1, P, None) == 0
