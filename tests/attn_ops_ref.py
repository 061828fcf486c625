"""Reference of the composed (per-op) GAT attention kernels (csrc/attention.hip), one function per entry point, on CSR arrays.
TEST INFRASTRUCTURE: plain torch on the CPU, no project kernel.  Every function computes in the dtype of its float input: float64
is the reference, float32 runs the SAME code in single precision (the yardstick of the kernels' rounding, tests/fp32_yardstick.py).

    t[e, h]     = s_grp[g(e) % mod, h] + s_oth[col[e] % mod, h]            g(e): the CSR row (softmax group) of entry e; mod = 0: no %
    alpha[e, h] = softmax over the entries of g(e) of LeakyReLU(t[e, h])

There is no hand-written backward: ``edge_softmax_bwd`` and ``elu_heads_bwd`` are ``torch.autograd.grad`` of the forward functions.

This module also holds the seeded graphs and inputs of tests/test_gpu_attn_ops.py, so that tests/test_attn_ops_ref_host.py can check
their guarantees without a GPU: every score sum t is at least MARGIN away from 0 (fp32 cannot flip LeakyReLU's branch), and no ELU
input lies within MARGIN of 0 except the exact zeros put there on purpose.
"""
import torch
import torch.nn.functional as F

from gat_attn_ref import MARGIN


# ----------------------------------------------------------------------------- CSR helpers
def row_of(rowptr):
    """row (group) of every entry"""
    rp = rowptr.long()
    return torch.repeat_interleave(torch.arange(rp.numel() - 1), rp[1:] - rp[:-1])


def _node(col, mod):
    c = col.long()
    return c % mod if mod else c


def transpose(rowptr, col, ncols):
    """(rowptr_t, col_t, src_e): CSR of A^T, the entries of a transposed row ascending by source row; src_e[p] = the entry of A"""
    r, c = row_of(rowptr), col.long()
    order = torch.argsort(c * (rowptr.numel() - 1) + r)
    rp_t = torch.zeros(ncols + 1, dtype=torch.int64)
    rp_t[1:] = torch.cumsum(torch.bincount(c, minlength=ncols), 0)
    return rp_t.to(torch.int32), r[order].to(torch.int32), order.to(torch.int32)


def inverse(perm):
    inv = torch.empty_like(perm)
    inv[perm.long()] = torch.arange(perm.numel(), dtype=perm.dtype)
    return inv


def tile(rowptr, col, ncols, k):
    """k copies of the graph below each other, copy c's columns shifted by c * ncols: with mod = ncols every copy reads graph 0's nodes"""
    rp, nnz = rowptr.long(), int(rowptr[-1])
    rps = [rp[:-1] + c * nnz for c in range(k)] + [torch.tensor([k * nnz])]
    return torch.cat(rps).to(torch.int32), torch.cat([col.long() + c * ncols for c in range(k)]).to(torch.int32)


# ----------------------------------------------------------------------------- the entry points
def _heads(x, H, Fh):
    return x[:, :H * Fh].reshape(x.size(0), H, Fh)


def node_scores(x, a, H, Fh):
    """s[r, h] = sum_f x[r, h Fh + f] a[h, f];  x [rows, >= H Fh], a [H, >= Fh]"""
    return (_heads(x, H, Fh) * a[:, :Fh].unsqueeze(0)).sum(dim=2)


def node_scores2(x, a1, a2, H, Fh):
    return node_scores(x, a1, H, Fh), node_scores(x, a2, H, Fh)


def edge_scores(rowptr, col, mod, s_grp, s_oth):
    g = row_of(rowptr)
    return s_grp[g % mod if mod else g] + s_oth[_node(col, mod)]


def _group_softmax(rowptr, e):
    g = row_of(rowptr)
    rows, H = rowptr.numel() - 1, e.size(1)
    idx = g.unsqueeze(1).expand(-1, H)
    m = torch.full((rows, H), -float("inf"), dtype=e.dtype).scatter_reduce(0, idx, e.detach(), "amax")
    p = torch.exp(e - m[g])
    den = torch.zeros(rows, H, dtype=e.dtype).index_add(0, g, p)
    return p / den[g]


def edge_softmax_fwd(rowptr, col, mod, s_grp, s_oth, slope):
    """alpha [nnz, H]"""
    return _group_softmax(rowptr, F.leaky_relu(edge_scores(rowptr, col, mod, s_grp, s_oth), slope))


def edge_softmax_bwd(rowptr, col, mod, s_grp, s_oth, slope, dalpha):
    """(dt [nnz, H], ds_grp [rows, H]) by autograd of edge_softmax_fwd: dt = d/dt[e, h], ds_grp = d/d(the group's own score), which
    is the sum of dt over the group's entries (0 for an empty group)"""
    g = row_of(rowptr)
    rows = rowptr.numel() - 1
    sg = s_grp[torch.arange(rows) % mod if mod else torch.arange(rows)].detach().clone().requires_grad_(True)
    tz = torch.zeros(g.numel(), s_grp.size(1), dtype=s_grp.dtype, requires_grad=True)
    t = sg[g] + s_oth.detach()[_node(col, mod)] + tz
    alpha = _group_softmax(rowptr, F.leaky_relu(t, slope))
    dt, dsg = torch.autograd.grad((alpha * dalpha.to(alpha.dtype)).sum(), [tz, sg], allow_unused=True)
    return dt, (dsg if dsg is not None else torch.zeros_like(sg))


def edge_permute(src, perm, scatter):
    """gather: dst[p] = src[perm[p]];  scatter: dst[perm[p]] = src[p]"""
    if not scatter:
        return src[perm.long()]
    dst = torch.empty_like(src)
    dst[perm.long()] = src
    return dst


def csr_row_sum(rowptr, val, eperm=None):
    """out[r, h] = sum over the row's entries of val[eperm[e], h]"""
    v = val[eperm.long()] if eperm is not None else val[:int(rowptr[-1])]
    return torch.zeros(rowptr.numel() - 1, val.size(1), dtype=val.dtype).index_add(0, row_of(rowptr), v)


def csr_spmm_heads(rowptr, col, mod, alpha, x, H, Fh, w1=None, a1=None, w2=None, a2=None, u=None, uw=None, rows_per_seg=0, row_seg=None,
                   uscale=1.0, eperm=None):
    """y[r, h Fh + f] = sum_e alpha[eperm[e], h] x[col[e] % mod, h Fh + f] + w1[r, h] a1[h, f] + w2[r, h] a2[h, f]
                        + uscale (uw ? uw[r, h] : 1) u[seg(r), h Fh + f],    seg(r) = row_seg[r] or r // rows_per_seg"""
    rows = rowptr.numel() - 1
    g = row_of(rowptr)
    al = alpha[eperm.long()] if eperm is not None else alpha[:g.numel()]
    y = torch.zeros(rows, H, Fh, dtype=x.dtype).index_add(0, g, al.unsqueeze(2) * _heads(x, H, Fh)[_node(col, mod)])
    if w1 is not None:
        y = y + w1.unsqueeze(2) * a1[:, :Fh].unsqueeze(0)
    if w2 is not None:
        y = y + w2.unsqueeze(2) * a2[:, :Fh].unsqueeze(0)
    if u is not None:
        seg = row_seg.long() if row_seg is not None else torch.arange(rows) // rows_per_seg
        wv = uw.unsqueeze(2) if uw is not None else 1.0
        y = y + uscale * wv * _heads(u, H, Fh)[seg]
    return y.reshape(rows, H * Fh)


def csr_sddmm_heads(rowptr, col, mod, dy, x, H, Fh):
    """dalpha[e, h] = <dy[g(e), head h], x[col[e] % mod, head h]>"""
    return (_heads(dy, H, Fh)[row_of(rowptr)] * _heads(x, H, Fh)[_node(col, mod)]).sum(dim=2)


def segment_wsum(x, w, H, Fh, seg_ptr, scale=1.0, mean=False):
    """out[s, c] = scale * sum_{r in segment s} w[r, c // Fh] x[r, c]  (w None: 1; mean: / the segment's length, 0 if empty);
    seg_ptr None: one segment of all rows"""
    rows = x.size(0)
    sp = torch.tensor([0, rows]) if seg_ptr is None else seg_ptr.long()
    nseg = sp.numel() - 1
    seg = torch.repeat_interleave(torch.arange(nseg), sp[1:] - sp[:-1])
    xs = _heads(x, H, Fh)[int(sp[0]):int(sp[-1])]
    if w is not None:
        xs = xs * w[int(sp[0]):int(sp[-1])].unsqueeze(2)
    out = torch.zeros(nseg, H, Fh, dtype=x.dtype).index_add(0, seg, xs).reshape(nseg, H * Fh)
    if mean:
        ln = (sp[1:] - sp[:-1]).to(x.dtype)
        sc = torch.where(ln > 0, scale / torch.clamp(ln, min=1), torch.zeros_like(ln))
        return out * sc.unsqueeze(1)
    return out * scale


def segment_wsum2(x, w1, w2, H, Fh, seg_ptr, scale=1.0):
    return segment_wsum(x, w1, H, Fh, seg_ptr, scale), segment_wsum(x, w2, H, Fh, seg_ptr, scale)


def gather_wsum(x, idx, w, seg_ptr, C, scale=1.0):
    """out[s, c] = scale * sum_{e in [seg_ptr[s], seg_ptr[s+1])} w[e] x[idx[e], c]"""
    sp = seg_ptr.long()
    nseg = sp.numel() - 1
    seg = torch.repeat_interleave(torch.arange(nseg), sp[1:] - sp[:-1])
    return scale * torch.zeros(nseg, C, dtype=x.dtype).index_add(0, seg, w.unsqueeze(1) * x[idx.long(), :C])


def broadcast_add(y, w, H, Fh, a=None, u=None, rows_per_seg=0, scale=1.0):
    """mode 0 (a): y[r, c] += scale w[r, c // Fh] a[c // Fh, c % Fh];  mode 1 (u): y[r, c] += scale (w ? w[r, c // Fh] : 1) u[r // rows_per_seg, c]"""
    rows = y.size(0)
    wv = w.unsqueeze(2) if w is not None else torch.ones(rows, H, 1, dtype=y.dtype)
    if a is not None:
        add = wv * a[:, :Fh].unsqueeze(0)
    else:
        add = wv * _heads(u, H, Fh)[torch.arange(rows) // rows_per_seg]
    return y[:, :H * Fh] + scale * add.reshape(rows, H * Fh)


def elu_heads_fwd(x, H, Fh, mean_heads, apply_elu):
    v = _heads(x, H, Fh).sum(dim=1) / H if mean_heads else x[:, :H * Fh]
    return F.elu(v) if apply_elu else v


def elu_heads_bwd(x, dy, H, Fh, mean_heads, apply_elu):
    x = x.detach().clone().requires_grad_(True)
    return torch.autograd.grad((elu_heads_fwd(x, H, Fh, mean_heads, apply_elu) * dy.to(x.dtype)).sum(), x)[0]


def pack_heads(ws, as_):
    """(W [Fin, H Fo], A [2, H, Fo]): W[i, h Fo + f] = w_h[i, f], A[s, h, f] = a_h[s Fo + f]"""
    Fo = ws[0].size(1)
    return torch.cat(list(ws), dim=1), torch.stack([a.reshape(2, Fo) for a in as_], dim=1)


def unpack_heads(dW, dA0, dA1, H, Fin, Fo):
    """(gw [H, Fin, Fo], ga [H, 2 Fo]): gw[h, i, f] = dW[i, h Fo + f], ga[h, s Fo + f] = dA_s[h, f]; a None source gives zeros"""
    z = torch.zeros
    gw = dW.reshape(Fin, H, Fo).permute(1, 0, 2).contiguous() if dW is not None else z(H, Fin, Fo)
    ga = torch.cat([dA0 if dA0 is not None else z(H, Fo), dA1 if dA1 is not None else z(H, Fo)], dim=1)
    return gw, ga


# ----------------------------------------------------------------------------- the composed layer (what attention.py issues)
def layout_csr(L):
    """(rowptr, col) of a gat_attn_ref.Layout's entries, rows ascending, columns ascending inside a row"""
    i, j = L.entries()
    order = torch.argsort(i * L.R + j)
    rp = torch.zeros(L.R + 1, dtype=torch.int64)
    rp[1:] = torch.cumsum(torch.bincount(i, minlength=L.R), 0)
    return rp.to(torch.int32), j[order].to(torch.int32)


def compose(h, a_row, a_col, rowptr, col, H, Fh, slope, by_column, uniform=None, drop_mult=None, mean_heads=False, apply_elu=True):
    """the per-op layer on CSR arrays: node_scores2 -> edge_softmax (over A^T's rows with the operands swapped when by_column, else
    over A's rows) -> the head-weighted aggregation over A (alpha read through the entry map when by_column; the uniform term of
    the edge-less columns in its epilogue) -> elu_heads.  uniform: None or (row_mult [R], row_graph [R], graph_ptr [B + 1], N);
    drop_mult [nnz, H]: per-target mode only"""
    R = rowptr.numel() - 1
    s_row, s_col = node_scores2(h, a_row, a_col, H, Fh)
    if by_column:
        rp_t, col_t, src_e = transpose(rowptr, col, R)
        alpha = edge_softmax_fwd(rp_t, col_t, 0, s_col, s_row, slope)
        epi = {"eperm": inverse(src_e)}
        if uniform is not None:
            mult, row_graph, graph_ptr, N = uniform
            iso = ((rp_t[1:] - rp_t[:-1]) == 0).to(h.dtype) * mult.to(h.dtype)
            u = segment_wsum(h, iso.unsqueeze(1).expand(R, H), H, Fh, graph_ptr, scale=1.0 / N)
            epi.update(u=u, row_seg=row_graph)
    else:
        alpha = edge_softmax_fwd(rowptr, col, 0, s_row, s_col, slope)
        if drop_mult is not None:
            alpha = alpha * drop_mult.to(alpha.dtype)
        epi = {}
    out = csr_spmm_heads(rowptr, col, 0, alpha, h, H, Fh, **epi)
    return elu_heads_fwd(out, H, Fh, mean_heads, apply_elu)


# ----------------------------------------------------------------------------- seeded graphs
SM_DEGREES = (0, 70, 1, 7, 8, 9, 17)          # a row without entries next to the longest; the 8-lane group and its strided tail
SM_ROWS = 110


def softmax_graph():
    """(rowptr, col), 110 x 110: rows 0..6 have SM_DEGREES entries (columns 40..), columns 10..16 have SM_DEGREES entries (rows 40..);
    every other row among 0..39 is empty: A and A^T both hold the degree set"""
    adj = torch.zeros(SM_ROWS, SM_ROWS, dtype=torch.bool)
    for k, d in enumerate(SM_DEGREES):
        adj[k, 40:40 + d] = True
        adj[40:40 + d, 10 + k] = True
    r, c = torch.nonzero(adj, as_tuple=True)
    rp = torch.zeros(SM_ROWS + 1, dtype=torch.int64)
    rp[1:] = torch.cumsum(torch.bincount(r, minlength=SM_ROWS), 0)
    return rp.to(torch.int32), c.to(torch.int32)


def degree_graph(degrees, rows, ncols, seed):
    """(rowptr, col): row k has degrees[k] distinct random columns (unsorted), the rows behind the list 0..5 of them"""
    gen = torch.Generator().manual_seed(seed)
    deg = list(degrees) + [int(d) for d in torch.randint(0, 6, (rows - len(degrees),), generator=gen)]
    assert len(deg) == rows and max(deg) <= ncols
    cols = [torch.randperm(ncols, generator=gen)[:d] for d in deg]
    rp = torch.zeros(rows + 1, dtype=torch.int64)
    rp[1:] = torch.cumsum(torch.tensor(deg), 0)
    return rp.to(torch.int32), torch.cat(cols).to(torch.int32)


VEC_DEGREES = (0, 1, 7, 8, 9, 17)
SCALAR_DEGREES = (63, 64, 65, 130)
SDDMM_DEGREES = (0, 70, 1, 7, 8, 9, 17)
_graphs = {}


def graph(name):
    """'softmax' | 'softmax_t' (its transpose) | 'vec' (33 rows = one more than a multiple of 16, 8 and 4; 33 columns) | 'scalar' (133
    x 133, the 64-entry batches) | 'sddmm' (81 x 81, rows of 0 and 70 entries side by side) -> (rowptr, col, ncols)"""
    if name not in _graphs:
        if name == "softmax":
            _graphs[name] = softmax_graph() + (SM_ROWS,)
        elif name == "softmax_t":
            _graphs[name] = transpose(*softmax_graph(), SM_ROWS)[:2] + (SM_ROWS,)
        elif name == "vec":
            _graphs[name] = degree_graph(VEC_DEGREES, 33, 33, 1) + (33,)
        elif name == "scalar":
            _graphs[name] = degree_graph(SCALAR_DEGREES, 133, 133, 2) + (133,)
        else:
            assert name == "sddmm"
            _graphs[name] = degree_graph(SDDMM_DEGREES, 81, 81, 3) + (81,)
    return _graphs[name]


# ----------------------------------------------------------------------------- seeded inputs
def rnd(seed, *shape, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


def score_margin(rowptr, col, mod, s_grp, s_oth):
    """min |t| over all entries and heads, of the float32 sum and of the exact one"""
    if int(rowptr[-1]) == 0:
        return float("inf")
    t32 = edge_scores(rowptr, col, mod, s_grp, s_oth).abs().min().item()
    t64 = edge_scores(rowptr, col, mod, s_grp.double(), s_oth.double()).abs().min().item()
    return min(t32, t64)


# (graph, H, tiled with mod = n, slope, scores of magnitude 60)
SOFTMAX_CELLS = [(g, H, False, 0.2, False) for g in ("softmax", "softmax_t") for H in (1, 3, 4)]
SOFTMAX_CELLS += [("softmax", 3, True, 0.2, False), ("softmax_t", 4, True, 0.2, False), ("softmax", 3, False, 1.0, False),
                  ("softmax_t", 1, False, 1.0, False), ("softmax", 4, False, 0.2, True), ("softmax_t", 3, False, 0.2, True)]
_sm = {}


def softmax_inputs(cell):
    """(rowptr, col, rows, mod, s_grp [n, H], s_oth [n, H]) float32.  Group scores whose sum with an entry's other score comes within
    MARGIN of the kink of LeakyReLU are redrawn until none does"""
    if cell not in _sm:
        name, H, tiled, slope, extreme = cell
        rowptr, col, n = graph(name)
        mod = 0
        if tiled:
            rowptr, col = tile(rowptr, col, n, 2)
            mod = n
        gen = torch.Generator().manual_seed(7000 + SOFTMAX_CELLS.index(cell))

        def scores(k):
            return (torch.rand(k, H, generator=gen) * 60 - 30) if extreme else torch.randn(k, H, generator=gen)
        s_grp, s_oth = scores(n), scores(n)
        g = row_of(rowptr)
        gi = g % mod if mod else g
        for _ in range(100):
            t32 = edge_scores(rowptr, col, mod, s_grp, s_oth)
            t64 = edge_scores(rowptr, col, mod, s_grp.double(), s_oth.double())
            bad = ((t32.abs() < 2 * MARGIN) | (t64.abs() < 2 * MARGIN)).any(dim=1)
            if not bad.any():
                break
            rows = torch.unique(gi[bad])
            s_grp[rows] = scores(rows.numel())
        assert score_margin(rowptr, col, mod, s_grp, s_oth) >= MARGIN
        _sm[cell] = (rowptr, col, rowptr.numel() - 1, mod, s_grp, s_oth)
    return _sm[cell]


# (rows, H, Fh, mean over heads, apply_elu, misaligned base)
ELU_CELLS = [(9, 4, 8, False, True, False), (9, 4, 8, False, False, False),          # vec4: n % 4 == 0, no mean
             (5, 3, 5, False, True, False),                                          # scalar: rows H Fh odd
             (9, 3, 8, True, True, False), (9, 3, 8, True, False, False),            # scalar: mean over H = 3 heads
             (9, 4, 8, False, True, True)]                                           # scalar: base off 16 bytes by one float
ELU_SPECIALS = (0.0, -0.0, -30.0)
_elu = {}


def elu_inputs(cell):
    """x [rows, H Fh] float32 ~ N(0, 1.5), pushed out of (-2 MARGIN, 2 MARGIN) — the head mean too; row 1 holds the exact values
    ELU_SPECIALS in columns 0..2 of every head (so the head mean there is special as well)"""
    if cell not in _elu:
        rows, H, Fh, mean, elu, _ = cell
        x = rnd(8000 + ELU_CELLS.index(cell), rows, H, Fh, scale=1.5)
        for _ in range(100):
            v = x.sum(dim=1, keepdim=True) / H
            v64 = x.double().sum(dim=1, keepdim=True) / H
            bad = (x.abs() < 2 * MARGIN) | ((v.abs() < 2 * MARGIN) | (v64.abs() < 2 * MARGIN)).expand_as(x)
            if not bad.any():
                break
            x = torch.where(bad, x + 0.37, x)
        for k, v in enumerate(ELU_SPECIALS):
            x[1, :, k] = v
        _elu[cell] = x.reshape(rows, H * Fh).contiguous()
    return _elu[cell]


def elu_special_mask(cell):
    rows, H, Fh, mean, _, _ = cell
    m = torch.zeros(rows, H, Fh, dtype=torch.bool)
    m[1, :, :len(ELU_SPECIALS)] = True
    return m.reshape(rows, H * Fh)


def elu_margin(cell):
    """min |ELU input| outside the special cells (the head mean in mean mode), float32 and exact"""
    rows, H, Fh, mean, _, _ = cell
    x, keep = elu_inputs(cell), ~elu_special_mask(cell)
    if mean:
        keep = keep.reshape(rows, H, Fh)[:, 0, :]
        return min((_heads(t, H, Fh).sum(dim=1) / H)[keep].abs().min().item() for t in (x, x.double()))
    return x[keep].abs().min().item()


def layer_inputs(L, H, Fh, seed, rowptr=None, col=None):
    """(h [R, H Fh], a_row [H, Fh], a_col [H, Fh]) float32 for the composed layer on a Layout; h rows are redrawn until every entry's
    score sum s_row[i] + s_col[j] keeps MARGIN from 0 in float32 and exactly"""
    if rowptr is None:
        rowptr, col = layout_csr(L)
    gen = torch.Generator().manual_seed(seed)
    a_row, a_col = torch.randn(H, Fh, generator=gen) * 0.5, torch.randn(H, Fh, generator=gen) * 0.5
    h = torch.randn(L.R, H * Fh, generator=gen)
    g = row_of(rowptr)
    for _ in range(100):
        m = []
        for dt in (torch.float32, torch.float64):
            s_row, s_col = node_scores2(h.to(dt), a_row.to(dt), a_col.to(dt), H, Fh)
            m.append((s_row[g] + s_col[col.long()]).abs() < 2 * MARGIN)
        bad = (m[0] | m[1]).any(dim=1)
        if not bad.any():
            break
        rows = torch.unique(g[bad])
        h[rows] = torch.randn(rows.numel(), H * Fh, generator=gen)
    return h, a_row, a_col


def layer_margin(h, a_row, a_col, rowptr, col, H, Fh):
    g = row_of(rowptr)
    out = float("inf")
    for dt in (torch.float32, torch.float64):
        s_row, s_col = node_scores2(h.to(dt), a_row.to(dt), a_col.to(dt), H, Fh)
        if g.numel():
            out = min(out, (s_row[g] + s_col[col.long()]).abs().min().item())
    return out


def self_looped(L):
    """(rowptr, col, edge_index [2, E'], entry_of [E']) for the per-target anchor: the Layout's entries without its loops plus one loop
    per row, as CSR (row = target) and as oracle/pyg_ref.gat_conv's edge list (source, target: kept edges, then the loops);
    entry_of[k] = the CSR entry of edge k"""
    i, j = L.entries()
    keep = i != j
    loop = torch.arange(L.R)
    tgt, src = torch.cat([i[keep], loop]), torch.cat([j[keep], loop])
    order = torch.argsort(tgt * L.R + src)
    rp = torch.zeros(L.R + 1, dtype=torch.int64)
    rp[1:] = torch.cumsum(torch.bincount(tgt, minlength=L.R), 0)
    return rp.to(torch.int32), src[order].to(torch.int32), torch.stack([src, tgt]), inverse(order)
