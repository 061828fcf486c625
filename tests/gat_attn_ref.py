"""Reference of the fused GAT attention kernels (csrc/gat_fused.hip) at the kernels' own boundary: the input is the packed
projection ``hp [R, Ns] = [ h_0 | .. | h_{H-1} | s_row_0 .. s_row_{H-1} | s_col_0 .. s_col_{H-1} | pad ]``, not ``(x, w, a)``.
TEST INFRASTRUCTURE: plain torch on the CPU, no project kernel.  Every function computes in the dtype of ``hp``: float64 is the
reference, float32 runs the SAME code in single precision (the yardstick of the kernels' rounding).

The arithmetic is the dense formulation of oracle/dense_ref.gat_head (encoders_GAT.py:29-49) per graph over the padded
``[N, N]`` block: ``e_ij = LeakyReLU(s_row[i] + s_col[j])`` where ``adj[i, j] != 0`` else ``-9e15``, softmax over i per column j (an
all-masked column becomes 1/N), times the dropout multipliers, ``out_i = sum_j att_ij h_j``, concat or mean over heads, ELU.
There is no hand-written backward: gradients are ``torch.autograd.grad`` of ``sum(dy * y)``.

A ``Layout`` maps the kernels' rows to padded slots.  ``padded``: identity.  ``ghost1`` (GraphBatch.from_dense_ghost1): the
``Nmax - n_b`` padded slots of graph b are index_select copies of its ONE representative row, so autograd sums their gradients —
exactly what ``row_mult`` stands for in the kernels.

This module also holds the seeded graphs and inputs of tests/test_gpu_gat_attn_kernels.py, so that
tests/test_gat_attn_ref_host.py can check their guarantees without a GPU.
"""
import numpy as np
import torch
import torch.nn.functional as F

MASK_NEG = -9e15            # encoders_GAT.py:38
MARGIN = 1e-3               # min |s_row[i] + s_col[j]| over all entries: the fp32 sum cannot flip LeakyReLU's branch


def packed_width(H, Fh):
    return (H * Fh + 2 * H + 3) // 4 * 4


# ----------------------------------------------------------------------------- layouts
class Layout:
    """adj [B, N, N] (CPU), real sizes n_b; kind 'padded' (all B * N rows) or 'ghost1' (n_b real rows + one representative of the
    padded slots per graph with n_b < N).  slot_row [B, N]: the row that padded slot (b, n) copies; rep_slot [R]: the flat padded
    slot b * N + n whose output IS row r's output."""

    def __init__(self, adj, sizes, kind):
        assert kind in ("padded", "ghost1") and adj.dim() == 3 and adj.size(1) == adj.size(2)
        sizes = np.asarray(sizes, dtype=np.int64).reshape(-1)
        self.adj, self.kind, self.real_sizes = adj, kind, sizes
        self.B, self.N = B, N = int(adj.size(0)), int(adj.size(1))
        assert sizes.size == B and (sizes >= 0).all() and (sizes <= N).all()
        for b, n in enumerate(sizes):                             # zero padding outside [:n_b, :n_b] (what GraphSampler produces)
            assert not adj[b, n:, :].any() and not adj[b, :, n:].any()
        self.mask = adj != 0
        n = np.arange(N)[None, :]
        if kind == "padded":
            rows = np.full(B, N, dtype=np.int64)
        else:
            rows = sizes + (sizes < N)
        gp = np.zeros(B + 1, dtype=np.int64)
        np.cumsum(rows, out=gp[1:])
        self.rows_per_graph, self.graph_ptr, self.R = rows, gp, int(gp[-1])
        slot_row = gp[:-1, None] + np.minimum(n, rows[:, None] - 1)
        self.slot_row = torch.from_numpy(slot_row)
        self.row_graph = np.repeat(np.arange(B), rows)
        self.rep_slot = torch.from_numpy(self.row_graph * N + (np.arange(self.R) - gp[self.row_graph]))
        mult = np.ones(self.R, dtype=np.float32)
        if kind == "ghost1":
            has = sizes < N
            mult[gp[1:][has] - 1] = (N - sizes[has]).astype(np.float32)
        self.row_mult = mult

    def expand(self, t):
        """[R, W] -> [B, N, W]"""
        return t.index_select(0, self.slot_row.reshape(-1)).reshape(self.B, self.N, t.size(1))

    def rows_of(self, t):
        """[B, N, W] -> [R, W]: every row from the padded slot it stands for"""
        return t.reshape(self.B * self.N, -1).index_select(0, self.rep_slot)

    def entries(self):
        """(row, column) of every adjacency entry, as row ids of this layout"""
        b, i, j = torch.nonzero(self.mask, as_tuple=True)
        return self.slot_row[b, i], self.slot_row[b, j]


# ----------------------------------------------------------------------------- forward / backward
class _EluGradFromY(torch.autograd.Function):
    """ELU whose derivative is taken from a GIVEN output y (y > 0 ? 1 : y + 1), as the kernel takes it from the y handed to it:
    kernel and reference branch on the same input bits"""

    @staticmethod
    def forward(ctx, pre, y):
        ctx.save_for_backward(y)
        return F.elu(pre)

    @staticmethod
    def backward(ctx, g):
        (y,) = ctx.saved_tensors
        return g * torch.where(y > 0, torch.ones_like(y), y + 1), None


def attn_dense(hp, L, H, Fh, slope, mean_heads, apply_elu, mult=None, y_given=None):
    """(y [R, Co], [att_h [B, N, N]]) — att_h: the softmax output of head h before the dropout multipliers.  mult: per head [B, N, N]
    multipliers (tsgnn_gat_dropout_mult_f32; exact, not re-derived).  y_given [R, Co]: ELU' comes from it instead of from y."""
    C = H * Fh
    d = L.expand(hp)
    mask = L.mask
    neg = torch.full((), MASK_NEG, dtype=hp.dtype)
    outs, atts = [], []
    for h in range(H):
        e = F.leaky_relu(d[:, :, C + h].unsqueeze(2) + d[:, :, C + H + h].unsqueeze(1), slope)
        att = torch.softmax(torch.where(mask, e, neg), dim=1)
        atts.append(att)
        if mult is not None:
            att = att * mult[h].to(hp.dtype)
        outs.append(torch.matmul(att, d[:, :, h * Fh:(h + 1) * Fh]))
    if mean_heads:
        s = outs[0]
        for o in outs[1:]:
            s = s + o
        pre = s / H
    else:
        pre = torch.cat(outs, dim=2)
    if apply_elu:
        pre = F.elu(pre) if y_given is None else _EluGradFromY.apply(pre, L.expand(y_given.to(hp.dtype)))
    return L.rows_of(pre), atts


def attn_fwd(hp, layout, H, Fh, slope, mean_heads, apply_elu, mult=None):
    return attn_dense(hp, layout, H, Fh, slope, mean_heads, apply_elu, mult)[0]


def readout_dy(L, ro_arg, ro_dout):
    """dy[i, c] = (ro_arg[b, c] == i) ? ro_dout[b, c] : 0 with b = the graph of row i"""
    rg = torch.from_numpy(L.row_graph)
    i = torch.arange(L.R).unsqueeze(1)
    return torch.where(ro_arg.long()[rg] == i, ro_dout[rg], torch.zeros((), dtype=ro_dout.dtype))


def attn_bwd(hp, layout, H, Fh, slope, mean_heads, apply_elu, y_given, dy=None, ro_arg=None, ro_dout=None, mult=None):
    """(dhp [R, Ns], S [R, H]) by autograd in hp's dtype.  dhp = dh | d s_row | d s_col | 0; S[j, h] = sum over column j's
    ENTRIES i of att_ij * dL/datt_ij (0 for an edge-less column).  Exactly one of dy [R, Co] and (ro_arg, ro_dout) [B, Co]."""
    assert (dy is None) != (ro_arg is None)
    L = layout
    if dy is None:
        dy = readout_dy(L, ro_arg, ro_dout)
    hp = hp.detach().clone().requires_grad_(True)
    y, atts = attn_dense(hp, L, H, Fh, slope, mean_heads, apply_elu, mult, y_given if apply_elu else None)
    grads = torch.autograd.grad((dy.to(hp.dtype) * y).sum(), [hp] + atts)
    S = torch.stack([(a.detach() * g * L.mask).sum(dim=1) for a, g in zip(atts, grads[1:])], dim=2)     # [B, N, H]
    return grads[0], L.rows_of(S)


def col_stats(hp, layout, H, Fh, slope):
    """(m [R, H], 1 / Z [R, H]) of every column over its entries; edge-less columns give (0, 0)"""
    L, C = layout, H * Fh
    d = L.expand(hp)
    e = F.leaky_relu(d[:, :, C:C + H].unsqueeze(2) + d[:, :, C + H:C + 2 * H].unsqueeze(1), slope)      # [B, i, j, H]
    mk = L.mask.unsqueeze(3)
    has = mk.any(dim=1)                                                                                  # [B, j, 1]
    m = torch.where(mk, e, torch.full((), -float("inf"), dtype=hp.dtype)).max(dim=1)[0]
    m = torch.where(has, m, torch.zeros((), dtype=hp.dtype))
    z = torch.where(mk, torch.exp(e - m.unsqueeze(1)), torch.zeros((), dtype=hp.dtype)).sum(dim=1)
    rz = torch.where(has, 1.0 / torch.where(has, z, torch.ones((), dtype=hp.dtype)), torch.zeros((), dtype=hp.dtype))
    return L.rows_of(m), L.rows_of(rz)


# ----------------------------------------------------------------------------- parameters of the heads <-> W'
def pack(ws, as_, Ns=None):
    """W' [Fin, Ns] = [ W_0 | .. | W_{H-1} | W_h a1_h .. | W_h a2_h .. | 0 ]; ws: H x [Fin, Fo], as_: H x [2 Fo] (or [2 Fo, 1])"""
    H, Fo = len(ws), int(ws[0].size(1))
    Ns = packed_width(H, Fo) if Ns is None else Ns
    a = [v.reshape(-1) for v in as_]
    cols = list(ws) + [(w @ v[:Fo]).unsqueeze(1) for w, v in zip(ws, a)] + [(w @ v[Fo:]).unsqueeze(1) for w, v in zip(ws, a)]
    out = torch.cat(cols, dim=1)
    return torch.cat([out, out.new_zeros(out.size(0), Ns - out.size(1))], dim=1)


def unpack(dwp, ws, as_):
    """(gw [H, Fin, Fo], ga [H, 2 Fo]) from dW' by the formulas of gat_unpack_kernel:
    gw[h][k, f] = dW'[k, hFo+f] + dW'[k, C+h] a1_h[f] + dW'[k, C+H+h] a2_h[f];
    ga[h][f] = sum_k W_h[k, f] dW'[k, C+h],  ga[h][Fo+f] = sum_k W_h[k, f] dW'[k, C+H+h]"""
    H, Fo = len(ws), int(ws[0].size(1))
    C = H * Fo
    gw, ga = [], []
    for h in range(H):
        a = as_[h].reshape(-1)
        d1, d2 = dwp[:, C + h], dwp[:, C + H + h]
        gw.append(dwp[:, h * Fo:(h + 1) * Fo] + d1.unsqueeze(1) * a[:Fo].unsqueeze(0) + d2.unsqueeze(1) * a[Fo:].unsqueeze(0))
        ga.append(torch.cat([ws[h].t() @ d1, ws[h].t() @ d2]))
    return torch.stack(gw), torch.stack(ga)


# ----------------------------------------------------------------------------- seeded graphs
EDGES_NMAX = 80
HUB = 3                      # index of the hub graph in the edges batch
HUB_DEGREES = (4, 5, 8, 9, 16, 17)


def _random_block(n, p, gen):
    return ((torch.rand(n, n, generator=gen) < p).float() * (1 - torch.eye(n)))


def edges_batch():
    """(adj [5, 80, 80], sizes): a full graph (no ghost row), a 1-node graph (self loop), a graph without any edge, a hub graph
    and a graph with an isolated real node.  Non-symmetric throughout.
    Hub graph (76 nodes): row 0 has the 70 columns 1..70, column 75 has the 70 rows 1..70; rows 2..7 have exactly 4, 5, 8, 9, 16,
    17 entries, columns 10..15 have exactly 4, 5, 8, 9, 16, 17 entries; nodes 71..74 form a directed cycle."""
    N = EDGES_NMAX
    gen = torch.Generator().manual_seed(20)
    sizes = [N, 1, 6, 76, 12]
    adj = torch.zeros(5, N, N)
    adj[0] = _random_block(N, 0.1, gen)
    adj[1, 0, 0] = 1.0
    a = torch.zeros(76, 76)
    a[0, 1:71] = 1.0
    a[1:71, 75] = 1.0
    for r, deg in zip(range(2, 8), HUB_DEGREES):                  # row r: column 75 + (deg - 1) of the columns 40..
        a[r, 40:40 + deg - 1] = 1.0
    for c, deg in zip(range(10, 16), HUB_DEGREES):                # column c: row 0 + (deg - 1) of the rows 40..
        a[40:40 + deg - 1, c] = 1.0
    for k in range(71, 75):
        a[k, 71 + (k - 70) % 4] = 1.0
    adj[HUB, :76, :76] = a
    b = _random_block(12, 0.3, gen)
    b[5, :] = 0.0
    b[:, 5] = 0.0
    adj[4, :12, :12] = b
    return adj, np.asarray(sizes, dtype=np.int64)


BLOCKS_NMAX = 6
BLOCKS_B = (1, 31, 33, 257)


def blocks_batch(B):
    """(adj [B, 6, 6], sizes): B graphs of 1-6 nodes for the per-graph blocks of the uniform term's gradient.  A 6-node graph is a
    directed cycle with chords: every column has an entry, so its list of edge-less columns is EMPTY in both layouts, next to
    graphs with listed columns; graphs of 1-5 nodes have fewer rows than P = 8 or 7 in the ghost layout."""
    N = BLOCKS_NMAX
    gen = torch.Generator().manual_seed(300 + B)
    sizes = [3] if B == 1 else [1 + (k * 5 + k // 6) % 6 for k in range(B)]
    adj = torch.zeros(B, N, N)
    for b, n in enumerate(sizes):
        if n == N:
            a = _random_block(n, 0.2, gen)
            for k in range(n):
                a[k, (k + 1) % n] = 1.0
        else:
            a = _random_block(n, 0.4, gen)
            if b % 4 == 1:
                a.zero_()                                         # a graph without any edge
            elif b == 0 and n > 1:
                a[0, 1] = 1.0                                     # (B = 1: the batch has an entry)
        adj[b, :n, :n] = a
    return adj, np.asarray(sizes, dtype=np.int64)


_batches = {}


def batch(name):
    """'edges' or 'blocks<B>' -> (adj, sizes), built once"""
    if name not in _batches:
        _batches[name] = edges_batch() if name == "edges" else blocks_batch(int(name[6:]))
    return _batches[name]


_layouts = {}


def layout(name, kind):
    if (name, kind) not in _layouts:
        _layouts[(name, kind)] = Layout(*batch(name), kind)
    return _layouts[(name, kind)]


# ----------------------------------------------------------------------------- seeded inputs
def score_margin(hp, L, H, Fh):
    """min |s_row[i, h] + s_col[j, h]| over all entries (i, j) and heads, of the float32 sum and of the exact one"""
    C = H * Fh
    i, j = L.entries()
    if i.numel() == 0:
        return float("inf")
    s32 = (hp[i, C:C + H] + hp[j, C + H:C + 2 * H]).abs().min().item()
    s64 = (hp[i, C:C + H].double() + hp[j, C + H:C + 2 * H].double()).abs().min().item()
    return min(s32, s64)


def make_hp(L, H, Fh, Ns, seed, extreme=False):
    """float32 [R, Ns]: features ~ N(0, 1); scores ~ N(0, 1), or uniform in [-30, 30] (``extreme``: e spans +-60); pad columns 0.
    Rows whose score comes within MARGIN of the kink of LeakyReLU at some entry are redrawn until none does."""
    C = H * Fh
    gen = torch.Generator().manual_seed(seed)
    hp = torch.zeros(L.R, Ns)
    hp[:, :C] = torch.randn(L.R, C, generator=gen)

    def scores(n):
        return (torch.rand(n, H, generator=gen) * 60 - 30) if extreme else torch.randn(n, H, generator=gen)

    hp[:, C:C + H] = scores(L.R)
    hp[:, C + H:C + 2 * H] = scores(L.R)
    i, j = L.entries()
    for _ in range(100):
        t32 = hp[i, C:C + H] + hp[j, C + H:C + 2 * H]
        t64 = hp[i, C:C + H].double() + hp[j, C + H:C + 2 * H].double()
        bad = ((t32.abs() < 2 * MARGIN) | (t64.abs() < 2 * MARGIN)).any(dim=1)
        if not bad.any():
            break
        rows = torch.unique(i[bad])
        hp[rows, C:C + H] = scores(rows.numel())
    assert score_margin(hp, L, H, Fh) >= MARGIN
    return hp


GRID = [(1, 4), (8, 4), (3, 8), (8, 8), (5, 16), (8, 16), (2, 32), (7, 32), (8, 32), (1, 64), (3, 64), (4, 64)]
PER_LPH = [(8, 4), (3, 8), (5, 16), (7, 32), (3, 64)]        # one pair per LPH: apply_elu = 0, dropout, readout form, wide strides
BLOCKS_HF = (2, 16)
EXTREME_HF = (4, 16)
KINDS = ("ghost1", "padded")


def input_keys():
    """(batch, layout kind, H, Fh, wide, extreme) of every hp the GPU module uses"""
    keys = [("edges", k, H, Fh, False, False) for k in KINDS for (H, Fh) in GRID]
    keys += [("edges", k, H, Fh, True, False) for k in KINDS for (H, Fh) in PER_LPH]
    keys += [("blocks%d" % B, k) + BLOCKS_HF + (False, False) for k in KINDS for B in BLOCKS_B]
    keys += [("edges", k) + EXTREME_HF + (False, True) for k in KINDS]
    return keys


_inputs = {}


def inputs(name, kind, H, Fh, wide=False, extreme=False):
    """(layout, hp [R, Ns] float32, Ns) of one key; wide: eight more (zeroed) pad columns"""
    key = (name, kind, H, Fh, wide, extreme)
    if key not in _inputs:
        L = layout(name, kind)
        Ns = packed_width(H, Fh) + (8 if wide else 0)
        seed = ((H * 64 + Fh) * 2 + KINDS.index(kind)) * 1024 + sum(map(ord, name)) % 997 + (500 if extreme else 0) + (250 if wide else 0)
        _inputs[key] = (L, make_hp(L, H, Fh, Ns, seed, extreme), Ns)
    return _inputs[key]
