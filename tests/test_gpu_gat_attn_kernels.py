"""The fused GAT attention kernels (csrc/gat_fused.hip) one by one through the C ABI against tests/gat_attn_ref.py in float64:
gat_col_stats + gat_attn_fwd (tsgnn_gat_attn_fwd_f32), gat_attn_bwd (tsgnn_gat_attn_bwd_f32 / _bwd_ro_f32), gat_score_rowsum,
gat_pack, gat_unpack.  The input is a random packed projection hp [R, Ns] with no product in front; the structure (CSR, its
transpose, the list of edge-less columns, the entry map) comes from the product's own builders, so the kernels are fed what the
product feeds them.  tests/test_gat_attn_ref_host.py ties the reference to the pinned oracle and checks the inputs' guarantees.

Every piecewise decision is taken on an INPUT: LeakyReLU's branch on s_row[i] + s_col[j], which the inputs keep >= 1e-3 away from
0 at every entry; ELU' on the y handed to the backward (the forward KERNEL's y, given to the reference as well); the readout's
winners are ro_arg.  So every element of every output is held to a rounding-sized bound.

Every output buffer is prefilled with NaN: what a kernel must write is compared, what it must zero (the pad columns C+2H .. Ns-1 of
dhp, the statistics of edge-less columns, W''s pad columns) is compared with 0 exactly, what it must not touch (columns >= Ns of a
wider ldh, columns >= Co of a wider ldy) must still be NaN.  The pad columns of hp are NaN on the device: nothing may read them.
Before every launch the test asserts on the CPU that index arrays are in range, pointer arrays monotone and buffers of the size the
header states: a wrong test fails on the host.

Tolerance (fp32_yardstick.py), for every float tensor — y, m, 1/Z, S and the three column blocks of dhp each on their own:

    max|hip - ref64|  <=  K * max( max|cpu32 - ref64| , 2**-23 * max|ref64| ),   K = 8

Every test prints its ratios  max|hip - ref64| / yardstick  before asserting.  The largest ratio per output measured on the MI355X
over the whole module (1018 checks):

    gat_col_stats     m 0.46 (H1 Fh64 padded)           1/Z 1.00 (H5 Fh16 padded, dropout)
    gat_attn_fwd      y 2.65 (H8 Fh4 padded, mean, dropout)
    gat_attn_bwd      dh 1.38 (H5 Fh16 padded, mean, dropout, readout)      d s_col 4.00 (H5 Fh16 ghost1, mean, readout)
                      S 2.07 (H8 Fh4 padded, mean, wide)
    gat_score_rowsum  d s_row 1.70 (blocks1 ghost1 H2 Fh16)
    gat_pack          score columns 2.25 (H3 Fin300 Fo64); the heads' columns are bit-exact copies
    gat_unpack        gw 1.00 (H1 Fin13 Fo4)            ga 4.23 (H1 Fin300 Fo4)

The kernels' __expf stays inside K = 8 everywhere, the extreme-score cell included, so there is no K_EXP and no table of exceptions.

Cells: (H, Fh) in GRID covers every LPH in {1, 2, 4, 8, 16}, full waves (H * LPH = 64), partly live waves and EB = 8 at H = 8, each
with concat + ELU and mean + ELU in both layouts (ragged ghost-representative with row_graph; padded with row_graph NULL); one pair
per LPH also without ELU, with attention dropout p = 0.3 (padded only, as gat_fused.batch_ok decides), in the readout form, and with
wider strides ldh, ldy, lddy and eight more pad columns.  The edges batch has rows and columns of degree 4, 5, 8, 9, 16, 17 and 70
(entry batches of 8 in the forward, the col_t reload of the backward, the eight-lane loops of the statistics), a graph without
edges, a 1-node graph, a full graph and an isolated real node.
"""
import numpy as np
import pytest
import torch

import gat_attn_ref as G
from fp32_yardstick import K_DEFAULT, _check

pytestmark = pytest.mark.gpu

NAN = float("nan")
SLOPE = 0.2
EINVAL, EUNSUPPORTED = -1, -3
K = K_DEFAULT
DROP_P, DROP_SEED = 0.3, 0x1234567887654321


def _nat():
    from two_stage_gnn_amd import _native as nat
    return nat


@pytest.fixture(autouse=True)
def _end_the_run_at_a_device_error():
    """these tests launch kernels on raw pointers: after a launch that failed on the device, nothing more is started"""
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit("device error after a kernel test, no further launches: %s" % e, returncode=3)


def _rc(name, *args):
    """the entry point's return code (nat.call raises on every non-zero one)"""
    nat = _nat()
    return getattr(nat.lib(), "tsgnn_" + name)(*[nat._arg(a) for a in args], nat.stream_handle())


def nan_buf(*shape):
    return torch.full(shape, NAN, dtype=torch.float32, device="cuda")


def dev(t, ld=None, cols=None):
    """[rows, ld] float32 on the device: the first ``cols`` columns of t, NaN everywhere else"""
    rows, W = t.shape
    cols = W if cols is None else cols
    b = torch.full((rows, ld or W), NAN, dtype=torch.float32)
    b[:, :cols] = t[:, :cols]
    return b.cuda()


def _monotone(p, last):
    p = p.cpu().long()
    return p[0].item() == 0 and bool((p[1:] >= p[:-1]).all()) and p[-1].item() == last


# ----------------------------------------------------------------------------- device structure, from the product's builders
class Struct:
    def __init__(self, name, kind):
        from two_stage_gnn_amd import attention as att
        from two_stage_gnn_amd.graph import GraphBatch
        self.L = L = G.layout(name, kind)
        adj, sizes = G.batch(name)
        if kind == "ghost1":
            self.g = g = GraphBatch.from_dense_ghost1(adj.cuda(), sizes)
        else:
            self.g = g = GraphBatch.from_dense(adj.cuda(), layout="padded")
        self.R, self.B, self.nmax, self.nnz = int(g.total_rows), int(g.B), int(g.nmax), int(g.nnz)
        self.rp_t, self.col_t, src_e_t = g.transpose_map()
        self.eperm = att._inverse_entry_map(g, src_e_t)
        self.row_seg = att._row_seg(g)
        assert (self.row_seg is not None) == (kind == "ghost1")
        self._iso = {}
        # ---- on the CPU, before anything is launched: the structure is the reference's, every index in range, every pointer monotone
        R, nnz = self.R, self.nnz
        assert R == L.R and self.B == L.B and self.nmax == L.N and nnz == int(L.mask.sum()) and nnz > 0
        assert g.graph_ptr.cpu().tolist() == L.graph_ptr.tolist() and g.row_graph.cpu().tolist() == L.row_graph.tolist()
        assert g.rowptr.numel() == R + 1 and self.rp_t.numel() == R + 1 and _monotone(g.rowptr, nnz) and _monotone(self.rp_t, nnz)
        assert g.col.numel() == nnz and self.col_t.numel() == nnz and self.eperm.numel() == nnz
        col, col_t, eperm = g.col.cpu().long(), self.col_t.cpu().long(), self.eperm.cpu().long()
        assert 0 <= col.min() and col.max() < R and 0 <= col_t.min() and col_t.max() < R
        assert sorted(eperm.tolist()) == list(range(nnz))
        row_of = torch.repeat_interleave(torch.arange(R), (g.rowptr[1:] - g.rowptr[:-1]).cpu().long())
        row_of_t = torch.repeat_interleave(torch.arange(R), (self.rp_t[1:] - self.rp_t[:-1]).cpu().long())
        i, j = L.entries()
        assert sorted((row_of * R + col).tolist()) == sorted((i * R + j).tolist())
        assert torch.equal(col_t[eperm], row_of) and torch.equal(row_of_t[eperm], col)        # entry e = (i, j) sits at eperm[e] in A^T
        if kind == "ghost1":
            assert g.row_mult.cpu().tolist() == L.row_mult.tolist()
        self.deg_t = (self.rp_t[1:] - self.rp_t[:-1]).cpu().long()

    def iso(self, H):
        """(iso_row [R, H], (iso_idx, iso_w, iso_ptr)) as _GatLayer hands them over; checked on the CPU"""
        from two_stage_gnn_amd import attention as att
        if H not in self._iso:
            iso = att._isolated_columns(self.g, self.rp_t, self.R, H)
            lst = att._isolated_list(self.g, iso)
            assert lst is not None, "the product would not send this batch to the fused kernels"
            idx, w, ptr = lst
            n = int(idx.numel())
            assert tuple(iso.shape) == (self.R, H) and ptr.numel() == self.B + 1 and _monotone(ptr, n) and w.numel() == n
            ic = idx.cpu().long()
            assert 0 <= ic.min() and ic.max() < self.R and (self.deg_t[ic] == 0).all() and n == int((self.deg_t == 0).sum())
            assert torch.equal(w.cpu(), torch.from_numpy(self.L.row_mult)[ic])
            pc = ptr.cpu().long()
            for b in range(self.B):                                      # every listed column lies in its own graph
                rows = ic[pc[b]:pc[b + 1]]
                assert ((rows >= self.L.graph_ptr[b]) & (rows < self.L.graph_ptr[b + 1])).all()
            self._iso[H] = (iso, lst)
        return self._iso[H]


_structs = {}


def struct(name, kind):
    if (name, kind) not in _structs:
        _structs[(name, kind)] = Struct(name, kind)
    return _structs[(name, kind)]


# ----------------------------------------------------------------------------- launches
class Cell:
    """one input (batch, layout, H, Fh) with one set of flags and strides"""

    def __init__(self, name, kind, H, Fh, mean=False, elu=True, drop=0.0, wide=False, extreme=False):
        self.S = struct(name, kind)
        self.L, self.hp, self.Ns = G.inputs(name, kind, H, Fh, wide, extreme)
        self.H, self.Fh, self.C, self.mean, self.elu, self.drop = H, Fh, H * Fh, bool(mean), bool(elu), float(drop)
        self.Co = Fh if mean else H * Fh
        self.ldh = self.Ns + (4 if wide else 0)
        self.ldy = self.Co + (4 if wide else 0)
        self.lddy = self.Co + (8 if wide else 0)
        self.what = "%s %s H%d Fh%d %s%s%s%s%s" % (name, kind, H, Fh, "mean" if mean else "concat", "+elu" if elu else "",
                                                   " drop" if drop else "", " wide" if wide else "", " extreme" if extreme else "")
        self.mult = self._mults() if drop else None
        self._fwd = None
        self._ref = None

    def _mults(self):
        """[H][B, N, N]: the multipliers the kernels apply (tsgnn_gat_dropout_mult_f32), for the padded layout's rows b * N + i"""
        assert self.L.kind == "padded"                                  # (batch_ok never sends a ragged batch under dropout)
        B, N, H = self.L.B, self.L.N, self.H
        blocks = []
        for b in range(B):
            t = nan_buf(N, N, H)
            _nat().call("gat_dropout_mult_f32", self.drop, DROP_SEED, None, b * N, N, b * N, N, H, t)
            blocks.append(t.cpu())
        full = torch.stack(blocks)
        nz = full[full != 0]
        assert (nz == nz[0]).all() and abs(nz[0].item() - 1.0 / (1.0 - self.drop)) < 1e-6      # every multiplier is 0 or 1 / (1 - p)
        assert abs(float((full == 0).float().mean()) - self.drop) < 0.02
        return [full[..., h].contiguous() for h in range(H)]

    # --- references, once per cell
    def ref_fwd(self):
        if self._ref is None:
            a = (self.L, self.H, self.Fh, SLOPE, self.mean, self.elu, self.mult)
            self._ref = (G.attn_fwd(self.hp.double(), *a), G.attn_fwd(self.hp, *a),
                         G.col_stats(self.hp.double(), *a[:4]), G.col_stats(self.hp, *a[:4]))
        return self._ref

    def ref_bwd(self, y_given, **grad):
        a = (self.L, self.H, self.Fh, SLOPE, self.mean, self.elu, y_given)
        return G.attn_bwd(self.hp.double(), *a, mult=self.mult, **grad), G.attn_bwd(self.hp, *a, mult=self.mult, **grad)

    # --- forward: statistics + y
    def fwd(self):
        """(hp on the device, stat [R, H, 2], y [R, ldy]) of tsgnn_gat_attn_fwd_f32, launched once per cell"""
        if self._fwd is None:
            S, g, H = self.S, self.S.g, self.H
            _, (i_idx, i_w, i_ptr) = S.iso(H)
            hp = dev(self.hp, self.ldh, cols=self.C + 2 * H)
            stat, y = nan_buf(S.R, H, 2), nan_buf(S.R, self.ldy)
            assert hp.shape == (S.R, self.ldh) and self.ldh >= self.Ns >= self.C + 2 * H and self.ldh % 4 == 0 and self.ldy % 4 == 0
            _nat().call("gat_attn_fwd_f32", hp, self.ldh, g.rowptr, g.col, S.rp_t, S.col_t, S.R, H, self.Fh, SLOPE, S.row_seg, S.nmax,
                        i_idx, i_w, i_ptr, 1.0 / S.nmax, int(self.mean), int(self.elu), self.drop, DROP_SEED if self.drop else 0, None,
                        stat, y, self.ldy)
            assert _nat().last_kernel() == "gat_attn_fwd_kernel<%d,%s>" % (self.Fh // 4, "true" if self.drop else "false")
            self._fwd = (hp, stat, y)
        return self._fwd

    def check_fwd(self):
        hp, stat, y = self.fwd()
        y64, y32, (m64, z64), (m32, z32) = self.ref_fwd()
        yc, st = y.cpu(), stat.cpu()
        assert torch.isnan(yc[:, self.Co:]).all(), self.what + ": y written beyond its Co columns"
        _check("stat m    | " + self.what, st[:, :, 0], m64, m32, K)
        _check("stat 1/Z  | " + self.what, st[:, :, 1], z64, z32, K)
        assert (st[self.S.deg_t == 0] == 0).all(), self.what + ": an edge-less column's statistics are (0, 0)"
        _check("fwd y     | " + self.what, yc[:, :self.Co], y64, y32, K)
        assert torch.isfinite(yc[:, :self.Co]).all()

    # --- backward: gat_attn_bwd + gat_score_rowsum -> completed dhp, S
    def check_bwd(self, ro=False, seed=1):
        S, g, H, C, Co = self.S, self.S.g, self.H, self.C, self.Co
        nat = _nat()
        hp, stat, y = self.fwd()
        iso_row, (i_idx, i_w, i_ptr) = S.iso(H)
        gen = torch.Generator().manual_seed(seed + 7 * H + self.Fh)
        P = int(nat.lib().tsgnn_gat_bwd_parts(S.B))
        assert P == max(1, min(8, 256 // S.B))
        dhp = nan_buf(S.R, self.ldh)
        t1, t2, Sb = nan_buf(max(S.nnz, 1), H), nan_buf(max(S.nnz, 1), H), nan_buf(S.R, H)
        dupart = nan_buf(S.B * P * C)
        us = 1.0 / S.nmax
        tail = (g.graph_ptr, S.B, i_idx, i_w, i_ptr, iso_row, H, us, self.drop, DROP_SEED if self.drop else 0, None, stat, dhp, self.Ns,
                t1, t2, Sb, dupart)
        head = (hp, self.ldh, y, self.ldy)
        mid = (S.rp_t, S.col_t, S.R, H, self.Fh, SLOPE, int(self.mean), int(self.elu))
        assert g.graph_ptr.numel() == S.B + 1 and iso_row.stride(0) == H and dupart.numel() == S.B * P * C
        if ro:
            # winners: a random row of graph b per column (the ghost representative and repeated winners occur)
            rows = torch.from_numpy(self.L.rows_per_graph).unsqueeze(1)
            arg = (torch.from_numpy(self.L.graph_ptr[:-1]).unsqueeze(1) + (torch.rand(S.B, Co, generator=gen) * rows).long().clamp(max=rows - 1))
            arg = arg.to(torch.int32)
            dout = torch.randn(S.B, Co, generator=gen)
            grad = dict(ro_arg=arg, ro_dout=dout)
            ro_ldo = Co + 4
            assert (arg.long() >= torch.from_numpy(self.L.graph_ptr[:-1]).unsqueeze(1)).all()
            assert (arg.long() < torch.from_numpy(self.L.graph_ptr[1:]).unsqueeze(1)).all() and g.row_graph.numel() == S.R
            nat.call("gat_attn_bwd_ro_f32", *head, None, 0, *mid, *tail, dev(dout, ro_ldo), ro_ldo, arg.cuda(), g.row_graph)
        else:
            dy = torch.randn(S.R, Co, generator=gen)
            grad = dict(dy=dy)
            nat.call("gat_attn_bwd_f32", *head, dev(dy, self.lddy), self.lddy, *mid, *tail)
        assert nat.last_kernel() == "gat_attn_bwd_kernel<%d,%s>" % (self.Fh // 4, "true" if self.drop else "false")
        fin = self.drop == 0.0                                           # (with dropout the backward completes the listed columns itself)
        nat.call("gat_score_rowsum_f32", g.rowptr, g.col, S.eperm, t1, t2, Sb, S.R, H, dhp, self.ldh, C, dupart if fin else None, S.B,
                 i_idx if fin else None, i_w if fin else None, i_ptr if fin else None, us)
        (d64, S64), (d32, S32) = self.ref_bwd(y.cpu()[:, :Co], **grad)
        what = self.what + (" readout" if ro else "")
        d = dhp.cpu()
        assert torch.isnan(d[:, self.Ns:]).all(), what + ": dhp written beyond its Ns columns"
        assert (d[:, C + 2 * H:self.Ns] == 0).all(), what + ": the pad columns of dhp are zero"
        assert not d64[:, C + 2 * H:].any()
        _check("bwd dh    | " + what, d[:, :C], d64[:, :C], d32[:, :C], K)
        _check("bwd ds_col| " + what, d[:, C + H:C + 2 * H], d64[:, C + H:C + 2 * H], d32[:, C + H:C + 2 * H], K)
        _check("row ds_row| " + what, d[:, C:C + H], d64[:, C:C + H], d32[:, C:C + H], K)
        _check("bwd S     | " + what, Sb, S64, S32, K)
        assert torch.isfinite(d[:, :self.Ns]).all()


_cells = {}


def cell(*a, **kw):
    k = (a, tuple(sorted(kw.items())))
    if k not in _cells:
        _cells[k] = Cell(*a, **kw)
    return _cells[k]


def _flag_sets(H, Fh):
    """concat + ELU and mean + ELU everywhere; one pair per LPH also without ELU"""
    return [(False, True), (True, True)] + ([(False, False), (True, False)] if (H, Fh) in G.PER_LPH else [])


_ids = lambda hf: "H%d-Fh%d" % hf          # noqa: E731


# ----------------------------------------------------------------------------- (a) forward + column statistics
@pytest.mark.parametrize("kind", G.KINDS)
@pytest.mark.parametrize("HF", G.GRID, ids=_ids)
def test_attn_fwd_grid(HF, kind):
    assert _nat().lib().tsgnn_gat_fused_supported(*HF) == 1
    for mean, elu in _flag_sets(*HF):
        cell("edges", kind, *HF, mean=mean, elu=elu).check_fwd()


# ----------------------------------------------------------------------------- (b) backward + score row sums
@pytest.mark.parametrize("kind", G.KINDS)
@pytest.mark.parametrize("HF", G.GRID, ids=_ids)
def test_attn_bwd_grid(HF, kind):
    for mean, elu in _flag_sets(*HF):
        cell("edges", kind, *HF, mean=mean, elu=elu).check_bwd()


@pytest.mark.parametrize("kind", G.KINDS)
@pytest.mark.parametrize("HF", G.PER_LPH, ids=_ids)
def test_attn_bwd_readout_form(HF, kind):
    """dy[i, c] = (ro_arg[b, c] == i) ? ro_dout[b, c] : 0 formed on the fly (ro_ldo > Co)"""
    for mean in (False, True):
        cell("edges", kind, *HF, mean=mean).check_bwd(ro=True)


@pytest.mark.parametrize("kind", G.KINDS)
@pytest.mark.parametrize("HF", G.PER_LPH, ids=_ids)
def test_attn_wide_strides_and_pad_columns(HF, kind):
    """ldh = Ns + 4 with Ns - C - 2H in 8..11 zeroed pad columns, ldy = Co + 4, lddy = Co + 8"""
    for mean in (False, True):
        c = cell("edges", kind, *HF, mean=mean, wide=True)
        assert c.ldh > c.Ns and 8 <= c.Ns - c.C - 2 * c.H <= 11 and c.lddy > c.ldy > c.Co
        c.check_fwd()
        c.check_bwd()


# ----------------------------------------------------------------------------- (c) attention dropout
@pytest.mark.parametrize("HF", G.PER_LPH, ids=_ids)
def test_attn_dropout(HF):
    """p = 0.3 with the kernels' own multipliers handed to the reference; the backward completes the listed columns itself and
    gat_score_rowsum runs without a list, as _GatLayer.backward calls it"""
    for mean in (False, True):
        c = cell("edges", "padded", *HF, mean=mean, drop=DROP_P)
        c.check_fwd()
        c.check_bwd()
    c.check_bwd(ro=True)


# ----------------------------------------------------------------------------- (d) per-graph blocks of the uniform term
@pytest.mark.parametrize("kind", G.KINDS)
@pytest.mark.parametrize("B", G.BLOCKS_B)
def test_attn_graph_blocks(B, kind):
    """P = tsgnn_gat_bwd_parts(B) = 8, 8, 7, 1 row ranges per graph; graphs with fewer rows than P, graphs without a list"""
    assert int(_nat().lib().tsgnn_gat_bwd_parts(B)) == {1: 8, 31: 8, 33: 7, 257: 1}[B]
    c = cell("blocks%d" % B, kind, *G.BLOCKS_HF)
    c.check_fwd()
    c.check_bwd()
    c = cell("blocks%d" % B, kind, *G.BLOCKS_HF, mean=True)
    c.check_fwd()
    c.check_bwd(ro=True)


# ----------------------------------------------------------------------------- (e) extreme scores
@pytest.mark.parametrize("kind", G.KINDS)
def test_attn_extreme_scores(kind):
    """e spans +-60: the maximum is subtracted before every exp, nothing is inf or NaN"""
    c = cell("edges", kind, *G.EXTREME_HF, extreme=True)
    c.check_fwd()
    c.check_bwd()


# ----------------------------------------------------------------------------- (f) pack / unpack
def _pack_case(layers, seed, extra_pad=0):
    """layers [(H, Fin, Fo)] -> one launch of gat_pack and one of gat_unpack over a descriptor built by gat_fused._desc"""
    from two_stage_gnn_amd import gat_fused as gf
    nat = _nat()
    gen = torch.Generator().manual_seed(seed)
    assert 1 <= len(layers) <= 4
    host, lay_p, ptr_p, lay_u, ptr_u = [], [], [], [], []
    for H, Fin, Fo in layers:
        assert 1 <= H <= 8 and Fo % 4 == 0 and Fo <= 64 and Fin >= 1
        Ns = gf.packed_width(H, Fo) + extra_pad
        assert Ns == G.packed_width(H, Fo) + extra_pad
        ws = [torch.randn(Fin, Fo, generator=gen) for _ in range(H)]
        as_ = [torch.randn(2 * Fo, generator=gen) for _ in range(H)]
        dwp = torch.randn(Fin, Ns, generator=gen)
        wd, ad = [w.cuda() for w in ws], [a.cuda() for a in as_]
        wp, gw, ga = nan_buf(Fin, Ns), nan_buf(H, Fin, Fo), nan_buf(H, 2 * Fo)
        dwp_d = dev(dwp, cols=H * Fo + 2 * H)                            # (the pad columns of dW' are not read)
        host.append((H, Fin, Fo, Ns, ws, as_, dwp, wp, gw, ga, wd, ad, dwp_d))
        lay_p.append((H, Fin, Fo, Ns, wd, ad))
        ptr_p.append((wp, None, None))
        lay_u.append((H, Fin, Fo, Ns, wd, ad))
        ptr_u.append((dwp_d, gw, ga))
    d = gf._desc(lay_p, ptr_p)
    assert d.size == 1 + len(layers) * int(nat.lib().tsgnn_gat_pack_desc_words())
    nat.call("gat_pack_f32", d.ctypes.data)
    d = gf._desc(lay_u, ptr_u)
    nat.call("gat_unpack_f32", d.ctypes.data)
    for H, Fin, Fo, Ns, ws, as_, dwp, wp, gw, ga, *_ in host:
        what = "H%d Fin%d Fo%d" % (H, Fin, Fo)
        C = H * Fo
        w64, w32 = G.pack([w.double() for w in ws], [a.double() for a in as_], Ns), G.pack(ws, as_, Ns)
        wp = wp.cpu()
        assert torch.equal(wp[:, :C], w32[:, :C]), what + ": the heads' columns are copies"
        assert (wp[:, C + 2 * H:] == 0).all(), what + ": the pad columns of W' are zero"
        _check("pack W'   | " + what, wp[:, C:C + 2 * H], w64[:, C:C + 2 * H], w32[:, C:C + 2 * H], K)
        (gw64, ga64), (gw32, ga32) = G.unpack(dwp.double(), [w.double() for w in ws], [a.double() for a in as_]), G.unpack(dwp, ws, as_)
        _check("unpack gw | " + what, gw, gw64, gw32, K)
        _check("unpack ga | " + what, ga, ga64, ga32, K)


@pytest.mark.parametrize("Fo", [4, 8, 16, 32, 64])
def test_pack_unpack_grid(Fo):
    """single-layer descriptors over H x Fin (the KQ = 1024 / Fo row groups of gat_unpack: one ragged pass, several passes)"""
    for H in (1, 3, 8):
        for Fin in (1, 13, 89, 300):
            _pack_case([(H, Fin, Fo)], seed=Fo * 1000 + H * 10 + Fin, extra_pad=4 if Fin == 13 else 0)


def test_unpack_more_rows_than_one_pass():
    """Fin = 1100 at Fo = 4: more than 4 * KQ = 1024 rows, the row loop of gat_unpack takes a second trip"""
    _pack_case([(3, 1100, 4)], seed=11)


def test_pack_unpack_four_layers():
    """four different (H, Fin, Fo) in one launch: blk0 selects every layer"""
    _pack_case([(1, 13, 64), (3, 300, 8), (8, 1, 16), (2, 89, 32)], seed=12)


# ----------------------------------------------------------------------------- (g) refusals, decided before any launch
def _refusal_buffers(H, Fh, Ns, ldh):
    S = struct("edges", "ghost1")
    _, lst = S.iso(min(H, 8))
    C = H * Fh
    iso_row = torch.ones(S.R, H, device="cuda")                        # (sized for H, should a refusal ever fail to come)
    bufs = dict(hp=torch.zeros(S.R, max(ldh, Ns) + 4, device="cuda"), stat=nan_buf(S.R, H, 2), y=nan_buf(S.R, C + 4), dhp=nan_buf(S.R, max(ldh, Ns) + 4),
                t1=nan_buf(S.nnz, H), t2=nan_buf(S.nnz, H), Sb=nan_buf(S.R, H), dupart=nan_buf(S.B * 8 * C), dy=torch.zeros(S.R, C, device="cuda"),
                yin=torch.zeros(S.R, C, device="cuda"))
    return S, iso_row, lst, bufs


def _fwd_rc(H, Fh, Ns, ldh):
    S, iso_row, (i_idx, i_w, i_ptr), b = _refusal_buffers(H, Fh, Ns, ldh)
    g = S.g
    rc = _rc("gat_attn_fwd_f32", b["hp"], ldh, g.rowptr, g.col, S.rp_t, S.col_t, S.R, H, Fh, SLOPE, S.row_seg, S.nmax, i_idx, i_w, i_ptr,
             1.0 / S.nmax, 0, 1, 0.0, 0, None, b["stat"], b["y"], H * Fh)
    torch.cuda.synchronize()
    assert torch.isnan(b["stat"]).all() and torch.isnan(b["y"]).all()
    return rc


def _bwd_rc(H, Fh, Ns, ldh, dy=True, ro=False):
    S, iso_row, (i_idx, i_w, i_ptr), b = _refusal_buffers(H, Fh, Ns, ldh)
    g = S.g
    C = H * Fh
    arg = torch.zeros(S.B, C, dtype=torch.int32, device="cuda")
    dout = torch.zeros(S.B, C, device="cuda")
    rc = _rc("gat_attn_bwd_ro_f32", b["hp"], ldh, b["yin"], C, b["dy"] if dy else None, C, S.rp_t, S.col_t, S.R, H, Fh, SLOPE, 0, 1,
             g.graph_ptr, S.B, i_idx, i_w, i_ptr, iso_row, H, 1.0 / S.nmax, 0.0, 0, None, b["stat"], b["dhp"], Ns, b["t1"], b["t2"], b["Sb"],
             b["dupart"], dout if ro else None, C, arg if ro else None, g.row_graph if ro else None)
    torch.cuda.synchronize()
    for k in ("dhp", "t1", "t2", "Sb", "dupart"):
        assert torch.isnan(b[k]).all(), k
    return rc


@pytest.mark.parametrize("H,Fh", [(9, 4), (8, 64), (2, 12), (1, 128)])
def test_unsupported_head_shapes_are_refused(H, Fh):
    assert _nat().lib().tsgnn_gat_fused_supported(H, Fh) == 0
    Ns = G.packed_width(H, Fh)
    assert _fwd_rc(H, Fh, Ns, Ns) == EUNSUPPORTED
    assert _bwd_rc(H, Fh, Ns, Ns) == EUNSUPPORTED


def test_unsupported_strides_and_bad_gradient_sources_are_refused():
    H, Fh = 3, 8
    Ns = G.packed_width(H, Fh)
    assert _fwd_rc(H, Fh, Ns, Ns + 1) == EUNSUPPORTED and _bwd_rc(H, Fh, Ns, Ns + 1) == EUNSUPPORTED        # ldh % 4 != 0
    assert _bwd_rc(H, Fh, Ns + 68, Ns + 68) == EUNSUPPORTED                                                  # Ns - C - 2H > 64
    assert _bwd_rc(H, Fh, Ns, Ns, dy=True, ro=True) == EINVAL                                                # both sources
    assert _bwd_rc(H, Fh, Ns, Ns, dy=False, ro=False) == EINVAL                                              # neither
    S, iso_row, (i_idx, i_w, i_ptr), b = _refusal_buffers(H, Fh, Ns, Ns)
    assert _rc("gat_attn_bwd_f32", b["hp"], Ns, b["yin"], H * Fh, None, H * Fh, S.rp_t, S.col_t, S.R, H, Fh, SLOPE, 0, 1, S.g.graph_ptr, S.B,
               i_idx, i_w, i_ptr, iso_row, H, 1.0 / S.nmax, 0.0, 0, None, b["stat"], b["dhp"], Ns, b["t1"], b["t2"], b["Sb"],
               b["dupart"]) == EINVAL
    torch.cuda.synchronize()
    assert torch.isnan(b["dhp"]).all()
