"""The per-node-slot kernels of the GraphSage stack (csrc/sage_fused.hip, and the unfused fallback in csrc/bn_readout.hip) one by one
against tests/slot_ref.py in float64, over their whole dispatch grid.

Every piecewise decision of these kernels is taken on an INPUT — the ReLU mask on v, the readout winners are arg, the clamp flag is
rinv — so the kernel and the reference, fed the same bits, take the same branches and every element of every row can be held to a
rounding-sized bound.  v32 = normalize(u).float() and rinv32 = (1/|u|).float() go to the kernel, v32.double() and rinv32.double() to
the reference.  Every output buffer is prefilled with NaN: what the kernel must write is compared, what it must zero is compared
with 0 exactly, what it must not touch (the padding columns of strided outputs, rows beyond the launch) must still be NaN.

Tolerance, for every float tensor T (ref64: slot_ref in float64; cpu32: the SAME code with dtype=float32 on the CPU):

    max|hip - ref64|  <=  K * max( max|cpu32 - ref64| , 2**-23 * max|ref64| ),   K = 8

The yardstick is the reference's own fp32 rounding, never the kernel; 8 allows for the kernels' different summation order (wave
trees, then waves in fixed groups of four).  Every test prints its ratio  max|hip - ref64| / yardstick  before asserting.
No cell needs a K of its own: the largest ratio measured over the whole module is 1.9, so there is no table of exceptions.

Dispatch cells by parametrisation (B -> block threads BT: <= 32: 256, <= 64: 512, else 1024; F/4 -> (TPR, NV): <= 8: (8, 1),
<= 16: (8, 2) or, for B <= 16, (16, 1), else (8, 4)):
    B in {1, 16}        BT 256, the wide16 cell <16,1,256> at F in {36, 64}
    B in {17, 32}       BT 256, <8,2,256> at F in {36, 64}
    B in {33, 64}       BT 512;   B in {65, 128}  BT 1024
    F in {4, 20, 32}    NV 1 (ragged, ragged, exactly filled);  {36, 64}  NV 2;  {100, 128}  NV 4
    backward only:      F == 128 and B <= 32 -> <16,2,512>, B in {33, 64} -> <16,2,1024>, B in {65, 128} -> <8,4,1024>
    slot_post_wgrad:    K_in in {1, 3, 32} MT 1, {33, 64} MT 2, {89} MT 3, {97, 128} MT 4
"""
import numpy as np
import pytest
import torch

import slot_ref as S
from fp32_yardstick import EPS32, K_DEFAULT, _check, _ratio

pytestmark = pytest.mark.gpu

NAN = float("nan")
NMAX = 11
GRID_B = [1, 16, 17, 32, 33, 64, 65, 128]
GRID_F = [4, 20, 32, 36, 64, 100, 128]
EUNSUPPORTED = -3


def _nat():
    from two_stage_gnn_amd import _native as nat
    return nat


# ----------------------------------------------------------------------------- tolerance (_ratio, _check: fp32_yardstick.py)
def _check_rows(what, hip, ref64, cpu32, special_rows, K=K_DEFAULT):
    """the rows of a clamped norm carry gradients 1e12 times the others': they are held to their own scale"""
    hip = hip.detach().cpu()
    keep = torch.ones(ref64.size(0), dtype=torch.bool)
    keep[special_rows] = False
    _check(what, hip[keep], ref64[keep], cpu32[keep], K)
    _check(what + " (clamped rows)", hip[~keep], ref64[~keep], cpu32[~keep], K)


# ----------------------------------------------------------------------------- sizes
def sizes_of(profile, B, nmax=NMAX):
    """ragged: sizes[0] = 9 (the first ghost user of a slot is never graph 0 below slot 9), a graph of one node, two graphs of equal
    size, every size in 1..9 — so slots 9 and 10 have no real candidate, every graph uses their ghost rows (first and last wave of the
    workgroup included), and slot 0 is present everywhere: its ghost row is unused.  full: one graph fills all nmax slots."""
    if B == 1:
        return [7] if profile == "ragged" else [nmax]
    tail = (1, 4, 4, 7, 2, 9, 3, 5, 8, 6)
    s = [9] + [tail[i % 10] for i in range(B - 1)]
    if profile == "full":
        s[B // 2] = nmax
    return s


class Case:
    """one batch layout with its operands on the CPU (float32 bits) and the device-side structure"""

    def __init__(self, B, F, ghosts, profile="ragged", pad=0, clamp=False, seed=0):
        from two_stage_gnn_amd.graph import GraphBatch
        self.B, self.F, self.ghosts = B, F, ghosts
        sizes = sizes_of(profile, B)
        self.L = L = S.Layout(sizes, NMAX, NMAX if ghosts else 0, n_real=sum(sizes) + pad)
        self.g = g = GraphBatch.structure_only(sizes, NMAX, "cuda", ghosts=ghosts)
        assert g.graph_ptr.cpu().tolist() == L.graph_ptr.tolist() and g.slot_count.cpu().tolist() == L.slot_count.tolist()
        gen = torch.Generator().manual_seed(((B * 131 + F) * 2 + int(ghosts)) * 16 + seed + (5 if profile == "full" else 0))
        self.gen = gen
        u = torch.randn(L.rows, F, dtype=torch.float64, generator=gen)
        self.clamped_rows = []
        if clamp:
            # a clamped norm (|u| < 1e-12: v = u / 1e-12, rinv = 1e12, no projection in the backward): two all-zero rows — a real one and
            # the ghost row of slot 9, which every graph uses — and two rows of norm 0.5e-12, whose v is NOT zero
            zero_rows, tiny_rows = [int(L.graph_ptr[1])], [1]
            if ghosts:
                zero_rows.append(L.n_real + 9)
                tiny_rows.append(L.n_real + 10)
            for r in zero_rows:
                u[r] = 0.0
            for r in tiny_rows:
                u[r] = u[r].abs() * (0.5e-12 / u[r].norm())
            self.clamped_rows = zero_rows + tiny_rows
        nrm = u.norm(dim=1, keepdim=True).clamp(min=1e-12)
        self.v32 = (u / nrm).float()
        self.rinv32 = (1.0 / nrm[:, 0]).float()
        assert not ((self.v32 == 0) & torch.signbit(self.v32)).any()
        self.v64, self.rinv64 = self.v32.double(), self.rinv32.double()
        for r in self.clamped_rows:
            assert self.rinv32[r].item() >= S.CLAMPED
        self._fwd = {}
        self._bwd = {}
        # gradients (float32 bits); dxs is NaN where the kernel must not read it: ghost rows and capacity padding
        self.dxs = torch.randn(L.rows, F, generator=gen)
        self.dxs2 = torch.randn(L.rows, F, generator=gen)
        for t in (self.dxs, self.dxs2):
            t[int(L.graph_ptr[-1]):] = NAN
        self.dout = torch.randn(B, F, generator=gen)
        # winners drawn by the test: a random candidate of graph b per column (ghost winners and repeated winners occur);
        # one graph has no winner in every third column
        ncand = torch.full((B,), NMAX) if ghosts else torch.as_tensor(np.asarray(sizes))
        n = (torch.rand(B, F, generator=gen) * ncand[:, None]).long().clamp(max=NMAX - 1)
        self.arg = torch.gather(L.idx, 1, n).to(torch.int32)
        assert (self.arg >= 0).all()
        self.arg[B // 3, 0::3] = -1

    def dev_struct(self):
        return (self.g.graph_ptr, self.g.slot_count, self.B, NMAX, self.L.n_real, self.L.n_ghost)

    # --- references (computed once per case and flag set)
    def fwd_ref(self, relu):
        if relu not in self._fwd:
            self._fwd[relu] = (S.slot_bn(self.v64, self.L, relu=relu), S.slot_bn(self.v64, self.L, relu=relu, dtype=torch.float32))
        return self._fwd[relu]

    def bwd_ref(self, relu=True, bn=True, dxs=True, dxs2=False, ro=True):
        key = (relu, bn, dxs, dxs2, ro)
        if key not in self._bwd:
            kw = dict(dxs=self.dxs if dxs else None, dxs2=self.dxs2 if dxs2 else None, dout=self.dout if ro else None,
                      arg=self.arg if ro else None, relu=relu, bn=bn)
            self._bwd[key] = (S.slot_post_bwd(self.v64, self.rinv64, self.L, **kw),
                              S.slot_post_bwd(self.v64, self.rinv64, self.L, dtype=torch.float32, **kw))
        return self._bwd[key]


_cases = {}


def case(*key, **kw):
    k = (key, tuple(sorted(kw.items())))
    if k not in _cases:
        _cases[k] = Case(*key, **kw)
    return _cases[k]


# ----------------------------------------------------------------------------- device buffers
def dev(t, ld=None):
    """[rows, ld] float32 on the device: t in the first columns, NaN in the padding"""
    rows, F = t.shape
    b = torch.full((rows, ld or F), NAN, dtype=torch.float32)
    b[:, :F] = t
    return b.cuda()


def nan_buf(*shape):
    return torch.full(shape, NAN, dtype=torch.float32, device="cuda")


def _untouched(buf, F):
    """the padding columns of a strided output are still NaN"""
    return buf.size(1) == F or bool(torch.isnan(buf[:, F:]).all().item())


def _bt(B):
    """threads of a slot workgroup"""
    return 256 if B <= 32 else (512 if B <= 64 else 1024)


def _table_cell(kernel, B, F):
    """the instantiation the dispatch table picks, as tsgnn_last_kernel() names it; the wide16 cell needs TSGNN_SLOT_WIDE16 unset or
    non-zero (its default), which the grid tests require so that the cell cannot drop out of the grid unnoticed"""
    import os
    assert os.environ.get("TSGNN_SLOT_WIDE16", "1") != "0", "TSGNN_SLOT_WIDE16=0 removes the <16,1,256> cell from the grid"
    if 32 < F <= 64 and B <= 16:
        return "%s<16,1,256>" % kernel
    return "%s<8,%d,%d>" % (kernel, 1 if F <= 32 else (2 if F <= 64 else 4), _bt(B))


def run_fwd(c, relu, ldv=None, ldy=None, zero=None):
    """tsgnn_slot_bn_fwd_f32 -> mean, rstd, y on the CPU"""
    L, F = c.L, c.F
    v = dev(c.v32, ldv)
    mean, rstd, y = nan_buf(NMAX), nan_buf(NMAX), nan_buf(L.rows, ldy or F)
    _nat().call("slot_bn_fwd_f32", *c.dev_struct(), v, v.stride(0), F, int(relu), mean, rstd, y, y.stride(0), zero,
                0 if zero is None else zero.numel())
    assert _untouched(y, F)
    return mean, rstd, y[:, :F]


def check_fwd(what, c, relu, mean, rstd, y):
    (m64, r64, y64), (m32, r32, y32) = c.fwd_ref(relu)
    _check(what + " mean", mean, m64, m32)
    _check(what + " rstd", rstd, r64, r32)
    _check(what + " y", y, y64, y32)
    y = y.cpu()
    for r in c.L.unused_ghost_rows:
        assert (y[r] == 0).all(), "%s: unused ghost row %d" % (what, r)


def run_bwd(c, mean, rstd, relu=True, bn=True, dxs=True, dxs2=False, ro=True, ldv=None, lddxs=None, lddu=None, ldo=None):
    """tsgnn_slot_post_bwd_f32 -> du on the CPU"""
    L, F = c.L, c.F
    v = dev(c.v32, ldv)
    d1 = dev(c.dxs, lddxs) if dxs else None
    d2 = dev(c.dxs2, lddxs) if dxs2 else None
    dout = dev(c.dout, ldo) if ro else None
    arg = c.arg.cuda() if ro else None
    du = nan_buf(L.rows, lddu or F)
    _nat().call("slot_post_bwd_f32", *c.dev_struct(), v, v.stride(0), d1, d1.stride(0) if dxs else 0, d2, d2.stride(0) if dxs2 else 0,
                dout, dout.stride(0) if ro else 0, arg, F, int(relu), int(bn), mean if bn else None, rstd if bn else None,
                c.rinv32.cuda(), du, du.stride(0))
    assert _untouched(du, F)
    return du[:, :F]


def check_bwd(what, c, du, **flags):
    d64, d32 = c.bwd_ref(**flags)
    if c.clamped_rows:
        _check_rows(what + " du", du, d64, d32, c.clamped_rows)
    else:
        _check(what + " du", du, d64, d32)
    du = du.cpu()
    for r in c.L.unused_ghost_rows + c.L.pad_rows:
        assert (du[r] == 0).all(), "%s: row %d must be zero" % (what, r)


# ----------------------------------------------------------------------------- (a) slot_bn_fwd
@pytest.mark.parametrize("ghosts", [True, False], ids=["ghost", "noghost"])
@pytest.mark.parametrize("F", GRID_F)
@pytest.mark.parametrize("B", GRID_B)
def test_slot_bn_fwd_grid(B, F, ghosts):
    for profile in ("ragged", "full"):
        c = case(B, F, ghosts, profile)
        for relu in (True, False):
            check_fwd("fwd B%d F%d %s %s relu%d" % (B, F, "ghost" if ghosts else "noghost", profile, relu), c, relu, *run_fwd(c, relu))
            assert _nat().last_kernel() == _table_cell("slot_bn_fwd", B, F)


@pytest.mark.parametrize("B,F", [(16, 64), (40, 36), (128, 128)])
def test_slot_bn_fwd_zero_ptr_and_strides(B, F):
    """the side clear of the readout buffer (zero_n = nmax * BT + 77 words: more than one pass of the grid-stride loop, ragged end)
    and row strides ldv, ldy > F"""
    c = case(B, F, True)
    bt = _bt(B)
    words = torch.full((NMAX * bt + 77 + 8,), 0x5A5A5A5A5A5A, dtype=torch.int64, device="cuda")
    mean, rstd, y = run_fwd(c, True, ldv=F + 4, ldy=F + 8, zero=words[:-8])
    check_fwd("fwd zero_ptr B%d F%d" % (B, F), c, True, mean, rstd, y)
    assert (words[:-8] == 0).all().item() and (words[-8:] == 0x5A5A5A5A5A5A).all().item()


# ----------------------------------------------------------------------------- (b) slot_post_bwd
@pytest.mark.parametrize("ghosts", [True, False], ids=["ghost", "noghost"])
@pytest.mark.parametrize("F", GRID_F)
@pytest.mark.parametrize("B", GRID_B)
def test_slot_post_bwd_grid(B, F, ghosts):
    """relu = bn = 1 with dxs, dout and arg at every cell, mean / rstd from the forward kernel"""
    for profile in ("ragged", "full"):
        c = case(B, F, ghosts, profile)
        mean, rstd, _ = run_fwd(c, True)
        check_bwd("bwd B%d F%d %s %s" % (B, F, "ghost" if ghosts else "noghost", profile), c, run_bwd(c, mean, rstd))
        if F == 128 and B <= 64:                                       # the special case of the backward's dispatch
            assert _nat().last_kernel() == "slot_post_bwd<16,2,%d>" % (512 if B <= 32 else 1024)
        else:
            assert _nat().last_kernel() == _table_cell("slot_post_bwd", B, F)


VARIANTS = {
    "relu0_bn0": dict(relu=False, bn=False),
    "relu1_bn0": dict(relu=True, bn=False),
    "relu0_bn1": dict(relu=False, bn=True),
    "no_dxs": dict(dxs=False),
    "dxs_and_dxs2": dict(dxs2=True),
    "dxs2_only": dict(dxs=False, dxs2=True),
    "no_readout": dict(ro=False),
}


@pytest.mark.parametrize("variant", list(VARIANTS) + ["wide_ld"])
@pytest.mark.parametrize("ghosts", [True, False], ids=["ghost", "noghost"])
@pytest.mark.parametrize("F", [36, 128])
@pytest.mark.parametrize("B", [5, 40, 100])
def test_slot_post_bwd_variants(B, F, ghosts, variant):
    c = case(B, F, ghosts)
    what = "bwd %s B%d F%d %s" % (variant, B, F, "ghost" if ghosts else "noghost")
    if variant == "wide_ld":
        mean, rstd, _ = run_fwd(c, True)
        check_bwd(what, c, run_bwd(c, mean, rstd, ldv=F + 4, lddxs=F + 8, lddu=F + 12, ldo=F + 4))
        return
    flags = VARIANTS[variant]
    mean, rstd, _ = run_fwd(c, flags.get("relu", True))
    check_bwd(what, c, run_bwd(c, mean, rstd, **flags), **flags)


@pytest.mark.parametrize("ghosts", [True, False], ids=["ghost", "noghost"])
@pytest.mark.parametrize("B,F", [(5, 36), (40, 128), (100, 64)])
def test_slot_post_bwd_clamped_norm(B, F, ghosts):
    """rows with rinv = 1e12: du = rinv * dv without the projection.  Two all-zero rows (one real, one the ghost row every graph
    shares) and two rows of norm 0.5e-12, whose v = u / 1e-12 is not zero — only there does the projection differ from none."""
    c = case(B, F, ghosts, clamp=True)
    for flags in (dict(), dict(relu=False)):
        mean, rstd, _ = run_fwd(c, flags.get("relu", True))
        check_bwd("bwd clamped B%d F%d %s %s" % (B, F, "ghost" if ghosts else "noghost", flags), c, run_bwd(c, mean, rstd, **flags), **flags)


@pytest.mark.parametrize("ghosts", [True, False], ids=["ghost", "noghost"])
@pytest.mark.parametrize("B,F", [(5, 36), (40, 128), (100, 100)])
def test_slot_post_bwd_capacity_padded(B, F, ghosts):
    """n_real = graph_ptr[B] + 37: the padding rows hold random v, belong to no graph, and their du is zeroed by the launch"""
    c = case(B, F, ghosts, pad=37)
    assert len(c.L.pad_rows) == 37
    mean, rstd, y = run_fwd(c, True)
    (m64, r64, y64), (m32, r32, y32) = c.fwd_ref(True)
    _check("fwd padded mean", mean, m64, m32)
    _check("fwd padded rstd", rstd, r64, r32)
    # the forward does not write the padding rows (nobody's candidate); every other row is addressed past them correctly
    y = y.cpu()
    assert torch.isnan(y[c.L.pad_rows]).all().item()
    keep = torch.ones(c.L.rows, dtype=torch.bool)
    keep[c.L.pad_rows] = False
    _check("fwd padded y", y[keep], y64[keep], y32[keep])
    for r in c.L.unused_ghost_rows:
        assert (y[r] == 0).all()
    check_bwd("bwd padded B%d F%d" % (B, F), c, run_bwd(c, mean, rstd))


# ----------------------------------------------------------------------------- (c) pair launches
@pytest.mark.parametrize("ghosts", [True, False], ids=["ghost", "noghost"])
@pytest.mark.parametrize("B,F", [(16, 64), (12, 36), (40, 128)])
def test_pair_launches(B, F, ghosts):
    """grid.y = 2: each half is bit-identical to the single launch on the same operands, and right against fp64"""
    nat = _nat()
    c0, c1 = case(B, F, ghosts, seed=0), case(B, F, ghosts, seed=1)
    L = c0.L
    v0, v1 = dev(c0.v32), dev(c1.v32)
    m0, m1, r0, r1 = (nan_buf(NMAX) for _ in range(4))
    y0, y1 = nan_buf(L.rows, F), nan_buf(L.rows, F)
    nat.call("slot_bn_fwd_pair_f32", *c0.dev_struct(), v0, v1, F, F, 1, m0, m1, r0, r1, y0, y1, F)
    for c, m, r, y in ((c0, m0, r0, y0), (c1, m1, r1, y1)):
        ms, rs, ys = run_fwd(c, True)
        assert torch.equal(ms, m) and torch.equal(rs, r) and torch.equal(ys, y)
        check_fwd("pair fwd B%d F%d" % (B, F), c, True, m, r, y)
    for use_dxs, use_dxs2 in ((True, False), (True, True), (False, True), (False, False)):
        d0, d1 = (dev(c.dxs) if use_dxs else None for c in (c0, c1))
        e0, e1 = (dev(c.dxs2) if use_dxs2 else None for c in (c0, c1))
        du0, du1 = nan_buf(L.rows, F), nan_buf(L.rows, F)
        nat.call("slot_post_bwd_pair_f32", *c0.dev_struct(), v0, v1, F, d0, d1, F if use_dxs else 0, e0, e1, F if use_dxs2 else 0, F, 1, 1,
                 m0, m1, r0, r1, c0.rinv32.cuda(), c1.rinv32.cuda(), du0, du1, F)
        if F == 128:                                                   # the paired launch takes the single launch's instantiation
            assert nat.last_kernel() == "slot_post_bwd<16,2,1024>"
        for c, m, r, du in ((c0, m0, r0, du0), (c1, m1, r1, du1)):
            flags = dict(dxs=use_dxs, dxs2=use_dxs2, ro=False)
            single = run_bwd(c, m, r, **flags)
            check_bwd("pair bwd B%d F%d dxs%d dxs2%d" % (B, F, use_dxs, use_dxs2), c, du, **flags)
            assert torch.equal(single, du), "pair half differs from the single launch by %g" % (single - du).abs().max().item()


# ----------------------------------------------------------------------------- (d) slot_post_wgrad
def _wgrad_call(c, mean, rstd, z, K_in, ws, nblocks, dxs=True, ro=True, F=None):
    nat = _nat()
    F = F or c.F
    v = dev(c.v32)
    d1 = dev(c.dxs) if dxs else None
    dout = dev(c.dout) if ro else None
    arg = c.arg.cuda() if ro else None
    L = nat.lib()
    rc = L.tsgnn_slot_post_wgrad_f32(*[nat._arg(a) for a in (
        *c.dev_struct(), v, v.stride(0), d1, F if dxs else 0, dout, F if ro else 0, arg, F, 1, 1, mean, rstd, c.rinv32.cuda(), z,
        z.stride(0), K_in, ws, nblocks)], nat.stream_handle())
    torch.cuda.synchronize()
    return rc


def _z_of(c, K_in):
    """z [rows, ldz], ldz = roundup4(K_in) + 4: NaN in the padding columns and in the ghost rows (a ghost row aggregates nothing)"""
    ldz = (K_in + 3) // 4 * 4 + 4
    z = torch.randn(c.L.rows, K_in, generator=torch.Generator().manual_seed(K_in))
    z[c.L.n_real:] = NAN
    return z, dev(z, ldz)


@pytest.mark.parametrize("K_in", [1, 3, 32, 33, 64, 89, 97, 128])
@pytest.mark.parametrize("B", [1, 8, 32])
def test_slot_post_wgrad(B, K_in):
    """layer 0's dU and its weight / bias gradient slabs in one launch: the slabs summed in fp64 are Z^T dU over the real rows and, in
    row K_in, the column sums of dU over real AND ghost rows; every word of every slab is written, nothing behind them"""
    F = 128
    c = case(B, F, True)
    L = c.L
    mean, rstd, _ = run_fwd(c, True)
    z, zd = _z_of(c, K_in)
    z64 = torch.nan_to_num(z.double(), nan=0.0)
    for dxs, ro in ((True, True), (False, True), (True, False), (False, False)):
        d64, d32 = c.bwd_ref(dxs=dxs, ro=ro)
        ref64 = S.wgrad_slab_sum(z64, d64, L.n_real, K_in)
        cpu32 = S.wgrad_slab_sum(z64.float(), d32, L.n_real, K_in)
        for nblocks in (1, 6, 11):
            n = nblocks * (K_in + 1) * F
            ws = nan_buf(n + 256)
            assert _wgrad_call(c, mean, rstd, zd, K_in, ws, nblocks, dxs=dxs, ro=ro) == 0
            assert torch.isnan(ws[n:]).all().item(), "wrote behind the slabs"
            slabs = ws[:n].cpu()
            assert not torch.isnan(slabs).any().item(), "%d slab words were never written" % int(torch.isnan(slabs).sum())
            got = slabs.double().reshape(nblocks, K_in + 1, F).sum(0)
            what = "wgrad B%d K%d nblocks%d dxs%d ro%d" % (B, K_in, nblocks, dxs, ro)
            _check(what + " dW", got[:K_in], ref64[:K_in], cpu32[:K_in])
            _check(what + " db", got[K_in:], ref64[K_in:], cpu32[K_in:])


@pytest.mark.parametrize("why", ["B33", "F64", "noghost", "nblocks"])
def test_slot_post_wgrad_unsupported(why):
    """TSGNN_EUNSUPPORTED is decided before anything is launched: the slabs stay untouched"""
    B, F, ghosts, nblocks = (33 if why == "B33" else 8), (64 if why == "F64" else 128), why != "noghost", (NMAX + 1 if why == "nblocks" else 4)
    c = case(B, F, ghosts)
    mean, rstd, _ = run_fwd(c, True)
    z, zd = _z_of(c, 32)
    ws = nan_buf(12 * 33 * 128)
    assert _wgrad_call(c, mean, rstd, zd, 32, ws, nblocks) == EUNSUPPORTED
    assert torch.isnan(ws).all().item()


# ----------------------------------------------------------------------------- (e) readout_l2_bwd
@pytest.mark.parametrize("ghost_rows", ["none", "max_size+1", "nmax"])
@pytest.mark.parametrize("F", [4, 20, 64, 128])
@pytest.mark.parametrize("B", [1, 5, 40])
def test_readout_l2_bwd(B, F, ghost_rows):
    """The last layer's dU from the max-readout gradient alone.  PRECONDITION of the kernel: a ghost winner of graph b is always row
    n_real + sizes[b] — the last layer has no slot batch-norm, so all ghost rows share one value and the smallest row id among them
    wins; ghost row n_real + n therefore collects exactly the graphs of size n, in graph order.  arg is drawn accordingly.
    Rows [n_real + n_ghost_rows, ...) are not part of the launch and stay untouched; padding rows (row_graph >= B) get 0."""
    sizes = sizes_of("ragged", B)
    pad = 5
    L = S.Layout(sizes, NMAX, NMAX, n_real=sum(sizes) + pad)
    ngr = {"none": 0, "max_size+1": max(sizes) + 1, "nmax": NMAX}[ghost_rows]
    gen = torch.Generator().manual_seed(B * 1000 + F * 3 + ngr)
    u = torch.randn(L.rows, F, dtype=torch.float64, generator=gen)
    clamped = 1                                                        # a real row of graph 0 with norm 0.5e-12
    u[clamped] = u[clamped].abs() * (0.5e-12 / u[clamped].norm())
    nrm = u.norm(dim=1, keepdim=True).clamp(min=1e-12)
    v32, rinv32 = (u / nrm).float(), (1.0 / nrm[:, 0]).float()
    dout = torch.randn(B, F, generator=gen)
    sz = torch.as_tensor(np.asarray(sizes))
    gp = torch.as_tensor(L.graph_ptr[:-1])
    arg = (gp[:, None] + (torch.rand(B, F, generator=gen) * sz[:, None]).long().clamp(max=NMAX - 1)).long()
    ghost_ok = (sz < ngr)[:, None]
    pick = torch.rand(B, F, generator=gen)
    arg = torch.where((pick < 0.3) & ghost_ok, (L.n_real + sz)[:, None].expand(B, F), arg)
    arg = torch.where(pick > 0.9, torch.full_like(arg, -1), arg)
    arg[0, 1] = clamped
    if B >= 5 and ngr > 4:                                             # graphs 2 and 3 both have 4 nodes and both win ghost row n_real + 4
        assert sizes[2] == sizes[3] == 4
        arg[2, 0] = arg[3, 0] = L.n_real + 4
    arg = arg.to(torch.int32)
    rg = L.row_graph()
    rg[-2:] = B + 7                                                    # any value >= B marks a padding row
    d64 = S.readout_l2_bwd(v32.double(), rinv32.double(), dout, arg, rg, ngr)
    d32 = S.readout_l2_bwd(v32.double(), rinv32.double(), dout, arg, rg, ngr, dtype=torch.float32)
    ldv, ldo, lddu = F + 4, F + 8, F + 12
    vd, doutd, du = dev(v32, ldv), dev(dout, ldo), nan_buf(L.rows, lddu)
    _nat().call("readout_l2_bwd_f32", c_ptr(L.graph_ptr), torch.from_numpy(rg).cuda(), B, L.n_real, ngr, vd, ldv, doutd, ldo, arg.cuda(), F,
                rinv32.cuda(), du, lddu)
    rows = L.n_real + ngr
    assert torch.isnan(du[rows:]).all().item() and _untouched(du, F)
    _check_rows("readout_l2_bwd B%d F%d ghost rows %d" % (B, F, ngr), du[:rows, :F], d64, d32, [clamped])
    du = du.cpu()
    for r in L.pad_rows:
        assert (du[r, :F] == 0).all()


def c_ptr(a):
    return torch.as_tensor(np.asarray(a, dtype=np.int32)).cuda()


# ----------------------------------------------------------------------------- (f) readout forward
def _readout_sizes(B, nmax, ghosts, kind):
    if B == 1:
        return [nmax if (kind == "allneg" or not ghosts) else max(1, nmax - 2)]
    s = [max(1, min(nmax, k)) for k in (nmax, 1, nmax // 2, nmax - 1, 3, 64, 65)]
    if not ghosts:
        s[4] = 0                                                       # a graph without any candidate: out 0, arg -1
    return s


def _readout_input(kind, L, F, seed):
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn(L.rows, F, generator=gen)
    if kind == "allneg":
        x = -x.abs() - 0.125
    gp, sz = L.graph_ptr, L.sizes
    if kind == "ties":
        for b in range(L.B):
            r0 = int(gp[b])
            if sz[b] >= 2:
                x[r0, 0] = x[r0 + 1, 0] = 50.0                         # among real rows the smallest row wins
            if sz[b] >= 3:
                x[r0 + 2, 1] = x[r0 + 1, 1] = 50.0
            if L.n_ghost and 1 <= sz[b] < L.nmax:
                x[r0 + int(sz[b]) - 1, 2] = x[L.n_real + int(sz[b]), 2] = 60.0   # a real row beats a ghost row of the same value
    if kind == "ghostmax":
        x[L.n_real + L.nmax - 1] = 100.0
        if L.nmax > 2:
            x[L.n_real + 1, 3] = 200.0
    assert not ((x == 0) & torch.signbit(x)).any()
    return x


@pytest.mark.parametrize("kind,ghosts", [("random", True), ("random", False), ("allneg", False), ("ties", True), ("ties", False),
                                         ("ghostmax", True)])
@pytest.mark.parametrize("nmax", [5, 64, 65, 130])
@pytest.mark.parametrize("B", [1, 7])
def test_readout_partial_decode(B, nmax, kind, ghosts):
    """readout_partial per layer on a zeroed packed buffer, then ONE readout_decode_layers for L = 3 layers (Fh = 36, Fl = 20):
    out and arg are exactly slot_ref.readout_max's, and message_passing.readout_fwd_raw gives the same on the same rows"""
    from two_stage_gnn_amd import message_passing as mp
    from two_stage_gnn_amd.graph import GraphBatch
    nat = _nat()
    Lyr, Fh, Fl = 3, 36, 20
    sizes = _readout_sizes(B, nmax, ghosts, kind)
    L = S.Layout(sizes, nmax, nmax if ghosts else 0)
    g = GraphBatch.structure_only(sizes, nmax, "cuda", ghosts=ghosts)
    widths = [Fh] * (Lyr - 1) + [Fl]
    xs = [_readout_input(kind, L, w, 100 * l + nmax + B) for l, w in enumerate(widths)]
    P = (Lyr - 1) * Fh + Fl
    packed = torch.zeros(B * P, dtype=torch.int64, device="cuda")
    off = 0
    for x, w in zip(xs, widths):
        xd = dev(x, w + 4)
        nat.call("readout_partial_f32", g.graph_ptr, B, nmax, L.n_real, L.n_ghost, xd, xd.stride(0), w, packed[off:])
        off += B * w
    out = nan_buf(B, P + 4)
    arg = torch.full((B * P,), -7, dtype=torch.int32, device="cuda")
    nat.call("readout_decode_layers_f32", packed, B, Lyr, Fh, Fl, out, out.stride(0), arg)
    assert _untouched(out, P)
    out, arg = out.cpu(), arg.cpu()
    off = 0
    for l, (x, w) in enumerate(zip(xs, widths)):
        o_ref, a_ref = S.readout_max(x, L)
        assert torch.equal(out[:, l * Fh:l * Fh + w], o_ref), "layer %d out" % l
        assert torch.equal(arg[off:off + B * w].reshape(B, w), a_ref), "layer %d arg" % l
        off += B * w
        o2, a2 = mp.readout_fwd_raw(x.cuda(), g)
        assert torch.equal(o2.cpu(), o_ref) and torch.equal(a2.cpu(), a_ref), "readout_fwd_raw layer %d" % l
        if kind == "ghostmax":
            assert (a_ref >= L.n_real).any()
        if kind == "ties" and ghosts and B > 1:
            assert int(a_ref[1, 2]) == int(L.graph_ptr[1])              # graph 1 (one node): its real row, not ghost row n_real + 1


# ----------------------------------------------------------------------------- (g) unfused fallback
@pytest.mark.parametrize("relu,bn", [(True, True), (False, True), (True, False)])
@pytest.mark.parametrize("ghosts", [True, False], ids=["ghost", "noghost"])
@pytest.mark.parametrize("B,F", [(3, 7), (130, 32), (5, 200), (129, 130), (32, 128)])
def test_bn_slots_unfused(B, F, ghosts, relu, bn):
    """message_passing.bn_slots (csrc/bn_readout.hip: what runs at the shapes the fused kernels refuse), forward and backward through
    autograd.  It normalises an unused ghost row like any row of its slot (the fused kernel writes 0 there; nobody reads it): that
    row is compared with (act(v) - mean) * rstd, and carries no gradient.  At (32, 128) the fused kernels run too and agree."""
    from two_stage_gnn_amd import message_passing as mp
    fused = bool(_nat().lib().tsgnn_slot_fused_supported(B, F))
    assert fused == ((B, F) == (32, 128))
    c = case(B, F, ghosts)
    L = c.L
    v = c.v32.cuda().requires_grad_(True)
    y = mp.bn_slots(v, c.g, relu=relu, bn=bn)
    dy = torch.randn(L.rows, F, generator=torch.Generator().manual_seed(B + F))
    dy[L.unused_ghost_rows] = 0.0
    y.backward(dy.cuda())
    refs = []
    for dt in (torch.float64, torch.float32):
        m, r, yr = S.slot_bn(c.v64, L, relu=relu, bn=bn, dtype=dt)
        for row in L.unused_ghost_rows:
            h = c.v64[row].to(dt)
            h = torch.relu(h) if relu else h
            yr[row] = (h - m[row - L.n_real]) * r[row - L.n_real] if bn else h
        refs.append((yr, S.slot_bn_bwd(c.v64, L, dy, relu=relu, bn=bn, dtype=dt)))
    what = "unfused B%d F%d %s relu%d bn%d" % (B, F, "ghost" if ghosts else "noghost", relu, bn)
    _check(what + " y", y, refs[0][0], refs[1][0])
    _check(what + " dv", v.grad, refs[0][1], refs[1][1])
    if fused and relu and bn:
        # the fused backward with rinv = 2**40 on every row (at or above the clamp mark: no projection): du = 2**40 * dv exactly
        mean, rstd, yf = run_fwd(c, True)
        check_fwd(what + " fused", c, True, mean, rstd, yf)
        # only real rows carry a gradient here: a ghost row's reaches the fused kernel through dout / arg alone
        dy_real = dy.clone()
        dy_real[L.n_real:] = 0.0
        v2 = c.v32.cuda().requires_grad_(True)
        mp.bn_slots(v2, c.g, relu=True, bn=True).backward(dy_real.cuda())
        dy_in = dy_real.clone()
        dy_in[L.n_real:] = NAN                                         # the fused kernel must not read dxs on ghost rows
        du = nan_buf(L.rows, F)
        _nat().call("slot_post_bwd_f32", *c.dev_struct(), c.v32.cuda(), F, dy_in.cuda(), F, None, 0, None, 0, None, F, 1, 1, mean, rstd,
                    torch.full((L.rows,), 2.0 ** 40, device="cuda"), du, F)
        ref64 = S.slot_bn_bwd(c.v64, L, dy_real, dtype=torch.float64)
        ref32 = S.slot_bn_bwd(c.v64, L, dy_real, dtype=torch.float32)
        dv_fused = (du * 2.0 ** -40).cpu()
        dv_unfused = v2.grad.detach().cpu()
        _check(what + " fused dv", dv_fused, ref64, ref32)
        _check(what + " unfused dv (real-row dy)", dv_unfused, ref64, ref32)
        yard = max((ref32.double() - ref64).abs().max().item(), EPS32 * ref64.abs().max().item())
        diff = (dv_fused.double() - dv_unfused.double()).abs().max().item()
        print("%s: max|fused dv - unfused dv| / yardstick = %.3f" % (what, diff / yard))
        assert diff <= K_DEFAULT * yard
