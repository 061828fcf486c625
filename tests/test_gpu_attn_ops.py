"""The composed (per-op) GAT attention kernels (csrc/attention.hip) one by one through the C ABI against tests/attn_ops_ref.py in float64:
node_scores / node_scores2, edge_softmax_fwd / _bwd, edge_permute, csr_row_sum / _perm, csr_spmm_heads / _epi, csr_sddmm_heads,
segment_wsum / wsum2, gather_wsum, broadcast_add, elu_heads_fwd / _bwd, pack_heads / unpack_heads — the path the fused GAT kernels
decline to, and "the module" of the GAT triplet and stream tests.  tests/test_attn_ops_ref_host.py ties the reference to the oracles
and checks the inputs' guarantees (every LeakyReLU argument >= 1e-3 away from 0, every ELU argument too, except exact zeros put there on
purpose, whose two branches agree).

Every output sits in a guard_buf.Out prefilled with one NaN pattern, with a leading dimension wider than the row wherever the entry
point takes one and spare rows behind the last where it takes none: what a kernel must write is compared, what it must not touch
(pad columns, alpha / dt of no entry, the guard words) must still be that pattern.  Every input's pad columns are NaN on the device:
nothing may read them.  Every cell is launched twice into fresh buffers and the two results are compared bit for bit, and every
cell asserts the kernel ``nat.last_kernel()`` names.  Copies (edge_permute, pack_heads, unpack_heads) are compared bit for bit.

Tolerance (fp32_yardstick.py), for every float output on its own:

    max|hip - ref64|  <=  K * max( max|cpu32 - ref64| , 2**-23 * max|ref64| ),   K = 8

Every test prints its ratios  max|hip - ref64| / yardstick  before asserting.  The largest ratio per kernel measured on the MI355X:

    node_scores / node_scores2      s 1.50 (H1 Fh128 rows1, the scalar kernel's 64-stride loop)
    edge_softmax_fwd                alpha 0.97 (rows of A, H4)
    edge_softmax_bwd                dt 1.42 (rows of A, H4)           ds_grp 1.26 (rows of A, H1)
    csr_row_sum / _perm             0.94 (H3) / 0.58 (H4)
    csr_spmm_heads / _epi           vec4 1.28 (H4 Fh32, every epilogue term, row_seg)      scalar 1.70 (H2 Fh6, u + row_seg + eperm)
    csr_sddmm_heads                 0.90 (H1 Fh64)
    segment_wsum / wsum2            0.55 (six segments, w null) / 0.32 (out2);  mean 0.30
    gather_wsum                     0.42 (C264)
    broadcast_add                   0.51 (mode 1 with w)
    elu_heads_fwd / _bwd            0.51 (mean over 3 heads) / 0.27 (vec4)
    the autograd node               y 1.33 (edges ghost1, uniform term, mean)      dh 1.48 (edges padded, per target + drop_mult)
                                    da_row 1.54 (edges padded, by column, mean)    da_col 1.71 (blocks31 padded, uniform term)

No output comes near K = 8, the cell with scores of magnitude 60 included, so there is no second yardstick and no table of exceptions.

The last tests run the autograd node (attention_aggregate + elu_heads) against float64 autograd of the composed reference, and the
whole encoder on graphs without any edge (nnz = 0: the one-word placeholders of the transpose are zero, never an index) on both GAT
paths against oracle/dense_ref.gat_encoder.
"""
import numpy as np
import pytest
import torch

import attn_ops_ref as A
import gat_attn_ref as G
from fp32_yardstick import K_DEFAULT, _check
from guard_buf import Out

pytestmark = pytest.mark.gpu

NAN = float("nan")
K = K_DEFAULT
EINVAL = -1


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
    nat = _nat()
    return getattr(nat.lib(), "tsgnn_" + name)(*[nat._arg(a) for a in args], nat.stream_handle())


# ----------------------------------------------------------------------------- device buffers
def dmat(t, ld=None, off=0):
    """[rows, ld] float32 view on the device holding t in its first columns, NaN in the pad columns; off: floats the base pointer is
    moved off its 16-byte alignment"""
    rows, W = t.shape
    ld = ld or W
    buf = torch.full((rows * ld + off + 4,), NAN, dtype=torch.float32)
    buf[off:off + rows * ld].view(rows, ld)[:, :W] = t
    d = buf.cuda()
    v = d[off:off + rows * ld].view(rows, ld)
    assert v.data_ptr() % 16 == (4 * off) % 16
    return v


def dint(t):
    return t.to(torch.int32).contiguous().cuda()


def owned(out, rows, cols):
    m = torch.zeros(out.rows, out.ld, dtype=torch.bool)
    m[:rows, :cols] = True
    return m


def twice(kernel, fn):
    """fn() -> the guard_buf.Out buffers one launch into fresh buffers wrote; launched twice, compared bit for bit"""
    a = fn()
    assert _nat().last_kernel() == kernel, (_nat().last_kernel(), kernel)
    b = fn()
    torch.cuda.synchronize()
    for x, y in zip(a, b):
        assert torch.equal(x.bits, y.bits), "%s: two launches differ" % kernel
    print("kernel: %s" % kernel)
    return a


def check(what, out, ref64, cpu32, mask=None):
    """the [rows, cols] block of ``out`` against the reference; everything else of the buffer untouched.  mask (bool, ref's shape):
    the elements the launch owns inside the block (default all)"""
    rows, cols = ref64.shape
    hip = out.mat[:rows, :cols].cpu()
    own = owned(out, rows, cols)
    if mask is not None:
        own[:rows, :cols] = mask
        assert bool(torch.isnan(hip[~mask]).all()), "%s: elements of no entry were written" % what
        hip, ref64, cpu32 = hip[mask].view(1, -1), ref64[mask].view(1, -1), cpu32[mask].view(1, -1)
    r = _check(what, hip, ref64, cpu32, K) if ref64.numel() else 0.0
    out.rest_untouched(what, own)
    return r


def exact(what, out, ref):
    rows, cols = ref.shape
    hip = out.mat[:rows, :cols].cpu()
    assert torch.equal(hip.view(torch.int32), ref.float().view(torch.int32)), "%s: not a bit-exact copy" % what
    out.rest_untouched(what, owned(out, rows, cols))


def both(fn, *ts):
    """(fn in float64, fn in float32) of float32 inputs"""
    return fn(*[t.double() if t is not None else None for t in ts]), fn(*ts)


# ----------------------------------------------------------------------------- node_scores / node_scores2
NS_ROWS = (1, 3, 4, 5, 9)
NS_VEC = [(1, 4), (3, 4), (3, 8), (3, 16), (3, 32), (3, 64), (4, 64), (8, 32), (16, 16)]
NS_SCALAR = [(2, 6, ""), (2, 12, ""), (2, 20, ""), (1, 128, ""), (8, 64, ""), (3, 8, "ldx"), (3, 8, "lda"), (3, 8, "base")]
NS_CELLS = [(H, Fh, "", NS_ROWS[k % 5]) for k, (H, Fh) in enumerate(NS_VEC)] + [c + (NS_ROWS[(k + 2) % 5],) for k, c in enumerate(NS_SCALAR)]


@pytest.mark.parametrize("H,Fh,why,rows", NS_CELLS)
def test_node_scores(H, Fh, why, rows):
    nat = _nat()
    C = H * Fh
    vec = not why and Fh in (4, 8, 16, 32, 64) and H * (Fh // 4) <= 64
    kernel = "node_scores_vec4_kernel<%d>" % (Fh // 4) if vec else "node_scores_kernel"
    ldx = C + 1 if why == "ldx" else C + 4
    lda = Fh + 1 if why == "lda" else Fh + 4
    x, a1, a2 = A.rnd(100 + C, rows, C), A.rnd(200 + C, H, Fh), A.rnd(300 + C, H, Fh)
    xd, a1d, a2d = dmat(x, ldx, off=1 if why == "base" else 0), dmat(a1, lda), dmat(a2, lda)
    what = "node_scores H%d Fh%d rows%d %s" % (H, Fh, rows, why)

    def one():
        s = Out(rows + 2, H)
        nat.call("node_scores_f32", xd, ldx, rows, H, Fh, a1d, lda, s.mat)
        return (s,)

    def two():
        s1, s2 = Out(rows + 2, H), Out(rows + 2, H)
        nat.call("node_scores2_f32", xd, ldx, rows, H, Fh, a1d, lda, s1.mat, a2d, lda, s2.mat)
        return s1, s2
    r1 = both(lambda x_, a_: A.node_scores(x_, a_, H, Fh), x, a1)
    r2 = both(lambda x_, a_: A.node_scores(x_, a_, H, Fh), x, a2)
    (s,) = twice(kernel, one)
    check(what + " s", s, *r1)
    s1, s2 = twice(kernel, two)
    check(what + " s1", s1, *r1)
    check(what + " s2", s2, *r2)


# ----------------------------------------------------------------------------- edge softmax, row sums
@pytest.mark.parametrize("cell", A.SOFTMAX_CELLS, ids=lambda c: "%s-H%d%s-slope%g%s" % (c[0], c[1], "-mod" if c[2] else "", c[3], "-x60" if c[4] else ""))
def test_edge_softmax_and_row_sums(cell):
    nat = _nat()
    rowptr, col, rows, mod, s_grp, s_oth = A.softmax_inputs(cell)
    H, slope = cell[1], cell[3]
    nnz = int(rowptr[-1])
    assert rowptr.numel() == rows + 1 and col.numel() == nnz and int(col.max()) < (2 * mod if mod else s_oth.size(0)) and s_grp.size(0) == (mod or rows)
    rp, cl, sg, so = dint(rowptr), dint(col), s_grp.cuda(), s_oth.cuda()
    what = "softmax %s" % (cell,)
    deg = (rowptr[1:] - rowptr[:-1]).long()

    def fwd():
        alpha = Out(nnz + 3, H)
        nat.call("edge_softmax_fwd_f32", rp, cl, rows, H, sg, so, mod, slope, alpha.mat)
        return (alpha,)
    a64, a32 = both(lambda g_, o_: A.edge_softmax_fwd(rowptr, col, mod, g_, o_, slope), s_grp, s_oth)
    (alpha,) = twice("edge_softmax_fwd_kernel", fwd)
    check(what + " alpha", alpha, a64, a32)
    sums = A.csr_row_sum(rowptr, alpha.mat[:nnz].cpu().double())
    assert ((sums - (deg > 0).double().unsqueeze(1)).abs() < 1e-5).all()                  # every group's coefficients add up to 1

    dalpha = A.rnd(500 + H, nnz, H)
    al_d, dal_d = a32.cuda(), dalpha.cuda()

    def bwd():
        dt, ds = Out(nnz + 3, H), Out(rows + 2, H)
        nat.call("edge_softmax_bwd_f32", rp, cl, rows, H, sg, so, mod, slope, al_d, dal_d, dt.mat, ds.mat)
        return dt, ds
    b64 = A.edge_softmax_bwd(rowptr, col, mod, s_grp.double(), s_oth.double(), slope, dalpha.double())
    b32 = A.edge_softmax_bwd(rowptr, col, mod, s_grp, s_oth, slope, dalpha)
    dt, ds = twice("edge_softmax_bwd_kernel", bwd)
    check(what + " dt", dt, b64[0], b32[0])
    check(what + " ds_grp", ds, b64[1], b32[1])
    assert not ds.mat[:rows].cpu()[deg == 0].any()                                        # ds_grp of an empty row is 0

    val = A.rnd(600 + H, nnz, H)
    perm = torch.randperm(nnz, generator=torch.Generator().manual_seed(H)).to(torch.int32)
    vd, pd = val.cuda(), dint(perm)

    def rsum():
        o = Out(rows + 2, H)
        nat.call("csr_row_sum_f32", rp, vd, rows, H, o.mat)
        return (o,)

    def rsum_perm():
        o = Out(rows + 2, H)
        nat.call("csr_row_sum_perm_f32", rp, vd, pd, rows, H, o.mat)
        return (o,)
    (o,) = twice("csr_row_sum_kernel", rsum)
    check(what + " row_sum", o, *both(lambda v_: A.csr_row_sum(rowptr, v_), val))
    (o,) = twice("csr_row_sum_kernel[eperm]", rsum_perm)
    check(what + " row_sum_perm", o, *both(lambda v_: A.csr_row_sum(rowptr, v_, perm), val))


# ----------------------------------------------------------------------------- edge_permute
@pytest.mark.parametrize("H", [1, 3])
@pytest.mark.parametrize("scatter", [0, 1])
def test_edge_permute(H, scatter):
    nat = _nat()
    n = 301                                                                               # two blocks at H = 1, four at H = 3
    src = A.rnd(700 + H, n, H)
    perm = torch.randperm(n, generator=torch.Generator().manual_seed(7 + H)).to(torch.int32)
    sd, pd = src.cuda(), dint(perm)

    def run():
        dst = Out(n + 3, H)
        nat.call("edge_permute_f32", sd, pd, n, H, scatter, dst.mat)
        return (dst,)
    (dst,) = twice("scatter_rows_small" if scatter else "gather_rows_small", run)
    exact("edge_permute", dst, A.edge_permute(src, perm, bool(scatter)))
    none = Out(4, H)
    assert _rc("edge_permute_f32", sd, pd, 0, H, scatter, none.mat) == 0                  # no entry: nothing is launched
    none.rest_untouched("edge_permute n = 0", owned(none, 0, 0))


# ----------------------------------------------------------------------------- head-weighted aggregation
SPMM_VEC = [(4, 4, 16), (5, 8, 16), (2, 32, 16), (9, 8, 32), (4, 32, 32), (17, 8, 64), (4, 64, 64)]        # F = 16, 40, 64, 72, 128, 136, 256
SPMM_SCALAR = [(2, 6, ""), (65, 4, ""), (4, 8, "ldx")]                                                       # Fh % 4, F = 260, ldx % 4
EPIS = [(), ("w1",), ("w2",), ("u",), ("u", "seg"), ("u", "uw"), ("u", "uscale"), ("eperm",), ("u", "eperm"), ("u", "seg", "eperm"),
        ("w1", "w2"), ("w1", "w2", "u", "uw", "uscale"), ("w1", "w2", "u", "uw", "uscale", "seg")]
FULL = EPIS[-1]
SPMM_CELLS = []
for H_, Fh_, G_ in SPMM_VEC:
    every = (H_, Fh_) in ((5, 8), (9, 8), (4, 64))
    SPMM_CELLS += [("vec", H_, Fh_, "", e, False) for e in (EPIS if every else [None, FULL])]
SPMM_CELLS += [("scalar", 2, 6, "", e, False) for e in EPIS + [None]]
SPMM_CELLS += [("scalar", 65, 4, "", FULL, False), ("scalar", 4, 8, "ldx", FULL, False), ("scalar", 4, 8, "ldx", None, False)]
SPMM_CELLS += [("vec", 5, 8, "", ("u", "eperm"), True), ("scalar", 2, 6, "", FULL, True), ("vec", 4, 64, "", None, True)]     # mod = n
_SPMM_KERNEL = {(H_, Fh_): "spmm_heads_vec4<%d>" % G_ for H_, Fh_, G_ in SPMM_VEC}


@pytest.mark.parametrize("gname,H,Fh,why,epi,tiled", SPMM_CELLS,
                         ids=lambda v: ("+".join(v) or "epi-none") if isinstance(v, tuple) else ("plain" if v is None else str(v)))
def test_csr_spmm_heads(gname, H, Fh, why, epi, tiled):
    """epi None: tsgnn_csr_spmm_heads_f32; a tuple: tsgnn_csr_spmm_heads_epi_f32 with those terms"""
    nat = _nat()
    F_ = H * Fh
    rowptr, col, n = A.graph(gname)
    mod = 0
    if tiled:
        rowptr, col = A.tile(rowptr, col, n, 2)
        mod = n
    rows, nnz = rowptr.numel() - 1, int(rowptr[-1])
    kernel = "spmm_heads_kernel" if gname == "scalar" else _SPMM_KERNEL[(H, Fh)]
    ldx, ldy = (F_ + 1, F_ + 3) if why == "ldx" else (F_ + 4, F_ + 8)
    seed = 1000 + 7 * F_ + len(epi or ())
    gen = torch.Generator().manual_seed(seed)
    x, alpha = A.rnd(seed, n, F_), A.rnd(seed + 1, nnz, H)
    nseg, rps = 5, (rows + 4) // 5
    kw = {}
    e = set(epi or ())
    if "w1" in e:
        kw.update(w1=A.rnd(seed + 2, rows, H), a1=A.rnd(seed + 3, H, Fh))
    if "w2" in e:
        kw.update(w2=A.rnd(seed + 4, rows, H), a2=A.rnd(seed + 5, H, Fh))
    if "u" in e:
        kw.update(u=A.rnd(seed + 6, nseg, F_), rows_per_seg=rps)
        if "seg" in e:
            kw.update(row_seg=torch.sort(torch.randint(0, nseg, (rows,), generator=gen))[0].to(torch.int32), rows_per_seg=0)
        if "uw" in e:
            kw.update(uw=A.rnd(seed + 7, rows, H))
        if "uscale" in e:
            kw.update(uscale=0.25)
    stored = alpha
    if "eperm" in e:
        kw.update(eperm=torch.randperm(nnz, generator=gen).to(torch.int32))
        stored = torch.empty_like(alpha)
        stored[kw["eperm"].long()] = alpha                                                  # entry e's weights live at stored[eperm[e]]
    lda, ldu = Fh + 2, F_ + 3
    assert int(col.max()) < (2 * n if mod else n) and ("u" not in e or "seg" in e or (rows - 1) // rps < nseg)
    rp, cl, xd, ad = dint(rowptr), dint(col), dmat(x, ldx), stored.cuda()
    d = {k: (dint(v) if v.dtype == torch.int32 else (dmat(v, lda) if k in ("a1", "a2") else (dmat(v, ldu) if k == "u" else v.cuda())))
         for k, v in kw.items() if torch.is_tensor(v)}

    def run():
        y = Out(rows, ldy)
        if epi is None:
            nat.call("csr_spmm_heads_f32", rp, cl, ad, H, Fh, xd, ldx, mod, y.mat, ldy, rows)
        else:
            nat.call("csr_spmm_heads_epi_f32", rp, cl, ad, H, Fh, xd, ldx, mod, y.mat, ldy, rows, d.get("w1"), d.get("a1"), lda, d.get("w2"),
                     d.get("a2"), lda, d.get("u"), ldu, d.get("uw"), kw.get("rows_per_seg", 0), d.get("row_seg"), kw.get("uscale", 1.0),
                     d.get("eperm"))
        return (y,)
    ints = {k: v for k, v in kw.items() if not torch.is_tensor(v) or v.dtype == torch.int32}
    flt = [k for k in kw if k not in ints]

    def ref(x_, al_, *fl):
        return A.csr_spmm_heads(rowptr, col, mod, al_, x_, H, Fh, **dict(zip(flt, fl)), **ints)
    (y,) = twice(kernel, run)
    check("spmm %s H%d Fh%d %s %s%s" % (gname, H, Fh, why, epi, " mod" if tiled else ""), y, *both(ref, x, stored, *[kw[k] for k in flt]))


# ----------------------------------------------------------------------------- SDDMM
SDDMM_CELLS = [(F_ // Fh, Fh) for F_ in (16, 40, 64, 72, 128, 136, 256) for Fh in (4, 8, 16, 32, 64) if F_ % Fh == 0]
SDDMM_SCALAR = [(2, 12), (2, 6)]


@pytest.mark.parametrize("H,Fh,tiled", [c + (False,) for c in SDDMM_CELLS + SDDMM_SCALAR] + [(5, 8, True), (2, 6, True), (4, 64, True)])
def test_csr_sddmm_heads(H, Fh, tiled):
    """tiled: two copies of the graph with mod = n, on one cell per kernel"""
    nat = _nat()
    F_ = H * Fh
    rowptr, col, n = A.graph("sddmm")
    mod = 0
    if tiled:
        rowptr, col = A.tile(rowptr, col, n, 2)
        mod = n
    rows, nnz = rowptr.numel() - 1, int(rowptr[-1])
    vec = (H, Fh) in SDDMM_CELLS
    kernel = "sddmm_heads_vec4<%d>" % (16 if F_ <= 64 else (32 if F_ <= 128 else 64)) if vec else "sddmm_heads_kernel"
    lddy, ldx = F_ + 4, F_ + 8
    dy, x = A.rnd(2000 + F_ + Fh, rows, F_), A.rnd(2100 + F_ + Fh, n, F_)
    rp, cl, dyd, xd = dint(rowptr), dint(col), dmat(dy, lddy), dmat(x, ldx)

    def run():
        da = Out(nnz + 3, H)
        nat.call("csr_sddmm_heads_f32", rp, cl, H, Fh, dyd, lddy, xd, ldx, mod, da.mat, rows)
        return (da,)
    (da,) = twice(kernel, run)
    check("sddmm H%d Fh%d%s" % (H, Fh, " mod" if tiled else ""), da, *both(lambda d_, x_: A.csr_sddmm_heads(rowptr, col, mod, d_, x_, H, Fh), dy, x))


# ----------------------------------------------------------------------------- segment sums
SEG_LENGTHS = (0, 1, 127, 128, 129, 300)


@pytest.mark.parametrize("case", ["segments", "one-long"])
@pytest.mark.parametrize("weights", [False, True], ids=["w-null", "w"])
@pytest.mark.parametrize("mean", [0, 1])
def test_segment_wsum(case, weights, mean):
    nat = _nat()
    if case == "segments":
        H, Fh = 9, 8                                                                       # C = 72: two column blocks, the second partly live
        seg_ptr = torch.tensor(np.concatenate([[0], np.cumsum(SEG_LENGTHS)]), dtype=torch.int32)
        nseg, longest = len(SEG_LENGTHS), max(SEG_LENGTHS)
    else:
        H, Fh = 2, 4                                                                       # 2,100 rows = 17 chunks: the final kernel's 16 chunk lanes wrap
        seg_ptr, nseg, longest = None, 1, 2100
    C = H * Fh
    rows = int(seg_ptr[-1]) if seg_ptr is not None else longest
    nchunk = (longest + 127) // 128
    assert case == "segments" or nchunk > 16
    ldx, ldo, scale = C + 4, C + 4, 0.5
    x, w = A.rnd(3000 + C, rows, C), (A.rnd(3100 + C, rows, H) if weights else None)
    w2 = A.rnd(3200 + C, rows, H)
    xd, wd, w2d, sp = dmat(x, ldx), (w.cuda() if weights else None), w2.cuda(), (dint(seg_ptr) if seg_ptr is not None else None)
    what = "segment_wsum %s w=%s mean=%d" % (case, weights, mean)

    def run():
        ws, out = Out(1, nchunk * nseg * C), Out(nseg, ldo)
        nat.call("segment_wsum_f32", xd, ldx, wd, H, Fh, sp, nseg, rows, longest, scale, mean, ws.mat, out.mat, ldo)
        return out, ws
    out, ws = twice("segment_wsum_kernel + segment_wsum_final", run)
    r64, r32 = both(lambda x_, w_: A.segment_wsum(x_, w_, H, Fh, seg_ptr, scale, bool(mean)), x, w)
    check(what, out, r64, r32)
    ws.rest_untouched(what + " workspace", owned(ws, 1, nchunk * nseg * C))
    if seg_ptr is not None:
        assert not out.mat[0, :C].cpu().any()                                              # the empty segment: 0, its mean too
    if weights and not mean:

        def run2():
            ws, o1, o2 = Out(1, 2 * nchunk * nseg * C), Out(nseg, ldo), Out(nseg, ldo)
            nat.call("segment_wsum2_f32", xd, ldx, wd, w2d, H, Fh, sp, nseg, rows, longest, scale, ws.mat, o1.mat, o2.mat, ldo)
            return o1, o2, ws
        o1, o2, ws = twice("segment_wsum_kernel + segment_wsum_final", run2)
        check(what + " wsum2 out1", o1, r64, r32)
        check(what + " wsum2 out2", o2, *both(lambda x_, w_: A.segment_wsum(x_, w_, H, Fh, seg_ptr, scale), x, w2))
        ws.rest_untouched(what + " wsum2 workspace", owned(ws, 1, 2 * nchunk * nseg * C))


@pytest.mark.parametrize("C", [8, 264])
def test_gather_wsum(C):
    nat = _nat()
    seg_ptr = torch.tensor([0, 0, 1, 6], dtype=torch.int32)                                # segments listing 0, 1 and 5 rows
    idx = torch.tensor([17, 3, 19, 0, 3, 11], dtype=torch.int32)
    ldx, ldo, scale = C + 4, C + 4, 0.125
    x, w = A.rnd(4000 + C, 20, C), A.rnd(4100 + C, 6)
    xd, wd, idd, sp = dmat(x, ldx), w.cuda(), dint(idx), dint(seg_ptr)

    def run():
        out = Out(3, ldo)
        nat.call("gather_wsum_f32", xd, ldx, idd, wd, sp, 3, C, scale, out.mat, ldo)
        return (out,)
    (out,) = twice("gather_wsum_kernel", run)
    check("gather_wsum C%d" % C, out, *both(lambda x_, w_: A.gather_wsum(x_, idx, w_, seg_ptr, C, scale), x, w))
    assert not out.mat[0, :C].cpu().any()


@pytest.mark.parametrize("mode", ["a", "u", "u-w-null"])
def test_broadcast_add(mode):
    nat = _nat()
    rows, H, Fh, rps, scale = 87, 2, 3, 20, 0.5                                            # 522 elements: three blocks, the last partly live
    C = H * Fh
    ldy, lda, ldu = C + 3, Fh + 2, C + 2
    y0, w = A.rnd(5000, rows, C), (None if mode == "u-w-null" else A.rnd(5001, rows, H))
    a, u = (A.rnd(5002, H, Fh) if mode == "a" else None), (None if mode == "a" else A.rnd(5003, 5, C))
    y0d, wd = y0.cuda(), (w.cuda() if w is not None else None)
    ad, ud = (dmat(a, lda) if a is not None else None), (dmat(u, ldu) if u is not None else None)

    def run():
        y = Out(rows, ldy)
        y.mat[:, :C] = y0d                                                                 # accumulation onto a non-zero y
        nat.call("broadcast_add_f32", y.mat, ldy, rows, H, Fh, wd, ad, lda, ud, ldu, 0 if mode == "a" else rps, scale)
        return (y,)
    (y,) = twice("broadcast_add_kernel", run)
    check("broadcast_add " + mode, y, *both(lambda y_, w_, a_, u_: A.broadcast_add(y_, w_, H, Fh, a_, u_, rps, scale), y0, w, a, u))


# ----------------------------------------------------------------------------- ELU over heads
@pytest.mark.parametrize("cell", A.ELU_CELLS, ids=lambda c: "rows%d-H%d-Fh%d%s%s%s" % (c[0], c[1], c[2], "-mean" if c[3] else "", "-elu" if c[4] else "",
                                                                                        "-base" if c[5] else ""))
def test_elu_heads(cell):
    nat = _nat()
    rows, H, Fh, mean, elu, base = cell
    n, Co = rows * H * Fh, (Fh if mean else H * Fh)
    vec = not mean and n % 4 == 0 and not base
    x = A.elu_inputs(cell)
    dy = A.rnd(6000 + n, rows, Co)
    xd, dyd = dmat(x.view(1, n), off=1 if base else 0), dy.cuda()

    def fwd():
        y = Out(1, rows * Co + 5)
        nat.call("elu_heads_fwd_f32", xd, rows, H, Fh, int(mean), int(elu), y.mat)
        return (y,)

    def bwd():
        dx = Out(1, n + 5)
        nat.call("elu_heads_bwd_f32", xd, dyd, rows, H, Fh, int(mean), int(elu), dx.mat)
        return (dx,)
    (y,) = twice("elu_vec4_fwd_kernel" if vec else "elu_heads_fwd_kernel", fwd)
    check("elu fwd %s" % (cell,), y, *[t.reshape(1, -1) for t in both(lambda x_: A.elu_heads_fwd(x_, H, Fh, mean, elu), x)])
    (dx,) = twice("elu_vec4_bwd_kernel" if vec else "elu_heads_bwd_kernel", bwd)
    check("elu bwd %s" % (cell,), dx, *[t.reshape(1, -1) for t in both(lambda x_, d_: A.elu_heads_bwd(x_, d_, H, Fh, mean, elu), x, dy)])
    if not mean:                                                                           # the special inputs: ELU(+-0) is 0 exactly, ELU(-30) is -1
        sp = A.elu_special_mask(cell).view(-1)
        got = y.mat[0, :n].cpu()[sp].view(H, 3)
        assert (got[:, :2] == 0).all() and (not elu or (got[:, 2] + 1).abs().max() < 1e-6)


# ----------------------------------------------------------------------------- parameters of the heads
@pytest.mark.parametrize("H", [1, 3, 8])
def test_pack_and_unpack_heads(H):
    nat = _nat()
    Fin, Fo = 5, 6
    ws, as_ = [A.rnd(7000 + h, Fin, Fo) for h in range(H)], [A.rnd(7100 + h, 2 * Fo) for h in range(H)]
    wd, ad = [t.cuda() for t in ws] + [None] * (8 - H), [t.cuda() for t in as_] + [None] * (8 - H)

    def pack():
        W, Ak = Out(Fin, H * Fo), Out(2, H * Fo)
        nat.call("pack_heads_f32", *wd, *ad, H, Fin, Fo, W.mat, Ak.mat)
        return W, Ak
    W, Ak = twice("pack_heads_kernel", pack)
    Wr, Ar = A.pack_heads(ws, as_)
    exact("pack W", W, Wr)
    exact("pack A", Ak, Ar.reshape(2, H * Fo))
    dW, dA0, dA1 = A.rnd(7200, Fin, H * Fo), A.rnd(7201, H, Fo), A.rnd(7202, H, Fo)
    for srcs in ((dW, dA0, dA1), (None, dA0, dA1), (dW, None, dA1), (dW, dA0, None), (None, None, None)):
        dev = [t.cuda() if t is not None else None for t in srcs]

        def unpack():
            gw, ga = Out(H * Fin, Fo), Out(H, 2 * Fo)
            nat.call("unpack_heads_f32", *dev, H, Fin, Fo, gw.mat, ga.mat)
            return gw, ga
        gw, ga = twice("unpack_heads_kernel", unpack)
        gwr, gar = A.unpack_heads(*srcs, H, Fin, Fo)
        exact("unpack gw", gw, gwr.reshape(H * Fin, Fo))                                    # (a null source: zeros, bit for bit)
        exact("unpack ga", ga, gar)


def test_pack_heads_refuses_a_ninth_head():
    W, Ak = Out(5, 54), Out(2, 54)
    p = torch.zeros(64, device="cuda")
    assert _nat().lib().tsgnn_pack_heads_max() == 8
    assert _rc("pack_heads_f32", *([p] * 16), 9, 5, 6, W.mat, Ak.mat) == EINVAL
    W.rest_untouched("pack H = 9", owned(W, 0, 0))
    Ak.rest_untouched("pack H = 9", owned(Ak, 0, 0))


# ----------------------------------------------------------------------------- the autograd node
_gb = {}


def _graph_batch(name, kind):
    if (name, kind) not in _gb:
        _gb[(name, kind)] = _build_graph_batch(name, kind)
    return _gb[(name, kind)]


def _build_graph_batch(name, kind):
    from two_stage_gnn_amd.graph import GraphBatch
    adj, sizes = G.batch(name)
    L = G.layout(name, kind)
    g = GraphBatch.from_dense_ghost1(adj.cuda(), sizes) if kind == "ghost1" else GraphBatch.from_dense(adj.cuda(), layout="padded")
    rowptr, col = g.rowptr.cpu(), g.col.cpu()[:int(g.nnz)]
    rp, cl = A.layout_csr(L)
    assert int(g.total_rows) == L.R and int(g.nmax) == L.N and torch.equal(rowptr, rp)
    assert torch.equal(torch.sort(A.row_of(rowptr) * L.R + col.long())[0], A.row_of(rp) * L.R + cl.long())
    assert g.graph_ptr.cpu().tolist() == L.graph_ptr.tolist()
    return g, L, rowptr, col


NODE_CELLS = [(name, kind, mode) for name in ("edges", "blocks31") for kind, mode in
              (("padded", "column+uniform"), ("ghost1", "column+uniform"), ("padded", "column"), ("padded", "target+drop"))]


@pytest.mark.parametrize("name,kind,mode", NODE_CELLS)
@pytest.mark.parametrize("mean_heads", [False, True], ids=["concat", "mean"])
def test_autograd_node_equals_float64_autograd_of_the_composition(name, kind, mode, mean_heads):
    """attention_aggregate + elu_heads: the output and the gradients of h, a_row, a_col"""
    from two_stage_gnn_amd import attention as att
    H, Fh, slope = 2, 8, 0.2
    g, L, rowptr, col = _graph_batch(name, kind)
    by_column, uni = mode.startswith("column"), mode == "column+uniform"
    uniform = (torch.from_numpy(L.row_mult), torch.from_numpy(L.row_graph), torch.from_numpy(L.graph_ptr), L.N) if uni else None
    inp = A.layer_inputs(L, H, Fh, 90 + len(name) + len(mode), rowptr, col)
    assert A.layer_margin(*inp, rowptr, col, H, Fh) >= G.MARGIN
    gen = torch.Generator().manual_seed(12)
    drop = ((torch.rand(max(col.numel(), 1), H, generator=gen) >= 0.3).float() / 0.7) if mode == "target+drop" else None
    dy = torch.randn(L.R, Fh if mean_heads else H * Fh, generator=gen)

    def ref(dt):
        leaves = [t.to(dt).requires_grad_(True) for t in inp]
        y = A.compose(*leaves, rowptr, col, H, Fh, slope, by_column, uniform, drop[:col.numel()] if drop is not None else None, mean_heads, True)
        return (y.detach(),) + torch.autograd.grad((y * dy.to(dt)).sum(), leaves)
    r64, r32 = ref(torch.float64), ref(torch.float32)
    leaves = [t.cuda().requires_grad_(True) for t in inp]
    pre = att.attention_aggregate(*leaves, g, H, slope, by_column, uni, drop.cuda() if drop is not None else None)
    y = att.elu_heads(pre, H, mean_heads, True)
    grads = torch.autograd.grad((y * dy.cuda()).sum(), leaves)
    what = "node %s %s %s %s" % (name, kind, mode, "mean" if mean_heads else "concat")
    for k, (nm, got) in enumerate(zip(("y", "dh", "da_row", "da_col"), (y,) + grads)):
        _check("%s %s" % (what, nm), got, r64[k], r32[k], K)


# ----------------------------------------------------------------------------- graphs without any edge, both GAT paths
@pytest.mark.parametrize("fused", [True, False], ids=["fused", "per-op"])
@pytest.mark.parametrize("n", [7, 1])
def test_encoder_on_a_graph_without_any_edge(n, fused, monkeypatch):
    """B = 1, n nodes, Nmax = 12, no entry at all (n = 1: no self loop): forward and backward of the two-layer encoder against
    oracle/dense_ref.gat_encoder.  The transpose's one-word placeholders are zero and the entry map is never built from them"""
    from oracle import dense_ref
    from two_stage_gnn_amd import gat_encoders as GE, gat_fused
    monkeypatch.setattr(gat_fused, "FUSED", fused)
    nmax, fin = 12, 5
    gen = torch.Generator().manual_seed(n)
    x = torch.zeros(1, nmax, fin)
    x[0, :n] = torch.randn(n, fin, generator=gen)
    adj = torch.zeros(1, nmax, nmax)
    sizes = np.array([n], dtype=np.int64)
    torch.manual_seed(5)
    m = GE.DGATEncoderGraph(fin, 8, 8, 2, None, num_layers=2, num_heads=[2, 2]).cuda()
    ge, go = torch.randn(1, 8, generator=gen), torch.randn(1, 8, generator=gen)
    p = {k: v.detach().cpu().clone().requires_grad_(True) for k, v in m.state_dict().items()}
    e_ref, o_ref = dense_ref.gat_encoder(p, x, adj)
    names = [k for k, _ in m.named_parameters()]
    g_ref = torch.autograd.grad((e_ref * ge).sum() + (o_ref * go).sum(), [p[k] for k in names], allow_unused=True)
    xd, ad = x.cuda(), adj.cuda()
    e, o = m(xd, ad, sizes)
    ((e * ge.cuda()).sum() + (o * go.cuda()).sum()).backward()
    g = m.packed_batch(xd, ad, sizes)[1]                                                   # (the cached batch of that call)
    assert int(g.nnz) == 0 and g.src_e_t.tolist() == [0] and g._t[1].tolist() == [0]
    assert getattr(g, "_inv_e_t", None) is None or g._inv_e_t.tolist() == [0]
    torch.testing.assert_close(e.detach().cpu(), e_ref.detach(), rtol=1e-4, atol=1e-4)
    torch.testing.assert_close(o.detach().cpu(), o_ref.detach(), rtol=1e-4, atol=1e-4)
    for k, gr in zip(names, g_ref):
        got = dict(m.named_parameters())[k].grad
        assert (got is None) == (gr is None), k
        if gr is not None:
            torch.testing.assert_close(got.cpu(), gr, rtol=1e-4, atol=1e-4, msg=lambda s, k=k: "%s: %s" % (k, s))
