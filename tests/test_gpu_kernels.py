"""GPU parity of the individual HIP kernels (through the C ABI) against the CPU oracle / dense torch math."""
import numpy as np
import pytest
import torch

from conftest import load_golden, params_of
from oracle import dense_ref as R
from util_graphs import dense_batch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def T():
    import two_stage_gnn_amd  # noqa
    from two_stage_gnn_amd import message_passing as mp
    from two_stage_gnn_amd.graph import GraphBatch
    return mp, GraphBatch


def csr_to_dense(g, n):
    rp = g.rowptr.cpu().numpy(); col = g.col.cpu().numpy()
    val = g.val.cpu().numpy() if g.val is not None else np.ones(len(col), np.float32)
    d = np.zeros((n, n), np.float32)
    for r in range(n):
        for e in range(rp[r], rp[r + 1]):
            d[r, col[e]] += val[e]
    return d


@pytest.mark.parametrize("weighted,symmetric", [(False, True), (True, True), (True, False)])
def test_dense_to_csr_layouts(T, weighted, symmetric):
    mp, GB = T
    x, adj, sizes = dense_batch(1, 5, 70, 3, weighted=weighted, symmetric=symmetric)
    # padded layout: block-diagonal of the padded matrices
    g = GB.from_dense(adj.cuda(), layout="padded")
    assert g.total_rows == 5 * 70 and g.n_ghost == 0
    d = csr_to_dense(g, g.total_rows)
    for b in range(5):
        np.testing.assert_array_equal(d[b * 70:(b + 1) * 70, b * 70:(b + 1) * 70], adj[b].numpy())
    assert d.sum() == pytest.approx(float(adj.sum()), rel=1e-6)
    # packed layout: real rows only + nmax empty ghost rows
    g = GB.from_dense(adj.cuda(), sizes=sizes, layout="packed")
    assert g.n_rows == sizes.sum() and g.n_ghost == 70
    d = csr_to_dense(g, g.total_rows)
    o = 0
    for b, n in enumerate(sizes):
        np.testing.assert_array_equal(d[o:o + n, o:o + n], adj[b, :n, :n].numpy())
        o += n
    assert d[o:].sum() == 0 and d[:, o:].sum() == 0
    # transpose
    rp, col, val = g.transposed()
    class G2: pass
    g2 = G2(); g2.rowptr, g2.col, g2.val = rp, col, val
    np.testing.assert_allclose(csr_to_dense(g2, g.total_rows), d.T)
    sc = g.slot_count.cpu().numpy()
    np.testing.assert_array_equal(sc, [(sizes > n).sum() for n in range(70)])


def test_scan_large(T):
    mp, GB = T
    from two_stage_gnn_amd.graph import exclusive_scan
    for n in [1, 7, 2048, 2049, 100003, 1 << 21]:
        c = torch.randint(0, 9, (n,), dtype=torch.int32, device="cuda")
        out = exclusive_scan(c).cpu().numpy()
        ref = np.concatenate([[0], np.cumsum(c.cpu().numpy())])
        np.testing.assert_array_equal(out, ref)


def test_coo_to_csr(T):
    mp, GB = T
    gen = torch.Generator().manual_seed(3)
    N, E = 200, 1500
    ei = torch.randint(0, N, (2, E), generator=gen)
    g = GB.from_edge_index(ei.cuda(), N)
    rp = g.rowptr.cpu().numpy(); col = g.col.cpu().numpy(); eid = g.eid.cpu().numpy()
    assert rp[-1] == E
    for i in range(N):
        es = np.nonzero(ei[1].numpy() == i)[0]          # stable: original edge order
        np.testing.assert_array_equal(eid[rp[i]:rp[i + 1]], es)
        np.testing.assert_array_equal(col[rp[i]:rp[i + 1]], ei[0].numpy()[es])
    with pytest.raises(IndexError):
        GB.from_edge_index(torch.tensor([[0, 1], [1, 999]]).cuda(), 10)


@pytest.mark.parametrize("F", [1, 3, 8, 48, 64, 89, 92, 128, 200, 256, 320])
@pytest.mark.parametrize("weighted", [False, True])
def test_spmm_vs_dense(T, F, weighted):
    mp, GB = T
    x, adj, sizes = dense_batch(F + weighted, 6, 90, F, weighted=weighted, p_edge=0.15)
    g = GB.from_dense(adj.cuda(), layout="padded")
    if not weighted:
        g.val = None
    xr = x.reshape(-1, F).cuda().requires_grad_(True)
    for add_self in (False, True):
        y = mp.aggregate(xr, g, add_self=add_self)
        ref = torch.matmul(adj, x) + (x if add_self else 0)
        torch.testing.assert_close(y.detach().cpu().reshape(6, 90, F), ref, rtol=1e-5, atol=1e-5)
    gy = torch.randn(6 * 90, F, generator=torch.Generator().manual_seed(5))
    y = mp.aggregate(xr, g, add_self=True)
    (y * gy.cuda()).sum().backward()
    gref = torch.matmul(adj.transpose(1, 2), gy.reshape(6, 90, F)) + gy.reshape(6, 90, F)
    torch.testing.assert_close(xr.grad.cpu().reshape(6, 90, F), gref, rtol=1e-5, atol=1e-5)


def test_spmm_high_degree_and_nonsymmetric(T):
    mp, GB = T
    x, adj, sizes = dense_batch(11, 2, 300, 128, p_edge=0.6, symmetric=False, weighted=True)   # degree ~180 > 64
    g = GB.from_dense(adj.cuda(), layout="padded")
    xr = x.reshape(-1, 128).cuda().requires_grad_(True)
    y = mp.aggregate(xr, g)
    torch.testing.assert_close(y.detach().cpu().reshape(2, 300, 128), adj @ x, rtol=1e-4, atol=1e-4)
    gy = torch.randn(600, 128)
    (y * gy.cuda()).sum().backward()
    torch.testing.assert_close(xr.grad.cpu().reshape(2, 300, 128), adj.transpose(1, 2) @ gy.reshape(2, 300, 128),
                               rtol=1e-4, atol=1e-4)


@pytest.mark.parametrize("K,N,normalize,bias", [(5, 7, True, True), (89, 128, True, True), (128, 128, True, False),
                                                 (92, 64, False, True), (33, 200, True, True), (128, 256, True, True),
                                                 (300, 20, True, True), (7, 1, False, True)])
def test_linear_l2norm(T, K, N, normalize, bias):
    mp, GB = T
    gen = torch.Generator().manual_seed(K * 1000 + N)
    R_ = 777
    z = torch.randn(R_, K + (3 if K == 89 else 0), generator=gen)
    if K == 89:
        z[:, 89:] = 0
    w = torch.randn(K, N, generator=gen) * 0.3
    b = torch.randn(N, generator=gen) if bias else None
    z[5] = 0                                         # a row whose pre-norm output is exactly the bias
    zc, wc = z.clone().requires_grad_(True), w.clone().requires_grad_(True)
    bc = b.clone().requires_grad_(True) if bias else None
    u = zc[:, :K] @ wc + (bc if bias else 0)
    ref = torch.nn.functional.normalize(u, p=2, dim=1) if normalize else u
    zg, wg = z.cuda().requires_grad_(True), w.cuda().requires_grad_(True)
    bg = b.cuda().requires_grad_(True) if bias else None
    v = mp.linear_l2norm(zg, wg, bg, normalize=normalize)
    torch.testing.assert_close(v.detach().cpu(), ref.detach(), rtol=2e-5, atol=2e-5)
    gy = torch.randn(R_, N, generator=gen)
    (ref * gy).sum().backward()
    (v * gy.cuda()).sum().backward()
    torch.testing.assert_close(zg.grad.cpu()[:, :K], zc.grad[:, :K], rtol=1e-4, atol=1e-4)
    torch.testing.assert_close(wg.grad.cpu(), wc.grad, rtol=1e-4, atol=2e-4)
    if bias:
        torch.testing.assert_close(bg.grad.cpu(), bc.grad, rtol=1e-4, atol=2e-4)


@pytest.mark.parametrize("tag", ["b5", "b1"])
def test_bn_slots_golden(T, tag):
    mp, GB = T
    g = load_golden("apply_bn_" + tag)
    x = torch.tensor(g["x"])
    B, N, F = x.shape
    gb = GB.structure_only(np.full(B, N), N, torch.device("cuda"), ghosts=False)
    xr = x.reshape(B * N, F).cuda().requires_grad_(True)
    y = mp.bn_slots(xr, gb, relu=False, bn=True)
    np.testing.assert_allclose(y.detach().cpu().numpy().reshape(B, N, F), g["y"], rtol=1e-4, atol=1e-5)
    (y * torch.tensor(g["gy"]).reshape(B * N, F).cuda()).sum().backward()
    np.testing.assert_allclose(xr.grad.cpu().numpy().reshape(B, N, F), g["gx"], rtol=1e-4, atol=2e-5)


def test_ghost_rows_equal_padded(T):
    """packed rows + per-slot ghost representatives == the reference's padded computation
    (relu + slot BN + max readout incl. ghost rows), forward and backward."""
    mp, GB = T
    B, nmax, F = 6, 40, 16
    sizes = np.array([40, 13, 27, 5, 31, 13])
    gen = torch.Generator().manual_seed(9)
    ghost_val = torch.randn(F, generator=gen)                  # what every padded row carries (normalize(bias))
    xp = ghost_val.expand(B, nmax, F).clone()
    for b, n in enumerate(sizes):
        xp[b, :n] = torch.randn(n, F, generator=gen)
    xp_ref = xp.clone().requires_grad_(True)
    y = R.bn_slots(torch.relu(xp_ref))
    out_ref = y.max(dim=1)[0]
    gout = torch.randn(B, F, generator=gen)
    gy = torch.randn(B, nmax, F, generator=gen) * (torch.arange(nmax)[None, :, None] < torch.tensor(sizes)[:, None, None])
    ((out_ref * gout).sum() + (y * gy).sum()).backward()

    g = GB.structure_only(sizes, nmax, torch.device("cuda"), ghosts=True)
    rows = torch.zeros(g.total_rows, F)
    o = 0
    for b, n in enumerate(sizes):
        rows[o:o + n] = xp[b, :n]; o += n
    rows[o:] = ghost_val
    rows = rows.cuda().requires_grad_(True)
    yr = mp.bn_slots(rows, g, relu=True, bn=True)
    out = mp.readout_max(yr, g)
    torch.testing.assert_close(out.detach().cpu(), out_ref.detach(), rtol=1e-4, atol=1e-5)
    gy_rows = torch.zeros(g.total_rows, F)
    o = 0
    for b, n in enumerate(sizes):
        gy_rows[o:o + n] = gy[b, :n]; o += n
    ((out * gout.cuda()).sum() + (yr * gy_rows.cuda()).sum()).backward()
    gr = rows.grad.cpu()
    o = 0
    for b, n in enumerate(sizes):
        torch.testing.assert_close(gr[o:o + n], xp_ref.grad[b, :n], rtol=1e-3, atol=2e-5); o += n
    # gradient of a ghost representative = sum over the padded copies it stands for
    gh = torch.zeros(nmax, F)
    for b, n in enumerate(sizes):
        gh[n:] += xp_ref.grad[b, n:]
    torch.testing.assert_close(gr[o:], gh, rtol=1e-3, atol=2e-5)


def test_pack_unpack(T):
    mp, GB = T
    x, adj, sizes = dense_batch(4, 4, 20, 6)
    g = GB.from_dense(adj.cuda(), sizes=sizes, layout="packed")
    xr = mp.pack_rows(x.cuda(), g, ld=8)
    assert xr.shape == (g.total_rows, 8)
    back = mp.unpack_rows(xr[:, :6].contiguous(), g)
    torch.testing.assert_close(back.cpu(), x)


@pytest.mark.parametrize("F,p_edge", [(128, 0.05), (64, 0.02), (92, 0.1), (256, 0.3)])
def test_ell_fast_path_equals_csr(T, F, p_edge):
    """fixed-width index table (+ CSR tail when a row has more than 16 neighbours) == CSR kernel"""
    mp, GB = T
    x, adj, sizes = dense_batch(int(F + 100 * p_edge), 5, 80, F, p_edge=p_edge)
    g = GB.from_dense(adj.cuda(), sizes=sizes, layout="packed")
    g.val = None
    xr = torch.zeros(g.total_rows, F)
    o = 0
    for b, n in enumerate(sizes):
        xr[o:o + n] = x[b, :n]; o += n
    xr = xr.cuda()
    ell, W, tail = g.ell()
    assert (tail is not None) == (p_edge >= 0.3)
    y_csr = mp.spmm_raw(g.rowptr, g.col, None, xr, g.total_rows)
    y_ell = mp.spmm_ell(g, xr)
    if tail is None:
        assert torch.equal(y_csr, y_ell)                       # same summation order: bitwise equal
    else:
        torch.testing.assert_close(y_ell, y_csr, rtol=1e-5, atol=1e-5)


def test_aggregation_properties_at_headline_size(T):
    """size-independent properties of the aggregation on the full BASELINE batch (DD-shaped, 32 graphs, Nmax 1000, F = 128), where
    the dense oracle is too slow to be the checker: A 1 = degree (bit-exact: small integers), linearity, symmetry
    <A x, z> = <x, A z>, and the three kernels that serve this size (CSR rows, fixed-width table, fused into the product)
    agreeing with each other"""
    mp, _ = T
    from two_stage_gnn_amd import synthetic, _native as nat
    hb = synthetic.host_batch(0, 32, "DD", 1000)
    g, _, _ = synthetic.to_device(hb, torch.device("cuda"))
    R, F = g.total_rows, 128
    gen = torch.Generator(device="cuda").manual_seed(3)
    x = torch.randn(R, F, generator=gen, device="cuda"); z = torch.randn(R, F, generator=gen, device="cuda")
    agg = lambda v: mp.spmm_raw(g.rowptr, g.col, None, v, R)
    deg = (g.rowptr[1:] - g.rowptr[:-1]).float()
    assert torch.equal(agg(torch.ones(R, F, device="cuda")), deg.unsqueeze(1).expand(R, F))
    ax, az = agg(x), agg(z)
    torch.testing.assert_close(agg(2.5 * x - 0.75 * z), 2.5 * ax - 0.75 * az, rtol=1e-4, atol=1e-4)
    lhs, rhs = (ax.double() * z.double()).sum(), (x.double() * az.double()).sum()
    assert abs(float(lhs - rhs)) <= 1e-6 * abs(float(lhs)) + 1e-6                      # TU graphs are undirected: A = A^T
    if mp.ell_ok(x):
        ell, W, tail = g.ell()
        y_ell = mp.spmm_ell(g, x)
        assert torch.equal(y_ell, ax) if tail is None else torch.allclose(y_ell, ax, rtol=1e-5, atol=1e-5)
        if tail is None:                                                                # fused into the product: z output = A x
            w = torch.eye(F, device="cuda"); v = torch.empty(g.n_rows, F, device="cuda"); zo = torch.empty(g.n_rows, F, device="cuda")
            nat.call("gather_rowgemm_f32", ell, W, None, None, x, F, w, F, 0, None, v, F, None, zo, F, g.n_rows, F, F, 0, 0)
            torch.testing.assert_close(zo, ax[:g.n_rows], rtol=1e-5, atol=1e-5)
            torch.testing.assert_close(v, ax[:g.n_rows], rtol=1e-4, atol=1e-4)


@pytest.mark.parametrize("rows,K,N,ldz", [(2629, 1, 128, 1), (70000, 3, 64, 4), (5, 4, 100, 4), (0, 1, 8, 1)])
def test_linear_wgrad_narrow_input(T, rows, K, N, ldz):
    """layers with <= 4 input columns (IMDB's single constant feature): dW = z^T du and db = colsum(du) from one pass over du"""
    mp, _ = T
    gen = torch.Generator(device="cuda").manual_seed(rows + K)
    z = torch.randn(max(rows, 1), ldz, generator=gen, device="cuda")[:rows]
    du = torch.randn(max(rows, 1), N, generator=gen, device="cuda")[:rows]
    dw, db = mp.linear_wgrad(z, K, du, True)
    assert dw.shape == (K, N) and db.shape == (N,)
    torch.testing.assert_close(dw.double(), z[:, :K].double().t() @ du.double(), rtol=1e-4, atol=1e-4)
    torch.testing.assert_close(db.double(), du.double().sum(0), rtol=1e-4, atol=1e-4)
    dw2, db2 = mp.linear_wgrad(z, K, du, False)
    assert db2 is None and torch.equal(dw2, dw)


@pytest.mark.parametrize("rows,K,N,trans_b,bias", [(1000, 92, 256, False, True), (1000, 256, 256, True, False), (1024, 64, 192, True, False),
                                                    (37, 128, 132, False, True), (4096, 128, 256, False, False),
                                                    (8518, 256, 264, False, False), (8518, 264, 256, True, False), (100, 20, 264, False, True),
                                                    (70, 36, 140, True, True), (1000, 89, 264, False, True), (33, 4, 160, True, False)])
def test_rowgemm_column_split(T, rows, K, N, trans_b, bias):
    """products without the row epilogue and more than 128 output columns run as column blocks of 128 (grid.y): same result as the
    torch product — ragged last column block (the 2H score columns of a GAT projection at its real size), partial row panel, K below
    and across a 32-wide chunk, padded K"""
    from two_stage_gnn_amd import _native as nat
    gen = torch.Generator(device="cuda").manual_seed(rows + N)
    ldk = (K + 3) // 4 * 4
    a = torch.randn(rows, ldk, generator=gen, device="cuda")
    w = torch.randn(N, ldk, generator=gen, device="cuda") if trans_b else torch.randn(K, N, generator=gen, device="cuda")
    b = torch.randn(N, generator=gen, device="cuda") if bias else None
    c = torch.full((rows, N + 4), 7.0, device="cuda")
    assert nat.lib().tsgnn_rowgemm_supported(a.data_ptr(), ldk, w.data_ptr(), w.stride(0), None, 0, K, N, int(trans_b))
    nat.call("rowgemm_f32", a, ldk, w, w.stride(0), int(trans_b), b, c, c.stride(0), None, rows, K, N, 0, 0)
    ref = a[:, :K].double() @ (w[:, :K].double().t() if trans_b else w.double())
    if bias:
        ref = ref + b.double()
    torch.testing.assert_close(c[:, :N].double(), ref, rtol=1e-4, atol=1e-4)
    assert bool((c[:, N:] == 7.0).all())                       # nothing written beyond the N columns


@pytest.mark.parametrize("F,weighted", [(128, False), (64, True), (92, False)])
def test_row_batched_gather_large(T, F, weighted):
    """>= 262144 rows switches to the row-batched kernel: must equal the one-row-per-group kernel bitwise."""
    mp, GB = T
    from two_stage_gnn_amd import synthetic
    hb = synthetic.host_batch(5, 1100, "DD", 600)
    g, x, _ = synthetic.to_device(hb, torch.device("cuda"))
    assert g.total_rows >= 262144
    X = torch.randn(g.total_rows, F, device="cuda")
    val = torch.rand(g.nnz, device="cuda") if weighted else None
    y_big = mp.spmm_raw(g.rowptr, g.col, val, X, g.total_rows, self_scalar=1.0)
    half = 200000                                           # below the threshold: classic kernel on two row ranges
    y_a = mp.spmm_raw(g.rowptr[: half + 1].contiguous(), g.col, val, X, half, self_scalar=1.0, out=torch.zeros_like(X))
    rp_b = g.rowptr[half:].contiguous()
    y_b = torch.zeros(g.total_rows - half, F, device="cuda")
    # second range: same kernel path (row count < threshold) needs x rows aligned: use self term via explicit add
    nat_rows = g.total_rows - half
    from two_stage_gnn_amd import _native as nat
    nat.call("csr_spmm_f32", rp_b, g.col, val, None, X, X.stride(0), y_b, y_b.stride(0), nat_rows, F, 0.0, 0, 0)
    y_b = y_b + X[half:]
    torch.testing.assert_close(y_big[:half], y_a[:half], rtol=0, atol=0)
    torch.testing.assert_close(y_big[half:], y_b, rtol=1e-6, atol=1e-6)


@pytest.mark.parametrize("normalize,bias", [(True, True), (True, False), (False, True)])
def test_rowgemm_fill_rows_equal_zero_input_rows(T, normalize, bias):
    """rows handed to the filler block (ghost rows: all-zero input) == the same rows pushed through the product."""
    mp, GB = T
    from two_stage_gnn_amd import _native as nat
    gen = torch.Generator().manual_seed(5)
    R_, nfill, K, N = 1000, 77, 128, 128
    z = torch.randn(R_ + nfill, K, generator=gen)
    z[R_:] = 0
    w = (torch.randn(K, N, generator=gen) * 0.2).cuda()
    b = torch.randn(N, generator=gen).cuda() if bias else None
    zg = z.cuda()
    outs = []
    for fill in (0, nfill):
        v = torch.full((R_ + nfill, N), float("nan"), device="cuda")
        rinv = torch.full((R_ + nfill,), float("nan"), device="cuda")
        nat.call("rowgemm_f32", zg, K, w, N, 0, b, v, N, rinv, R_ + nfill - fill, K, N, int(normalize), fill)
        torch.cuda.synchronize()
        outs.append((v.cpu(), rinv.cpu()))
    torch.testing.assert_close(outs[1][0], outs[0][0], rtol=1e-6, atol=1e-7)
    if normalize:
        torch.testing.assert_close(outs[1][1], outs[0][1], rtol=1e-6, atol=0)
    assert not torch.isnan(outs[1][0]).any()


@pytest.mark.parametrize("K,ld,N,trans_b,p_edge", [(128, 128, 128, False, 0.05), (89, 92, 128, False, 0.1), (128, 128, 64, False, 0.1),
                                                    (128, 128, 128, True, 0.1), (64, 64, 128, True, 0.05),
                                                    (128, 128, 128, False, 0.4), (128, 128, 128, True, 0.4)])
def test_gather_rowgemm_equals_aggregate_then_product(T, K, ld, N, trans_b, p_edge):
    """aggregation fused into the `.W` product (neighbour rows summed while the A panel is staged) == spmm then rowgemm,
    incl. rows with more neighbours than the register-staged eight or than the table (CSR tail), a partial last panel, a
    padded K and ghost fill rows."""
    mp, GB = T
    from two_stage_gnn_amd import _native as nat
    x, adj, sizes = dense_batch(77 + K + N, 6, 70, ld, p_edge=p_edge)
    g = GB.from_dense(adj.cuda(), sizes=sizes, layout="packed")
    g.val = None
    ell, W, tail = g.ell()
    assert (tail is not None) == (p_edge >= 0.3)          # the dense cases continue in the CSR tail (lists longer than 16)
    deg = (g.rowptr[1:] - g.rowptr[:-1])
    assert int(deg.max()) > 8 or p_edge < 0.1
    R_ = g.total_rows
    xr = torch.zeros(R_, ld)
    o = 0
    for b, n in enumerate(sizes):
        xr[o:o + n, :K] = x[b, :n, :K]; o += n
    xr = xr.cuda()
    gen = torch.Generator().manual_seed(3)
    if not trans_b:
        w = (torch.randn(K, N, generator=gen) * 0.2).cuda()
        bias = torch.randn(N, generator=gen).cuda()
        kk, nn_ = K, N
    else:
        w = (torch.randn(N, K, generator=gen) * 0.2).cuda()      # used transposed: out = z . w^T  -> [R, N]
        bias = None
        kk, nn_ = K, N
    nreal, nghost = g.n_rows, g.n_ghost
    z_ref = mp.spmm_ell(g, xr)
    v_ref = torch.empty(R_, nn_, device="cuda"); rinv_ref = torch.empty(R_, device="cuda")
    nat.call("rowgemm_f32", z_ref, ld, w, w.stride(0), int(trans_b), bias, v_ref, nn_, None if trans_b else rinv_ref, R_, kk, nn_,
             0 if trans_b else 1, 0)
    v = torch.full((R_, nn_), float("nan"), device="cuda"); rinv = torch.full((R_,), float("nan"), device="cuda")
    z = torch.full((R_, ld), float("nan"), device="cuda")
    nat.call("gather_rowgemm_f32", ell, W, tail[0] if tail is not None else None, tail[1] if tail is not None else None, xr, ld, w, w.stride(0), int(trans_b), bias, v, nn_, None if trans_b else rinv,
             None if trans_b else z, ld, nreal, kk, nn_, 0 if trans_b else 1, 0 if trans_b else nghost)
    torch.cuda.synchronize()
    rows = R_ if not trans_b else nreal
    torch.testing.assert_close(v[:rows], v_ref[:rows], rtol=2e-5, atol=2e-5)
    if not trans_b:
        torch.testing.assert_close(rinv, rinv_ref, rtol=2e-5, atol=0)
        kp = (K + 3) // 4 * 4
        torch.testing.assert_close(z[:nreal, :kp], z_ref[:nreal, :kp], rtol=1e-5, atol=1e-5)       # summation order differs


@pytest.mark.parametrize("R,K,N", [(128, 256, 128), (128, 128, 64), (128, 64, 2), (37, 50, 7)])
def test_linear_oi_matches_torch_linear(R, K, N):
    """x W^T + b with W in torch.nn.Linear's [out, in] layout (the SAGPool head, network.py:25-27,48-51)"""
    from two_stage_gnn_amd import message_passing as mp
    g = torch.Generator().manual_seed(R + K + N)
    x, w, b = torch.randn(R, K, generator=g), torch.randn(N, K, generator=g) * 0.1, torch.randn(N, generator=g)
    gy = torch.randn(R, N, generator=g)
    xr, wr, br = x.clone().requires_grad_(True), w.clone().requires_grad_(True), b.clone().requires_grad_(True)
    ref = torch.nn.functional.linear(xr, wr, br)
    (ref * gy).sum().backward()
    xg, wg, bg = x.cuda().requires_grad_(True), w.cuda().requires_grad_(True), b.cuda().requires_grad_(True)
    out = mp.linear_oi(xg, wg, bg)
    (out * gy.cuda()).sum().backward()
    torch.testing.assert_close(out.detach().cpu(), ref.detach(), rtol=1e-4, atol=1e-4)
    for a, c in ((xg, xr), (wg, wr), (bg, br)):
        torch.testing.assert_close(a.grad.cpu(), c.grad, rtol=1e-4, atol=1e-4)


@pytest.mark.parametrize("B,D0,D1,D2,C,p", [(128, 256, 128, 64, 2, 0.5), (6, 64, 32, 16, 2, 0.0), (37, 128, 60, 30, 5, 0.3)])
def test_mlp3_head_matches_torch(B, D0, D1, D2, C, p):
    """the SAGPool head (network.py:48-53) fused into one launch per direction, against torch's own ops with the same mask"""
    from two_stage_gnn_amd import message_passing as mp
    torch.manual_seed(B + D1)
    lins = [torch.nn.Linear(D0, D1), torch.nn.Linear(D1, D2), torch.nn.Linear(D2, C)]
    ref_lins = [torch.nn.Linear(D0, D1), torch.nn.Linear(D1, D2), torch.nn.Linear(D2, C)]
    for a, b in zip(lins, ref_lins):
        b.load_state_dict(a.state_dict())
    lins = [m.cuda() for m in lins]
    assert mp.mlp3_ok(torch.empty(B, D0, device="cuda"), *lins)
    x = torch.randn(B, D0)
    keep = torch.empty(B, D1).bernoulli_(1.0 - p) if p > 0 else None
    scale = 1.0 / (1.0 - p)
    xr = x.clone().requires_grad_(True)
    h = torch.relu(ref_lins[0](xr))
    if keep is not None:
        h = h * keep * scale
    ref = torch.log_softmax(ref_lins[2](torch.relu(ref_lins[1](h))), dim=-1)
    gy = torch.randn(B, C)
    (ref * gy).sum().backward()
    xg = x.cuda().requires_grad_(True)
    out = mp._Mlp3LogSoftmax.apply(xg, lins[0].weight, lins[0].bias, lins[1].weight, lins[1].bias, lins[2].weight, lins[2].bias,
                                   keep.cuda() if keep is not None else None, scale)
    (out * gy.cuda()).sum().backward()
    torch.testing.assert_close(out.detach().cpu(), ref.detach(), rtol=1e-4, atol=1e-5)
    torch.testing.assert_close(xg.grad.cpu(), xr.grad, rtol=1e-4, atol=1e-5)
    for a, b in zip(lins, ref_lins):
        torch.testing.assert_close(a.weight.grad.cpu(), b.weight.grad, rtol=1e-4, atol=1e-5)
        torch.testing.assert_close(a.bias.grad.cpu(), b.bias.grad, rtol=1e-4, atol=1e-5)


def test_mlp3_head_dropout_inside_the_launch():
    """mp.mlp3_log_softmax in training mode: the dropout mask is made inside the forward launch (Philox, device counter advanced by
    the launch).  With the regenerated mask handed to torch's own ops outputs and gradients agree like the no-dropout case; the
    keep rate is 1 - p; consecutive launches — and consecutive REPLAYS of a captured step — draw different masks"""
    from two_stage_gnn_amd import message_passing as mp
    B, D0, D1, D2, C, p = 128, 256, 128, 64, 2, 0.5
    torch.manual_seed(5)
    lins = [torch.nn.Linear(D0, D1).cuda(), torch.nn.Linear(D1, D2).cuda(), torch.nn.Linear(D2, C).cuda()]
    x = torch.randn(B, D0, device="cuda")
    xg = x.clone().requires_grad_(True)
    out = mp.mlp3_log_softmax(xg, *lins, p=p, training=True)
    pk, seed, used = mp.last_mlp3_dropout
    keep = mp.mlp3_dropout_mask(pk, seed, used, B, D1)
    assert set(keep.unique().tolist()) <= {0.0, 1.0} and abs(float(keep.mean()) - (1 - p)) < 0.03
    gy = torch.randn(B, C, device="cuda")
    (out * gy).sum().backward()
    xr = x.clone().requires_grad_(True)
    ws = [(l.weight.detach().clone().requires_grad_(True), l.bias.detach().clone().requires_grad_(True)) for l in lins]
    h = torch.relu(xr @ ws[0][0].t() + ws[0][1]) * keep / (1 - p)
    ref = torch.log_softmax(torch.relu(h @ ws[1][0].t() + ws[1][1]) @ ws[2][0].t() + ws[2][1], dim=-1)
    (ref * gy).sum().backward()
    torch.testing.assert_close(out.detach(), ref.detach(), rtol=1e-4, atol=1e-5)
    torch.testing.assert_close(xg.grad, xr.grad, rtol=1e-4, atol=1e-5)
    for l, (w, b) in zip(lins, ws):
        torch.testing.assert_close(l.weight.grad, w.grad, rtol=1e-4, atol=1e-5)
        torch.testing.assert_close(l.bias.grad, b.grad, rtol=1e-4, atol=1e-5)
    # a second launch: the counter has advanced by exactly one, the mask is another one
    mp.mlp3_log_softmax(x, *lins, p=p, training=True)
    _, _, used2 = mp.last_mlp3_dropout
    assert int(used2) == int(used) + 1
    assert not torch.equal(mp.mlp3_dropout_mask(pk, seed, used2, B, D1), keep)
    # replays of one captured forward: a new mask each time (the counter lives on the device)
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        g = torch.cuda.CUDAGraph()
        with torch.no_grad():
            mp.mlp3_log_softmax(x, *lins, p=p, training=True)
            torch.cuda.synchronize()
            with torch.cuda.graph(g, stream=st):
                y = mp.mlp3_log_softmax(x, *lins, p=p, training=True)
        _, _, used3 = mp.last_mlp3_dropout
        seen = []
        for _ in range(3):
            g.replay(); torch.cuda.synchronize()
            seen.append((int(used3), y.clone()))
    assert [s_[0] for s_ in seen] == [seen[0][0], seen[0][0] + 1, seen[0][0] + 2]
    assert not torch.equal(seen[0][1], seen[1][1]) and not torch.equal(seen[1][1], seen[2][1])


@pytest.mark.parametrize("K,ld,N,trans_b,normalize,fill", [(128, 128, 128, False, 1, 37), (89, 92, 128, False, 1, 0), (128, 128, 64, False, 0, 0),
                                                            (128, 128, 128, True, 0, 0), (64, 64, 128, True, 0, 0), (40, 40, 96, False, 1, 5)])
def test_rowgemm_large_batch_kernel_equals_row_panel_kernel(T, K, ld, N, trans_b, normalize, fill):
    """the B-stationary persistent kernel that tsgnn_rowgemm_f32 dispatches from 49,152 rows (rowgemm_big_body.h: W slice in
    registers for the whole K, double-buffered A panels, one barrier per panel) against the row-panel kernel: rows are
    independent, so the same call on two pieces below the threshold must give the same bits — incl. a partial last panel, a
    padded K, narrow N, the transposed operand, bias + L2 normalise + rinv, ghost fill rows — and a torch product agrees."""
    from two_stage_gnn_amd import _native as nat
    R = 50000 + 13                                       # > threshold, partial last panel
    gen = torch.Generator().manual_seed(5 + K + N)
    a = torch.zeros(R, ld); a[:, :K] = torch.randn(R, K, generator=gen)
    a = a.cuda()
    w = (torch.randn(N, K, generator=gen) if trans_b else torch.randn(K, N, generator=gen)).mul_(0.2).cuda()
    bias = None if trans_b else torch.randn(N, generator=gen).cuda()
    out = []
    for pieces in ([(0, R)], [(0, 32768), (32768, R)]):
        c = torch.full((R + fill, N), float("nan"), device="cuda")
        rinv = torch.full((R + fill,), float("nan"), device="cuda") if normalize else None
        names = []
        for lo, hi in pieces:
            last = hi == R
            nat.call("rowgemm_f32", a[lo:hi], ld, w, w.stride(0), int(trans_b), bias, c[lo:], N, rinv[lo:] if normalize else None, hi - lo, K, N,
                     normalize, fill if last else 0)
            names.append(nat.last_kernel())
        out.append((c, rinv, names))
    torch.cuda.synchronize()
    assert out[0][2][0].startswith("rowgemm_big_kernel"), out[0][2]
    assert all(not n.startswith("rowgemm_big_kernel") for n in out[1][2]), out[1][2]
    assert not torch.isnan(out[0][0]).any()
    torch.testing.assert_close(out[0][0], out[1][0], rtol=0, atol=0)
    if normalize:
        torch.testing.assert_close(out[0][1], out[1][1], rtol=0, atol=0)
    ref = a[:, :K] @ (w.t() if trans_b else w)
    if bias is not None:
        ref = ref + bias
    if normalize:
        ref = torch.nn.functional.normalize(ref, p=2, dim=1)
    torch.testing.assert_close(out[0][0][:R], ref, rtol=2e-4, atol=2e-4)


@pytest.mark.parametrize("F,ln,relu,with_dxs", [(128, 1, 1, True), (64, 1, 1, False), (200, 1, 1, True), (128, 0, 0, True)])
def test_row_post_bwd_against_autograd(T, F, ln, relu, with_dxs):
    """tsgnn_row_post_bwd_f32 (readout winners + per-row layer norm + ReLU + L2 normalise backward in one pass; the triplet step's
    row-local counterpart of slot_post_bwd) against torch autograd through the same chain: real rows take the next layer's gradient
    and the readout gradient of their own graph, ghost rows (no edges) only the readout gradients — of EVERY graph that picked them"""
    from two_stage_gnn_amd import _native as nat
    gen = torch.Generator().manual_seed(F + ln)
    sizes, n_ghost, B = [7, 12, 5], 6, 3
    n_real, R = sum(sizes), sum(sizes) + 6
    row_graph = torch.repeat_interleave(torch.arange(B), torch.tensor(sizes)).int()
    u = torch.randn(R, F, generator=gen, dtype=torch.float64, requires_grad=True)
    nrm = u.norm(dim=1, keepdim=True).clamp_min(1e-12)
    v = u / nrm
    y = torch.relu(v) if relu else v
    if ln:
        mu = y.mean(1, keepdim=True)
        y = (y - mu) / torch.sqrt(((y - mu) ** 2).mean(1, keepdim=True) + 1e-5)
    # readout winners: random rows of the own graph, or a ghost row (shared by several graphs)
    arg = torch.empty(B, F, dtype=torch.int32)
    off = 0
    for b, n in enumerate(sizes):
        own = torch.randint(off, off + n, (F,), generator=gen)
        gh = n_real + torch.randint(0, n_ghost, (F,), generator=gen)
        arg[b] = torch.where(torch.rand(F, generator=gen) < 0.3, gh, own).int()
        off += n
    dout = torch.randn(B, F, generator=gen, dtype=torch.float64)
    dxs = torch.randn(R, F, generator=gen, dtype=torch.float64)
    dy = torch.zeros(R, F, dtype=torch.float64)
    if with_dxs:
        dy[:n_real] += dxs[:n_real]
    for b in range(B):
        dy[arg[b].long(), torch.arange(F)] += dout[b]
    (y * dy).sum().backward()
    vg = v.detach().float().cuda()
    yr = torch.relu(vg) if relu else vg
    mean = yr.mean(1).contiguous() if ln else None
    rstd = (1.0 / torch.sqrt(((yr - yr.mean(1, keepdim=True)) ** 2).mean(1) + 1e-5)).contiguous() if ln else None
    rinv = (1.0 / nrm.detach().float().view(-1)).cuda()
    du = torch.full((R, F), float("nan"), device="cuda")
    dx_g = dxs.float().cuda() if with_dxs else None
    nat.call("row_post_bwd_f32", row_graph.cuda(), B, n_real, R, vg, vg.stride(0), dx_g, dx_g.stride(0) if with_dxs else 0,
             dout.float().cuda(), F, arg.cuda(), F, relu, ln, mean, rstd, rinv, du, du.stride(0))
    torch.testing.assert_close(du.cpu().double(), u.grad, rtol=2e-4, atol=2e-5)


def _fixed_order_sum(x):
    """float32 emulation of the reduction's order over x[nslab, E]: four groups of contiguous slab ranges, four accumulators each,
    (a0 + a1) + (a2 + a3), the groups added in order"""
    nslab = x.shape[0]
    per = (nslab + 3) // 4
    g = []
    for grp in range(4):
        a = [np.zeros(x.shape[1], np.float32) for _ in range(4)]
        s, s1 = grp * per, min(nslab, grp * per + per)
        while s + 4 <= s1:
            for u in range(4):
                a[u] = a[u] + x[s + u]
            s += 4
        while s < s1:
            a[0] = a[0] + x[s]
            s += 1
        g.append((a[0] + a[1]) + (a[2] + a[3]))
    return (g[0] + g[1]) + (g[2] + g[3])


def test_wgrad_reduce_every_set_kind_bitwise(T):
    """mp.wgrad_reduce (tsgnn_wgrad_reduce_sets_f32): [K, N] and [N, K] (lddw > K) sets, blocked matrices in both layouts, score-layer
    rows with a tail and GraphConv-scorer rows with a dw column offset — 14 sets, two launches — against the fixed order in float32,
    bit for bit; |grad|^2 shares per block and ONE step-counter advance"""
    mp, _ = T
    WB = 129 * 128                                               # slab floats of a 128 x 128 output block (blocked matrices)
    g = torch.Generator().manual_seed(11)
    F = 20
    dev = torch.device("cuda")
    # (name, nslab, K, N, kn, lddw, with_db, n_db, with_tail, blocked)
    kinds = [("kn", 1, 6, 8, 1, 8, True, 8, False, False), ("oi", 3, 5, 12, 0, 8, True, 12, False, False),
             ("blk_kn", 4, 200, 264, 1, 268, True, 264, False, True), ("blk_oi", 5, 132, 140, 0, 136, False, 140, False, True),
             ("rows", 17, 0, F + 4, 0, 0, True, F, True, False), ("gc_rows", 5, 0, 2 * F + 4, 0, F + 4, True, F, True, False)]
    sets, host, outs = [], [], []
    for name, nslab, K, N, kn, lddw, with_db, n_db, with_tail, blocked in kinds:
        nblk = ((K + 127) // 128) * ((N + 127) // 128) if blocked else 1
        ws = torch.randn(nblk * nslab * (WB if blocked else (K + 1) * N), generator=g)
        if K > 0:
            dw = torch.full((K, lddw) if kn else (N, lddw), 7.0, device=dev)
        else:
            dw = torch.full((n_db + 2,), 7.0, device=dev) if name == "gc_rows" else None
        db = torch.full((n_db + 3,), 7.0, device=dev) if with_db else None
        tail = torch.full((2,), 7.0, device=dev) if with_tail else None
        sets.append(mp.wgrad_set(ws.to(dev), nslab, K, N, dw, db, n_db=n_db, tail=tail, kn=kn, lddw=lddw, blocked=blocked))
        host.append((name, ws.numpy(), nslab, K, N, kn, lddw, n_db, blocked))
        outs.append((dw, db, tail))
    sink = mp.GradSink()
    sink.norm_parts = torch.full((4096,), -1.0, device=dev)
    sink.step_state = torch.full((4,), 5.0, device=dev)
    sink.norm_enabled = True
    assert mp.wgrad_reduce(sets, norm_sink=sink) and sink.stepped
    torch.cuda.synchronize()
    parts = sink.norm_parts.cpu().numpy()
    assert float(sink.step_state[0]) == 6.0 and float(sink.step_state[1]) == 5.0          # one advance for both launches
    blk = 0
    for (name, ws, nslab, K, N, kn, lddw, n_db, blocked), (dw, db, tail) in zip(host, outs):
        want_dw = np.full(tuple(dw.shape), 7.0, np.float32) if dw is not None else None
        want_db = np.full(tuple(db.shape), 7.0, np.float32) if db is not None else None
        want_tail = np.full(2, 7.0, np.float32) if tail is not None else None
        NB = (N + 127) // 128 if blocked else 1
        for t in range((((K + 127) // 128) * NB) if blocked else 1):
            kb, nb = divmod(t, NB)
            kc, nc = (min(128, K - 128 * kb), min(128, N - 128 * nb)) if blocked else (K, N)
            x = ws[t * nslab * WB:][:nslab * (kc + 1) * nc].reshape(nslab, (kc + 1) * nc)     # block t's slabs, packed [nslab][kc + 1][nc]
            img = _fixed_order_sum(x).reshape(kc + 1, nc)
            wrote = np.zeros((kc + 1, nc), bool)
            wrote[:kc] = True
            r0, c0 = (128 * kb, 128 * nb) if blocked else (0, 0)
            if kc > 0:
                if kn:
                    want_dw[r0:r0 + kc, c0:c0 + nc] = img[:kc]
                else:
                    want_dw[c0:c0 + nc, r0:r0 + kc] = img[:kc].T
            if want_db is not None and kb == 0:
                want_db[c0:c0 + min(nc, n_db)] = img[kc, :n_db]
                wrote[kc, :n_db] = True
            if want_tail is not None:
                want_tail[0] = img[kc, n_db]
                wrote[kc, n_db] = True
            if K == 0 and want_dw is not None:
                want_dw[:n_db] = img[0, lddw:lddw + n_db]
                wrote[0, lddw:lddw + n_db] = True
            sq = np.where(wrote, img.astype(np.float64) ** 2, 0.0).reshape(-1)
            nb_set = -(-sq.size // 64)
            np.testing.assert_allclose(parts[blk:blk + nb_set], np.add.reduceat(sq, np.arange(0, sq.size, 64)), rtol=3e-5, atol=1e-30,
                                       err_msg=name)
            blk += nb_set
        for got, want in ((dw, want_dw), (db, want_db), (tail, want_tail)):
            if got is not None:
                assert np.array_equal(got.cpu().numpy(), want), name
    assert sink.norm_used == blk and float(parts[blk]) == -1.0                             # the slots the library counted, no more


@pytest.mark.parametrize("R_,K,N,bias", [(8183, 192, 64, True), (1024, 192, 64, True), (500, 64, 128, False), (300, 260, 200, True)])
def test_linear_backward_products_merged_equals_separate(T, R_, K, N, bias):
    """torch.nn.Linear's backward with the weight-gradient slabs beside the input-gradient product in one launch
    (tsgnn_linear_bwd_products_f32 + a blocked tsgnn_wgrad_reduce_sets_f32 record; DiffPool's assignment predictor) == the separate launches,
    bit for bit, and torch"""
    mp, _ = T
    from two_stage_gnn_amd import _native as nat
    gen = torch.Generator(device="cuda").manual_seed(R_ + K + N)
    x = torch.randn(R_, K, generator=gen, device="cuda")
    dy = torch.randn(R_, N, generator=gen, device="cuda")
    w = torch.randn(N, K, generator=gen, device="cuda") * 0.1
    got = mp.linear_bwd_products(x, K, dy, w, bias)
    assert got is not None
    dw, db, dx = got
    dw_s, db_s = mp.linear_wgrad_oi(x, K, dy, bias)
    dx_s = torch.empty(R_, K, device="cuda")
    nat.call("rowgemm_f32", dy, dy.stride(0), w, w.stride(0), 0, None, dx_s, dx_s.stride(0), None, R_, N, K, 0, 0)
    assert torch.equal(dw, dw_s) and (not bias or torch.equal(db, db_s))
    torch.testing.assert_close(dx, dx_s, rtol=1e-5, atol=1e-5)            # (large row counts take the B-stationary kernel separately)
    torch.testing.assert_close(dw.double(), dy.double().t() @ x.double(), rtol=1e-4, atol=1e-3)
    torch.testing.assert_close(dx.double(), dy.double() @ w.double(), rtol=1e-4, atol=1e-4)
    if bias:
        torch.testing.assert_close(db.double(), dy.double().sum(0), rtol=1e-4, atol=1e-3)
    # through the autograd node, switch on and off
    outs = []
    for on in (True, False):
        mp.LINEAR_MERGED_BWD = on
        try:
            xg, wg = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
            bg = torch.zeros(N, device="cuda", requires_grad=True) if bias else None
            (mp.linear_oi(xg, wg, bg) * dy).sum().backward()
            outs.append((xg.grad, wg.grad, bg.grad if bias else None))
        finally:
            mp.LINEAR_MERGED_BWD = True
    torch.testing.assert_close(outs[0][0], outs[1][0], rtol=1e-5, atol=1e-5)
    assert torch.equal(outs[0][1], outs[1][1])
