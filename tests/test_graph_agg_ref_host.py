"""tests/graph_agg_ref.py anchored (no GPU): every restatement against an independent statement of the same thing — dense float64 matrix
algebra, float64 autograd, a python loop over the edge list, oracle/pyg_ref.gcn_norm — on small random graphs with repeated entries, self
loops, empty rows and empty columns."""
import ctypes

import numpy as np
import pytest
import torch

import graph_agg_ref as R
from oracle import pyg_ref as P

D = torch.float64


def _graph(seed, n, E, loops=True):
    """directed multigraph: E random edges (repeats happen), rows 0 and n-1 without in-edges, column 1 without out-edges"""
    g = torch.Generator().manual_seed(seed)
    src = torch.randint(0, n, (E,), generator=g)
    dst = torch.randint(1, max(n - 1, 2), (E,), generator=g)
    keep = src != 1
    if not loops:
        keep &= src != dst
    return torch.stack([src[keep], dst[keep]])


def _csr(seed, n, E, weighted=True, **kw):
    ei = _graph(seed, n, E, **kw)
    rp, col, eid = R.coo_to_csr(ei, n)
    val = torch.randn(ei.size(1), dtype=D, generator=torch.Generator().manual_seed(seed + 1)).numpy() if weighted else None
    return ei, rp, col, eid, val


@pytest.mark.parametrize("seed,n,E", [(0, 1, 0), (1, 9, 0), (2, 9, 40), (3, 40, 300)])
def test_scan_row_maps_and_coo(seed, n, E):
    ei = _graph(seed, n, E) if E else torch.zeros(2, 0, dtype=torch.int64)
    rp, col, eid = R.coo_to_csr(ei, n)
    assert rp[0] == 0 and rp[-1] == ei.size(1) and rp.size == n + 1
    A = torch.zeros(n, n, dtype=D)
    for s, t in zip(ei[0].tolist(), ei[1].tolist()):
        A[t, s] += 1                                         # repeated edges counted
    assert torch.equal(R.to_dense(rp, col), A)
    for i in range(n):                                       # stable: original edge order inside a row
        es = np.nonzero(ei[1].numpy() == i)[0]
        np.testing.assert_array_equal(eid[rp[i]:rp[i + 1]], es)
        np.testing.assert_array_equal(col[rp[i]:rp[i + 1]], ei[0].numpy()[es])
    c = np.diff(rp)
    ref = [0]
    for v in c.tolist():
        ref.append(ref[-1] + v)
    np.testing.assert_array_equal(R.scan(c), ref)
    np.testing.assert_array_equal(R.scan([]), [0])


def test_row_maps():
    for sizes in ([5], [0, 3, 0, 0, 2, 1, 0], [1, 1, 1], [0, 0, 4]):
        gp = R.scan(sizes)
        rg, rs = R.row_maps(gp, gp[-1])
        want_g = [b for b, s in enumerate(sizes) for _ in range(s)]
        want_s = [k for s in sizes for k in range(s)]
        np.testing.assert_array_equal(rg, want_g)
        np.testing.assert_array_equal(rs, want_s)


@pytest.mark.parametrize("packed", [False, True])
def test_dense_to_csr(packed):
    g = torch.Generator().manual_seed(5)
    B, nmax = 4, 7
    adj = torch.randn(B, nmax, nmax, generator=g) * (torch.rand(B, nmax, nmax, generator=g) < 0.4)
    adj[1, 2, 3] = -0.0                                      # dropped
    adj[1, 0, 1] = float("nan")                              # kept
    adj[2] = 0
    sizes = np.array([7, 5, 3, 0]) if packed else None
    rp, col, val = R.dense_to_csr(adj.numpy(), sizes, n_ghost=3 if packed else 0)
    sz = sizes if packed else np.full(B, nmax)
    n = int(sz.sum())
    assert rp.size == n + (3 if packed else 0) + 1 and (rp[n:] == rp[n]).all()
    want = torch.zeros(n, n, dtype=D)
    off = 0
    for b in range(B):
        s = int(sz[b])
        want[off:off + s, off:off + s] = adj[b, :s, :s].double()
        off += s
    got = R.to_dense(rp[:n + 1], col, val)
    assert torch.equal(torch.isnan(got), torch.isnan(want))
    assert torch.equal(torch.nan_to_num(got, nan=7.0), torch.nan_to_num(want, nan=7.0))
    assert not bool((torch.as_tensor(val) == 0).any()), "a zero (or -0.0) entry was kept"
    for r in range(n):
        assert (np.diff(col[rp[r]:rp[r + 1]]) > 0).all()     # columns ascend
    if packed:                                               # nothing outside [:n_b, :n_b] is read
        adj2 = adj.clone()
        for b in range(B):
            adj2[b, int(sz[b]):, :] = float("nan")
            adj2[b, :, int(sz[b]):] = float("nan")
        rp2, col2, val2 = R.dense_to_csr(adj2.numpy(), sizes, n_ghost=3)
        np.testing.assert_array_equal(rp2, rp)
        np.testing.assert_array_equal(col2, col)
        np.testing.assert_array_equal(val2.view(np.int32), val.view(np.int32))


@pytest.mark.parametrize("seed,n,E", [(2, 9, 40), (3, 40, 300), (4, 12, 0)])
def test_transpose(seed, n, E):
    ei, rp, col, eid, val = _csr(seed, n, E)
    rpt, colt, valt, src_e = R.transpose(rp, col, val)
    A = R.to_dense(rp, col, val)
    assert torch.equal(R.to_dense(rpt, colt, valt), A.t())
    np.testing.assert_array_equal(val[src_e], valt)
    np.testing.assert_array_equal(np.sort(src_e), np.arange(rp[-1]))
    rows = R.rows_of(rp)
    for c in range(n):                                       # ordered by (source row, source entry); entry p pairs with src_e[p]
        s = slice(rpt[c], rpt[c + 1])
        assert (col[src_e[s]] == c).all() and (rows[src_e[s]] == colt[s]).all()
        key = colt[s] * (rp[-1] + 1) + src_e[s]
        assert (np.diff(key) > 0).all()
    assert R.transpose(rp, col, None)[2] is None


@pytest.mark.parametrize("relu_in", [False, True])
@pytest.mark.parametrize("weighted", [False, True])
def test_spmm_equals_dense(weighted, relu_in):
    n, F = 30, 5
    ei, rp, col, eid, val = _csr(7, n, 200, weighted=weighted)
    g = torch.Generator().manual_seed(8)
    x = torch.randn(n + 3, F, dtype=D, generator=g)          # (more rows than the CSR has: only x[:n] carries a self term)
    x[3] = 0
    self_w = torch.randn(n, dtype=D, generator=g)
    y0 = torch.randn(n, F, dtype=D, generator=g)
    A = R.to_dense(rp, col, val, n_cols=n + 3)
    f = x.clamp_min(0) if relu_in else x
    torch.testing.assert_close(R.spmm(rp, col, val, x, relu_in=relu_in), A @ f, rtol=1e-13, atol=1e-13)
    torch.testing.assert_close(R.spmm(rp, col, val, x, self_scalar=1.0, relu_in=relu_in), A @ f + f[:n], rtol=1e-13, atol=1e-13)
    torch.testing.assert_close(R.spmm(rp, col, val, x, self_w=self_w, self_scalar=0.5, relu_in=relu_in, y0=y0),
                               A @ f + (self_w + 0.5)[:, None] * f[:n] + y0, rtol=1e-13, atol=1e-13)
    # the chunked path gives the same rows
    old = R.CHUNK_ENTRIES
    try:
        R.CHUNK_ENTRIES = 7
        few = list(R._row_chunks(rp))
        assert few[0][0] == 0 and few[-1][1] == n and all(a[1] == b[0] for a, b in zip(few, few[1:])) and len(few) > 3
        chunked = R.spmm(rp, col, val, x)
    finally:
        R.CHUNK_ENTRIES = old
    torch.testing.assert_close(chunked, A @ x, rtol=1e-13, atol=1e-13)
    r32 = R.spmm(rp, col, val, x, self_w=self_w, self_scalar=0.5, dtype=torch.float32)
    assert r32.dtype == torch.float32


def test_sddmm_equals_autograd():
    n, F = 25, 6
    ei, rp, col, eid, val = _csr(9, n, 150)
    g = torch.Generator().manual_seed(10)
    x = torch.randn(n, F, dtype=D, generator=g)
    dy = torch.randn(n, F, dtype=D, generator=g)
    v = torch.as_tensor(val).clone().requires_grad_(True)
    s = torch.randn(n, dtype=D, generator=g).requires_grad_(True)
    rows = torch.as_tensor(R.rows_of(rp))
    y = torch.zeros(n, F, dtype=D).index_add_(0, rows, x[torch.as_tensor(col)] * v[:, None]) + s[:, None] * x
    torch.testing.assert_close(y.detach(), R.spmm(rp, col, val, x, self_w=s.detach()), rtol=1e-13, atol=1e-13)
    (y * dy).sum().backward()
    dval, dself = R.sddmm(rp, col, dy, x)
    torch.testing.assert_close(dval, v.grad, rtol=1e-13, atol=1e-13)
    torch.testing.assert_close(dself, s.grad, rtol=1e-13, atol=1e-13)


@pytest.mark.parametrize("improved", [False, True])
@pytest.mark.parametrize("loops", [False, True])
@pytest.mark.parametrize("weighted", [False, True])
def test_gcn_norm_equals_pyg(weighted, loops, improved):
    n = 20
    ei = _graph(11, n, 90, loops=False)
    code = torch.unique(ei[0] * n + ei[1])                    # (PyG keeps ONE weight per existing self loop: simple graph here)
    ei = torch.stack([code // n, code % n])
    if loops:
        lp = torch.tensor([2, 5, 11])
        ei = torch.cat([ei, torch.stack([lp, lp])], 1)
    w = torch.rand(ei.size(1), dtype=D, generator=torch.Generator().manual_seed(12)) + 0.1 if weighted else None
    rp, col, eid = R.coo_to_csr(ei, n)
    val = None if w is None else w.numpy()[eid]
    dinv, val_out, self_w = R.gcn_norm(rp, col, val, 2.0 if improved else 1.0)
    got = R.to_dense(rp, col, val_out.numpy()) + torch.diag(self_w)
    prow, pcol, pw = P.gcn_norm(ei, n, w, improved=improved, dtype=D)
    want = torch.zeros(n, n, dtype=D).index_put_((pcol, prow), pw, accumulate=True)
    torch.testing.assert_close(got, want, rtol=1e-13, atol=1e-13)
    has = torch.zeros(n, dtype=torch.bool)
    if loops:
        has[lp] = True
    assert torch.equal(self_w == 0, has)
    assert bool((dinv > 0).all())


def test_gcn_norm_edges_of_the_rule():
    # row 0 isolated, row 1 two self loops (both kept), row 2 weights summing to -1, row 3 weights summing to 0 with a self loop
    rp = np.array([0, 0, 3, 5, 7])
    col = np.array([1, 0, 1, 0, 1, 3, 0])
    val = np.array([0.5, 1.0, 0.25, -3.0, 1.0, 2.0, -2.0])
    dinv, vo, sw = R.gcn_norm(rp, col, val, 0.0)
    assert dinv[0] == 0 and sw[0] == 0                       # isolated, self_fill 0: degree 0
    assert float(dinv[1]) == pytest.approx(1.75 ** -0.5) and sw[1] == 0
    assert dinv[2] == 0 and dinv[3] == 0                     # -3 + 1 + 0 <= 0 ;  2 - 2 = 0 (has a self loop: nothing added)
    assert bool((vo[3:] == 0).all())
    dinv, vo, sw = R.gcn_norm(rp, col, val, 2.0)
    assert float(dinv[0]) == pytest.approx(2 ** -0.5) and float(sw[0]) == pytest.approx(1.0)
    assert dinv[2] == 0                                      # -2 + 2 = 0
    assert float(vo[0]) == pytest.approx(0.5 / 1.75)


@pytest.mark.parametrize("W", [4, 8, 16])
def test_ell_plus_tail_is_the_csr(W):
    deg = [0, 1, W - 1, W, W + 1, 0, 40, 3]
    rp = R.scan(deg)
    col = np.random.default_rng(3).integers(0, len(deg), rp[-1])
    table, tp, tc = R.to_ell(rp, col, W)
    assert table.shape == (len(deg), W) and tp[-1] == tc.size == sum(max(d - W, 0) for d in deg)
    for r, d in enumerate(deg):
        got = np.concatenate([table[r][table[r] >= 0], tc[tp[r]:tp[r + 1]]])
        np.testing.assert_array_equal(got, col[rp[r]:rp[r + 1]])
        assert (table[r, min(d, W):] == -1).all() and (table[r, :min(d, W)] >= 0).all()
    assert R.ell_width(rp) == 16 and R.ell_width(R.scan([0, 4])) == 4 and R.ell_width(R.scan([5])) == 8
    assert R.ell_width(R.scan([8, 1])) == 8 and R.ell_width(R.scan([9])) == 16 and R.ell_width(R.scan([0, 0])) == 4


def test_coo_fill_takes_the_column_bound_and_a_flag():
    """tsgnn_coo_fill checks `other` against n_cols and reports through a nullable flag word; bad descriptions come back as EINVAL before
    any launch (no GPU needed)"""
    from two_stage_gnn_amd import _native as nat
    names = [p[1] for p in nat.parse_header()["tsgnn_coo_fill"][1]]
    assert names == ["key", "other", "E", "n_rows", "n_cols", "rowptr", "cursor", "col", "eid", "bad_flag", "stream"]
    L = nat.lib()
    one = (ctypes.c_int * 4)()
    p = ctypes.cast(one, ctypes.c_void_p)
    assert L.tsgnn_coo_fill(None, None, 0, 4, -1, p, p, None, None, None, None) == -1          # negative column bound
    assert L.tsgnn_coo_fill(None, None, 1, 4, 4, p, p, p, p, None, None) == -1                 # edges without an edge list
    assert L.tsgnn_coo_fill(None, None, 0, 4, 4, p, p, None, None, None, None) == 0            # no edge: nothing to do, flag nullable
