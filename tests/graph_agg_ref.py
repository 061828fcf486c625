"""Plain restatements of what csrc/graph_build.hip and csrc/aggregate.hip compute (tests/test_gpu_graph_aggregate.py compares the kernels
with them, tests/test_graph_agg_ref_host.py pins them on the CPU).  TEST INFRASTRUCTURE: no project kernel.

The integer builders (numpy, int64) are exact.  The float operations take a ``dtype``: float64 is the reference, the same code in float32
is the yardstick of tests/fp32_yardstick.py.  CSR arrays are numpy or torch; features are torch tensors."""
import numpy as np
import torch

D = torch.float64


def _np(a):
    if isinstance(a, torch.Tensor):
        a = a.detach().cpu().numpy()
    return np.asarray(a)


def _idx(a):
    return torch.as_tensor(_np(a).astype(np.int64))


# ============================================================================= builders (exact)
def scan(counts):
    """int[n] -> int64[n + 1] exclusive prefix sums, the total last"""
    c = _np(counts).astype(np.int64).reshape(-1)
    out = np.zeros(c.size + 1, dtype=np.int64)
    np.cumsum(c, out=out[1:])
    return out


def row_maps(graph_ptr, n_rows):
    """(row_graph, row_slot) of rows laid out graph after graph: row r belongs to the LAST graph b < B with graph_ptr[b] <= r (an empty
    graph owns no row), its slot is r - graph_ptr[b]"""
    gp = _np(graph_ptr).astype(np.int64)
    r = np.arange(int(n_rows), dtype=np.int64)
    rg = np.searchsorted(gp[:-1], r, side="right") - 1
    return rg, r - gp[rg]


def dense_to_csr(adj, sizes=None, n_ghost=0):
    """adj [B, nmax, nmax] -> (rowptr, col, val) over rows graph after graph: sizes given (packed) graph b has sizes[b] rows and only
    adj[b, n, :sizes[b]] is read; sizes None (padded) every graph has nmax rows.  Columns ascend; an entry is kept iff it is != 0 (-0.0 is
    dropped, NaN is kept); column ids are row ids of the batch.  n_ghost empty rows are appended."""
    a = _np(adj)
    B, nmax = a.shape[0], a.shape[1]
    sizes = np.full(B, nmax, dtype=np.int64) if sizes is None else _np(sizes).astype(np.int64)
    cnt, col, val, off = [], [], [], 0
    for b in range(B):
        s = int(sizes[b])
        for n in range(s):
            row = a[b, n, :s]
            j = np.nonzero(row != 0)[0]
            cnt.append(j.size)
            col.append(j + off)
            val.append(row[j])
        off += s
    cnt += [0] * int(n_ghost)
    col = np.concatenate(col).astype(np.int64) if col else np.zeros(0, np.int64)
    val = np.concatenate(val).astype(np.float32) if val else np.zeros(0, np.float32)
    return scan(cnt), col, val


def coo_to_csr(edge_index, n, n_ghost=0):
    """edge_index int64 [2, E] (row 0 source, row 1 target) -> (rowptr, col, eid): grouped by target, stable in the original edge order;
    eid[p] = the edge entry p came from"""
    ei = _np(edge_index).astype(np.int64).reshape(2, -1)
    eid = np.argsort(ei[1], kind="stable")
    rowptr = scan(np.bincount(ei[1], minlength=int(n) + int(n_ghost)))
    return rowptr, ei[0][eid], eid


def rows_of(rowptr):
    rp = _np(rowptr).astype(np.int64)
    return np.repeat(np.arange(rp.size - 1, dtype=np.int64), np.diff(rp))


def transpose(rowptr, col, val=None, n_cols=None):
    """-> (rowptr_t, col_t, val_t, src_e): the CSR of A^T, every transposed row ordered by (source row, source entry); src_e[p] = the entry
    of A that transposed entry p came from, val_t = val[src_e] (None when val is None)"""
    rp = _np(rowptr).astype(np.int64)
    nnz = int(rp[-1])
    col = _np(col).astype(np.int64)[:nnz]
    n_cols = rp.size - 1 if n_cols is None else int(n_cols)
    src_e = np.argsort(col, kind="stable")                  # entries ascend with their row: stable by column = (column, row, entry)
    rowptr_t = scan(np.bincount(col, minlength=n_cols))
    val_t = None if val is None else _np(val)[:nnz][src_e]
    return rowptr_t, rows_of(rp)[src_e], val_t, src_e


def ell_width(rowptr):
    rp = _np(rowptr).astype(np.int64)
    m = int(np.diff(rp).max()) if rp.size > 1 else 0
    return 4 if m <= 4 else (8 if m <= 8 else 16)


def to_ell(rowptr, col, W):
    """-> (table int64 [n, W], tail_ptr, tail_col): the first W entries of every row, -1 behind them; the entries beyond W as a CSR"""
    rp = _np(rowptr).astype(np.int64)
    col = _np(col).astype(np.int64)
    n = rp.size - 1
    table = np.full((n, W), -1, dtype=np.int64)
    tcnt, tcol = np.zeros(n, dtype=np.int64), []
    for r in range(n):
        c = col[rp[r]:rp[r + 1]]
        table[r, :min(W, c.size)] = c[:W]
        tcnt[r] = max(c.size - W, 0)
        tcol.append(c[W:])
    return table, scan(tcnt), (np.concatenate(tcol) if tcol else np.zeros(0, np.int64))


def to_dense(rowptr, col, val=None, n_cols=None, dtype=D):
    """the matrix a CSR stands for, repeated entries added up"""
    rp = _np(rowptr).astype(np.int64)
    nnz = int(rp[-1])
    n = rp.size - 1
    A = torch.zeros(n, n if n_cols is None else int(n_cols), dtype=dtype)
    v = torch.ones(nnz, dtype=dtype) if val is None else torch.as_tensor(_np(val)[:nnz]).to(dtype)
    A.index_put_((torch.as_tensor(rows_of(rp)), _idx(col)[:nnz]), v, accumulate=True)
    return A


# ============================================================================= float operations
CHUNK_ENTRIES = 1 << 17                 # entries gathered at a time (x[col] of a chunk is [entries, feat])


def _row_chunks(rp, limit=None):
    """consecutive row ranges of at most `limit` entries each (one row at least)"""
    limit = CHUNK_ENTRIES if limit is None else limit
    n, r0 = rp.size - 1, 0
    while r0 < n:
        r1 = int(np.searchsorted(rp, rp[r0] + limit, side="right")) - 1
        r1 = min(max(r1, r0 + 1), n)
        yield r0, r1
        r0 = r1


def spmm(rowptr, col, val, x, self_w=None, self_scalar=0.0, relu_in=False, y0=None, dtype=D):
    """y[i] = sum_e val[e] * f(x[col[e]]) + (self_w[i] + self_scalar) * f(x[i]) (+ y0[i]) over the entries e of row i, f = relu when
    relu_in; val None: unit weights; y0: the prior content an accumulating launch adds to.  [n, feat] in `dtype`, in row chunks"""
    rp = _np(rowptr).astype(np.int64)
    n = rp.size - 1
    col = _idx(col)
    x = x.to(dtype)
    if relu_in:
        x = x.clamp_min(0)
    val = None if val is None else torch.as_tensor(_np(val)).to(dtype)
    y = torch.zeros(n, x.size(1), dtype=dtype)
    for r0, r1 in _row_chunks(rp):
        e0, e1 = int(rp[r0]), int(rp[r1])
        msg = x[col[e0:e1]]
        if val is not None:
            msg = msg * val[e0:e1, None]
        y[r0:r1].index_add_(0, torch.as_tensor(rows_of(rp[r0:r1 + 1])), msg)
    if self_w is not None or self_scalar != 0.0:
        s = torch.full((n,), float(self_scalar), dtype=dtype)
        if self_w is not None:
            s = torch.as_tensor(_np(self_w)).to(dtype)[:n] + s
        y = y + s[:, None] * x[:n]
    if y0 is not None:
        y = y + y0.to(dtype)
    return y


def gcn_norm(rowptr, col, val, self_fill, dtype=D):
    """-> (dinv, val_out, self_w) by the rules of gcn_deg_kernel / gcn_norm_kernel: deg_i = sum of row i's weights (unit when val is None)
    + self_fill unless the row holds an entry (i, i) — an existing self loop is kept (every one of them) and none is added, self_w_i = 0
    then —; dinv_i = deg_i^-1/2, 0 when deg_i <= 0; val_out[e] = dinv_i val[e] dinv[col[e]]; self_w_i = dinv_i^2 self_fill"""
    rp = _np(rowptr).astype(np.int64)
    n, nnz = rp.size - 1, int(rp[-1])
    col = _idx(col)[:nnz]
    rows = torch.as_tensor(rows_of(rp))
    v = torch.ones(nnz, dtype=dtype) if val is None else torch.as_tensor(_np(val)[:nnz]).to(dtype)
    has_self = torch.zeros(n, dtype=torch.bool)
    has_self[rows[col == rows]] = True
    fill = torch.where(has_self, torch.zeros(n, dtype=dtype), torch.full((n,), float(self_fill), dtype=dtype))
    deg = torch.zeros(n, dtype=dtype).index_add_(0, rows, v) + fill
    dinv = torch.where(deg > 0, 1.0 / deg.clamp_min(1e-300 if dtype == D else 1e-38).sqrt(), torch.zeros(n, dtype=dtype))
    return dinv, dinv[rows] * v * dinv[col], dinv * dinv * fill


def sddmm(rowptr, col, dy, x, dtype=D):
    """gradient of spmm with respect to its weights: dval[e] = <dy[i], x[col[e]]> for the entries e of row i, dself[i] = <dy[i], x[i]>"""
    rp = _np(rowptr).astype(np.int64)
    n, nnz = rp.size - 1, int(rp[-1])
    col = _idx(col)[:nnz]
    rows = torch.as_tensor(rows_of(rp))
    dy, x = dy.to(dtype), x.to(dtype)
    return (dy[rows] * x[col]).sum(1), (dy[:n] * x[:n]).sum(1)
