"""The graph builders (csrc/graph_build.hip) and the CSR / ELL aggregation kernels (csrc/aggregate.hip) one by one through their C entry
points, and through GraphBatch / mp.spmm_ell where the Python wrapper is itself under test, against tests/graph_agg_ref.py.

Integer outputs (scan, row maps, dense -> CSR, COO -> CSR, transpose, CSR -> ELL + tail) are compared entry for entry.  Float outputs are
held to the rule of tests/fp32_yardstick.py at K = 8: the yardstick is graph_agg_ref's own float32 run on the CPU, never the kernel.
Every float output of a raw launch lives in guard_buf.Out (one NaN bit pattern, a leading dimension wider than the row where the entry
point takes one, guard words behind), every integer output in IntOut (IPAT, guard words behind); after a launch everything outside the
launch's own elements is bit for bit what was put there and no owned element still holds the pattern.  Every cell is launched twice into
equally prepared buffers and the two results are compared bit for bit (aggregate.hip: "no atomics: bitwise reproducible"; the COO and
transpose builders place with an atomic cursor and then sort).  The dispatched kernel (nat.last_kernel()) is asserted per cell.

Worst  max|hip - ref64| / yardstick  per kernel over this module (bound 8; each test prints its own), measured on an MI355X:
    spmv_rows       1.56  (1 block, weighted, relu_in, self_w, accumulate)
    spmm_scalar     1.74  (feat 8 with ldx 9, and the same cell with x one float off its boundary; 9 blocks, weighted, relu_in, self_w,
                           accumulate)       feat 3: 1.52   65: 1.28   89: 1.30   130: 1.14
    spmm_vec4<4>    1.65  (feat 16, 9 blocks, weighted, self_w + self_scalar, accumulate)
    spmm_vec4<8>    1.34  (feat 32, 1 block, weighted, relu_in, self_w + self_scalar, accumulate)
    spmm_vec4<16>   1.78  (feat 64, 9 blocks, weighted, relu_in, self_w + self_scalar, accumulate)
    spmm_vec4<32>   1.50  (feat 68, 17 blocks, weighted, no self term)
    spmm_vec4<64>   1.48  (feat 256, 9 blocks, weighted, relu_in, self_scalar, accumulate)      260: 1.25   320: 1.30 (two chunks)
    spmm_vec4_rb    0.91  <16,4,true> (feat 36)      1.00  <32,4,false> (feat 68)
    spmm_ell_vec4   1.00  <16,8> (feat 64, self_scalar 1); the other eight instantiations 0.56 .. 0.95      mp.spmm_ell  0.90 (feat 68)
    gcn_norm        1.00  (weighted, self_fill 1: self_w; self_fill 2: val_out)
    sddmm_rows      1.02  (feat 1000, dself)
Every worst cell of the CSR kernels is a weighted one: the kernels fuse weight x feature into one fma per entry where the float32
reference rounds the product and the sum separately; the unit-weight cells stayed at or below 1.19.  No cell exceeded 8, every integer output was
exact, no launch wrote outside its own elements, and every cell was bit-identical across its two launches.

The id checks of from_edge_index: on the sources before this module, `source -1`, `source N` and `source 2^32 + 3` did not raise (the
source row of edge_index was stored unchecked, 2^32 + 3 narrowed to node 3); `target -1` and `target N` always did.
"""
import numpy as np
import pytest
import torch

import graph_agg_ref as R
from fp32_yardstick import _check
from guard_buf import GUARD, Out

pytestmark = pytest.mark.gpu

EINVAL, EUNSUPPORTED = -1, -3
IPAT = -7
D, S32 = torch.float64, torch.float32
RB_MIN_ROWS = 262144                       # csrc/aggregate.hip: the row-batched gather exists from this many rows on


def _nat():
    from two_stage_gnn_amd import _native as nat
    return nat


def _GB():
    from two_stage_gnn_amd.graph import GraphBatch
    return GraphBatch


def _rc(name, *args):
    """the entry point's return code (call() raises on anything but 0)"""
    nat = _nat()
    return getattr(nat.lib(), "tsgnn_" + name)(*[nat._arg(a) for a in args], nat.stream_handle())


def _i32(a):
    return torch.as_tensor(np.asarray(a).astype(np.int32)).cuda()


def _f32(a):
    return torch.as_tensor(np.asarray(a)).to(S32).cuda()


def _strided(t, ld, lead=0):
    """an INPUT [rows, ld] on the device: t in the first columns, NaN in the padding; lead: floats in front of it (lead = 1 makes the
    pointer 4 bytes off a 16-byte boundary)"""
    rows = t.size(0)
    flat = torch.full((lead + rows * ld + 3,), float("nan"), dtype=S32)
    body = flat[lead:lead + rows * ld].view(rows, ld)
    body[:, :t.size(1)] = t
    dev = flat.cuda()
    return dev[lead:lead + rows * ld].view(rows, ld)


class IntOut:
    """n int32 on the device, every word IPAT, GUARD words behind"""

    def __init__(self, n):
        self.n = int(n)
        self.buf = torch.full((self.n + GUARD,), IPAT, dtype=torch.int32, device="cuda")
        self.t = self.buf[:self.n]

    def get(self, what, owned=None):
        """the body on the CPU; the guard words, and the body beyond the first `owned` words, must still hold IPAT"""
        torch.cuda.synchronize()
        b = self.buf.cpu()
        assert bool((b[self.n:] == IPAT).all()), "%s: guard words overwritten" % what
        if owned is not None:
            assert bool((b[owned:self.n] == IPAT).all()), "%s: written beyond its %d own words" % (what, owned)
            return b[:owned].long().numpy()
        return b[:self.n].long().numpy()


class Worst:
    """the worst ratio per kernel a test saw; printed at its end"""

    def __init__(self):
        self.w = {}

    def check(self, kernel, what, hip, r64, r32):
        r = _check("%s %s" % (kernel, what), hip, r64, r32, K=8)
        if r >= self.w.get(kernel, (-1.0, ""))[0]:
            self.w[kernel] = (r, what)
        return r

    def report(self):
        for k, (r, what) in sorted(self.w.items()):
            print("WORST %s: %.3f (%s)" % (k, r, what))


def _same(a, b, what):
    assert torch.equal(a.cpu(), b.cpu()), "%s: two launches differ" % what


def _eq(got, want, what):
    np.testing.assert_array_equal(np.asarray(got).astype(np.int64), np.asarray(want).astype(np.int64), err_msg=what)


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def _tf(b):
    return "true" if b else "false"


def _cols(rows, ld, feat):
    m = torch.zeros(rows, ld, dtype=torch.bool)
    m[:, :feat] = True
    return m


# ============================================================================= builders (exact)
@pytest.mark.parametrize("n", [0, 1, 7, 2047, 2048, 2049, 100003, 256 * 2048, 256 * 2048 + 1, 1 << 21])
def test_exclusive_scan(n):
    """one tile / two tiles (2048 items each), and 256 / 257 tile sums: phase 2 scans the tile sums 256 at a time with a carry"""
    from two_stage_gnn_amd.graph import _scan_ws
    nat = _nat()
    c = torch.randint(0, 9, (n,), dtype=torch.int32, generator=torch.Generator().manual_seed(n))
    want = R.scan(c)
    cd = c.cuda()
    outs = []
    for _ in range(2):
        O = IntOut(n + 1)
        ws = _scan_ws(n, "cuda")
        nat.call("exclusive_scan_i32", cd, n, O.t, ws)
        outs.append(O.get("scan n=%d" % n))
        _eq(outs[-1], want, "scan n=%d" % n)
    _eq(outs[0], outs[1], "scan twice")
    assert torch.equal(cd.cpu(), c)


ROW_MAP_SIZES = [[5], [0, 3, 0, 0, 2, 1, 0], [0, 0, 4], [4, 0, 0], [1] * 9, [100, 0, 155], [100, 0, 156], [1, 256, 0], [0]]


@pytest.mark.parametrize("sizes", ROW_MAP_SIZES, ids=lambda s: "x".join(map(str, s[:4])) + "_%d" % len(s))
def test_row_maps(sizes):
    """one graph; empty graphs first, in the middle, last, two in a row; graphs of one row; 255, 256, 257 rows (one 256-thread block and
    one row more); no row at all (nothing is launched, nothing is written)"""
    nat = _nat()
    gp = R.scan(sizes)
    n = int(gp[-1])
    rg, rs = R.row_maps(gp, n)
    res = []
    for _ in range(2):
        G, S = IntOut(n + 3), IntOut(n + 3)
        nat.call("row_maps", _i32(gp), len(sizes), n, G.t, S.t)
        res.append((G.get("row_graph", owned=n), S.get("row_slot", owned=n)))
        _eq(res[-1][0], rg, "row_graph")
        _eq(res[-1][1], rs, "row_slot")
    _eq(res[0][0], res[1][0], "twice")
    G = IntOut(n)                                           # either map alone
    nat.call("row_maps", _i32(gp), len(sizes), n, G.t, None)
    _eq(G.get("row_graph alone"), rg, "row_graph alone")


def _dense_case(nmax, seed):
    """[6, nmax, nmax] weighted (negatives too), asymmetric: graph sizes 0, 1, nmax, about half, nmax - 1, 0; graph 2's last row full
    but for one -0.0, graph 3's first row all zero with one -0.0"""
    g = torch.Generator().manual_seed(seed)
    sizes = np.array([0, 1, nmax, max(1, nmax // 2), nmax - 1, 0], dtype=np.int64)
    adj = torch.randn(6, nmax, nmax, generator=g) * (torch.rand(6, nmax, nmax, generator=g) < 0.3)
    adj[2, nmax - 1] = torch.where(adj[2, nmax - 1] == 0, torch.full((nmax,), 1.5), adj[2, nmax - 1])
    if nmax >= 3:
        adj[2, nmax - 1, nmax // 2] = -0.0
    adj[3, 0] = 0
    adj[3, 0, 0] = -0.0
    return adj, sizes


def _check_graph(g, rp, col, val, sizes, nmax, what):
    """every field of a GraphBatch against the reference CSR (rp over all rows, the empty ghost rows included)"""
    n = int(np.sum(sizes))
    assert g.n_rows == n and g.total_rows == rp.size - 1 and g.nnz == rp[-1], what
    _eq(g.rowptr.cpu().numpy(), rp, what + " rowptr")
    assert (rp[n:] == rp[-1]).all()                          # (the reference's ghost rows are empty; the kernel's equal them above)
    _eq(g.col.cpu().numpy()[:g.nnz], col, what + " col")
    if val is not None:
        _eq(_bits(g.val[:g.nnz]).numpy(), val.astype(np.float32).view(np.int32), what + " val bits")
    else:
        assert g.val is None
    gp = R.scan(sizes)
    rg, rs = R.row_maps(gp, n)
    _eq(g.graph_ptr.cpu().numpy(), gp, what + " graph_ptr")
    _eq(g.row_graph.cpu().numpy()[:n], rg, what + " row_graph")
    _eq(g.row_slot.cpu().numpy()[:n], rs, what + " row_slot")
    _eq(g.slot_count.cpu().numpy(), [(np.asarray(sizes) > k).sum() for k in range(nmax)], what + " slot_count")


def _dense_raw(adj_d, g, rp, col, val, what):
    """the two launches of from_dense once more into guarded buffers"""
    nat = _nat()
    B, nmax, n, nnz = adj_d.size(0), adj_d.size(1), g.n_rows, int(rp[-1])
    C = IntOut(g.total_rows)
    nat.call("dense_adj_count", adj_d, B, nmax, g.graph_ptr, g.row_graph, n, C.t)
    _eq(C.get(what + " row_cnt", owned=n), np.diff(rp)[:n], what + " row_cnt")
    CO, V = IntOut(nnz + 5), Out(1, nnz + 5)
    nat.call("dense_adj_fill", adj_d, B, nmax, g.graph_ptr, g.row_graph, n, _i32(rp), CO.t, V.mat)
    _eq(CO.get(what + " col", owned=nnz), col, what + " col (raw)")
    own = torch.zeros(1, nnz + 5, dtype=torch.bool)
    own[0, :nnz] = True
    V.rest_untouched(what + " val", own)
    _eq(_bits(V.mat[0, :nnz]).numpy(), val.astype(np.float32).view(np.int32), what + " val bits (raw)")


@pytest.mark.parametrize("layout", ["packed", "padded"])
@pytest.mark.parametrize("nmax", [1, 63, 64, 65, 129])
def test_from_dense(nmax, layout):
    """a row of 63 / 64 / 65 / 129 columns: under, at and over one 64-lane ballot, and three ballots"""
    GB = _GB()
    adj, sizes = _dense_case(nmax, 100 + nmax)
    packed = layout == "packed"
    rp, col, val = R.dense_to_csr(adj.numpy(), sizes if packed else None, n_ghost=nmax if packed else 0)
    szs = sizes if packed else np.full(6, nmax, dtype=np.int64)
    if nmax >= 3:
        assert np.diff(rp).max() == nmax - 1                 # the full row, less its -0.0
    adj_d = adj.cuda()
    g = GB.from_dense(adj_d, sizes if packed else None, layout=layout)
    assert g.n_ghost == (nmax if packed else 0) and g.val is not None
    _check_graph(g, rp, col, val, szs, nmax, "from_dense %s nmax %d" % (layout, nmax))
    g2 = GB.from_dense(adj_d, sizes if packed else None, layout=layout)
    for a, b in ((g.rowptr, g2.rowptr), (g.col[:g.nnz], g2.col[:g.nnz]), (_bits(g.val[:g.nnz]), _bits(g2.val[:g.nnz]))):
        _same(a, b, "from_dense")
    _dense_raw(adj_d, g, rp, col, val, "dense %s nmax %d" % (layout, nmax))
    if packed:                                               # only adj[b, :n_b, :n_b] is read
        bad = adj.clone()
        for b in range(6):
            bad[b, int(sizes[b]):, :] = float("nan")
            bad[b, :, int(sizes[b]):] = float("nan")
        g3 = GB.from_dense(bad.cuda(), sizes, layout="packed")
        _check_graph(g3, rp, col, val, szs, nmax, "from_dense, NaN outside [:n_b, :n_b]")


@pytest.mark.parametrize("layout", ["packed", "padded"])
def test_from_dense_all_zero(layout):
    GB = _GB()
    adj = torch.zeros(3, 65, 65)
    adj[1, 3, 4] = -0.0
    sizes = np.array([65, 0, 7])
    packed = layout == "packed"
    rp, col, val = R.dense_to_csr(adj.numpy(), sizes if packed else None, n_ghost=65 if packed else 0)
    assert rp[-1] == 0
    g = GB.from_dense(adj.cuda(), sizes if packed else None, layout=layout)
    _check_graph(g, rp, col, val, sizes if packed else np.full(3, 65), 65, "all-zero batch")
    _dense_raw(adj.cuda(), g, rp, col, val, "all-zero batch")
    rpt, colt, valt = g.transposed()                         # nnz 0, weights given
    _eq(rpt.cpu().numpy(), rp, "transpose of nothing")
    rpt, colt, src = g.transpose_map()
    _eq(rpt.cpu().numpy(), rp, "transpose_map of nothing")


def _edge_case(name):
    """(edge_index int64 [2, E], N, sizes or None, nmax or None)"""
    g = torch.Generator().manual_seed(sum(map(ord, name)))

    def rnd(N, E):
        src = torch.randint(0, N, (E,), generator=g)
        dst = torch.randint(0, N, (E,), generator=g)
        if N > 8:
            dst[dst == 3] = 4                                # node 3 (and whatever the draw missed) has no in-edge
            dst[dst == N - 1] = 0
        return torch.stack([src, dst])
    if name == "E0":
        return torch.zeros(2, 0, dtype=torch.int64), 10, None, None
    if name == "E1":
        return torch.tensor([[4], [4]]), 10, None, None      # one self loop
    if name.startswith("E"):
        E = int(name[1:])
        ei = rnd(300, E)
        ei[:, 7:17] = ei[:, 20:30]                           # repeated edges
        ei[1, 40:50] = ei[0, 40:50]                          # self loops
        return ei, 300, None, None
    if name.startswith("N"):
        N = int(name[1:])
        ei = rnd(N, 900)
        ei[:, 0:30] = ei[:, 100:130]
        ei[1, 40:50] = ei[0, 40:50]
        return ei, N, None, None
    if name == "hub":                                        # one target with 1000 in-edges: the per-row insertion sort
        ei = rnd(64, 200)
        hub = torch.stack([torch.randint(0, 64, (1000,), generator=g), torch.full((1000,), 7)])
        ei = torch.cat([ei[:, :100], hub, ei[:, 100:]], 1)
        return ei[:, torch.randperm(ei.size(1), generator=g)], 64, None, None
    if name == "ghosts":
        return rnd(10, 40), 10, np.array([3, 0, 4, 3]), 5
    raise KeyError(name)


@pytest.mark.parametrize("name", ["E0", "E1", "E255", "E256", "E257", "N255", "N256", "N257", "hub", "ghosts"])
def test_from_edge_index(name):
    GB, nat = _GB(), _nat()
    ei, N, sizes, nmax = _edge_case(name)
    E = ei.size(1)
    n_ghost = nmax or 0
    rp, col, eid = R.coo_to_csr(ei, N, n_ghost=n_ghost)
    if name == "hub":
        assert np.diff(rp).max() >= 1000
    ei_d = ei.cuda()
    kw = dict(sizes=sizes, nmax=nmax, ghosts=True) if sizes is not None else {}
    gs = [GB.from_edge_index(ei_d, N, **kw) for _ in range(2)]
    for g in gs:
        assert g.total_rows == N + n_ghost and g.nnz == E and g.val is None
        _eq(g.rowptr.cpu().numpy(), rp, name + " rowptr")
        _eq(g.col.cpu().numpy()[:E], col, name + " col")
        _eq(g.eid.cpu().numpy()[:E], eid, name + " eid")
    if sizes is not None:
        _check_graph(gs[0], rp, col, None, sizes, nmax, name)
    # the two launches once more into guarded buffers
    C, F = IntOut(N + n_ghost), IntOut(1)
    nat.call("coo_count", ei_d[1].contiguous(), E, N, C.t, F.t)
    _eq(C.get(name + " cnt", owned=N), np.diff(rp)[:N], name + " cnt")
    assert F.get(name + " flag")[0] == 0
    CO, EI = IntOut(E + 5), IntOut(E + 5)
    nat.call("coo_fill", ei_d[1].contiguous(), ei_d[0].contiguous(), E, N, N, _i32(rp), torch.empty(max(N, 1), dtype=torch.int32,
             device="cuda"), CO.t, EI.t, F.t)
    _eq(CO.get(name + " col", owned=E), col, name + " col (raw)")
    _eq(EI.get(name + " eid", owned=E), eid, name + " eid (raw)")
    assert F.get(name + " flag")[0] == 0                     # in-range ids leave the flag alone
    assert torch.equal(ei_d.cpu(), ei)


BAD_IDS = {"target -1": [[0, 1], [1, -1]], "target N": [[0, 1], [1, 10]], "source -1": [[0, -1], [1, 2]], "source N": [[0, 10], [1, 2]],
           "source 2^32 + 3": [[0, (1 << 32) + 3], [1, 2]]}


@pytest.mark.parametrize("name", list(BAD_IDS))
def test_from_edge_index_rejects_ids_outside_the_graph(name):
    """an id of EITHER row outside [0, num_nodes) raises: decided on the device from the int64 value, so 2^32 + 3 is not node 3.  Nothing
    consumes the graph afterwards."""
    with pytest.raises(IndexError):
        _GB().from_edge_index(torch.tensor(BAD_IDS[name], dtype=torch.int64).cuda(), 10)


def _multigraph(seed, n_real, n_total, E, weighted):
    """asymmetric CSR over n_total rows (the rows from n_real on empty): random entries, ten of them a second time (with another weight),
    rows 2 and n_real - 1 empty, columns 0 and 5 empty"""
    g = torch.Generator().manual_seed(seed)
    src = torch.randint(1, n_real, (E,), generator=g)
    dst = torch.randint(0, n_real - 1, (E,), generator=g)
    src[src == 5] = 6
    dst[dst == 2] = 3
    ei = torch.stack([src, dst])
    ei = torch.cat([ei, ei[:, :10]], 1)
    ei = ei[:, torch.randperm(ei.size(1), generator=g)]
    rp, col, eid = R.coo_to_csr(ei, n_total)
    val = torch.randn(ei.size(1), generator=g).numpy() if weighted else None
    return rp, col, val


@pytest.mark.parametrize("sizes,weighted", [((85, 85), True), ((84, 86), False), ((85, 86), True), ((3, 2), True)])
def test_transpose(sizes, weighted):
    """total_rows 255 / 256 / 257 (and 10): rowptr_t, col_t, val_t and the src_e pairing edge-softmax relies on"""
    GB, nat = _GB(), _nat()
    nmax, n_real = max(sizes), sum(sizes)
    total = n_real + nmax
    rp, col, val = _multigraph(total, n_real, total, 6 * n_real, weighted)
    nnz = int(rp[-1])
    rows = R.rows_of(rp)
    pair = rows * total + col
    assert np.unique(pair).size < nnz                        # the same (row, col) more than once
    rpt, colt, valt, src_e = R.transpose(rp, col, val)
    gs = []
    for _ in range(2):
        g = GB.from_csr(_i32(rp), _i32(col), _f32(val) if weighted else None, np.array(sizes), nmax, assume_symmetric=False)
        assert g.total_rows == total
        a, b, s = g.transpose_map()
        _eq(a.cpu().numpy(), rpt, "rowptr_t")
        _eq(b.cpu().numpy()[:nnz], colt, "col_t")
        _eq(s.cpu().numpy()[:nnz], src_e, "src_e_t")
        t = g.transposed()
        assert t[0] is a and t[1] is b
        if weighted:
            _eq(_bits(t[2][:nnz]).numpy(), valt.astype(np.float32).view(np.int32), "val_t")
        else:
            assert t[2] is None
        other = torch.randn(nnz, generator=torch.Generator().manual_seed(1))
        t2 = g.transposed(val=other.cuda())                  # other weights go through the same pairing
        _eq(_bits(t2[2]).numpy(), other.numpy()[src_e].view(np.int32), "transposed(val=other)")
        assert g.transposed(val=None)[2] is None
        gs.append(g)
    _same(gs[0].src_e_t, gs[1].src_e_t, "transpose")
    # the launch once more into guarded buffers
    from two_stage_gnn_amd.graph import _scan_ws
    RT, CT, SE, VT = IntOut(total + 1), IntOut(nnz + 5), IntOut(nnz + 5), Out(1, nnz + 5)
    nat.call("csr_transpose", _i32(rp), _i32(col), _f32(val) if weighted else None, total, total, nnz, RT.t, CT.t,
             VT.mat if weighted else None, SE.t, torch.empty(total, dtype=torch.int32, device="cuda"), _scan_ws(total, "cuda"))
    _eq(RT.get("rowptr_t"), rpt, "rowptr_t (raw)")
    _eq(CT.get("col_t", owned=nnz), colt, "col_t (raw)")
    _eq(SE.get("src_e", owned=nnz), src_e, "src_e (raw)")
    own = torch.zeros(1, nnz + 5, dtype=torch.bool)
    own[0, :nnz] = weighted
    VT.rest_untouched("val_t", own)
    if weighted:
        _eq(_bits(VT.mat[0, :nnz]).numpy(), valt.astype(np.float32).view(np.int32), "val_t (raw)")


def test_transpose_of_no_entries():
    g = _GB().from_edge_index(torch.zeros(2, 0, dtype=torch.int64).cuda(), 10)
    rpt, colt, src = g.transpose_map()
    _eq(rpt.cpu().numpy(), np.zeros(11), "rowptr_t")
    assert g.transposed()[2] is None


def _degree_graph(maxdeg, n, seed):
    """CSR over n rows + n empty ghost rows whose largest degree is exactly maxdeg: degrees cycle through 0 .. maxdeg's neighbours"""
    cyc = sorted({0, 1, 3, 4, 5, 8, 9, 16, 17, maxdeg})
    deg = np.array([d for d in cyc if d <= maxdeg] * n)[:n]
    deg[n // 2] = maxdeg
    deg = np.concatenate([deg, np.zeros(n, dtype=deg.dtype)])
    rp = R.scan(deg)
    col = np.random.default_rng(seed).integers(0, n, int(rp[-1]))
    return rp, col


@pytest.mark.parametrize("maxdeg", [0, 4, 5, 8, 9, 16, 17, 40])
def test_ell(maxdeg):
    """a largest degree at and one past every table width: the chosen W, the table with its -1 entries and ghost rows, the tail CSR"""
    GB, nat = _GB(), _nat()
    n = 37
    rp, col = _degree_graph(maxdeg, n, maxdeg)
    W = R.ell_width(rp)
    assert W == (4 if maxdeg <= 4 else 8 if maxdeg <= 8 else 16)
    table, tp, tc = R.to_ell(rp, col, W)
    for _ in range(2):
        g = GB.from_csr(_i32(rp), _i32(col), None, np.array([n]), n)
        ell, w, tail = g.ell()
        assert w == W and g.ell() is g._ell
        _eq(ell.cpu().numpy()[:2 * n * W].reshape(2 * n, W), table, "table")
        if maxdeg > W:
            _eq(tail[0].cpu().numpy(), tp, "tail_ptr")
            _eq(tail[1].cpu().numpy()[:tp[-1]], tc, "tail_col")
        else:
            assert tail is None and tp[-1] == 0
    g.val = torch.ones(1, device="cuda")
    g._ell = None
    assert g.ell() is None                                   # weighted graphs have no table
    # the launches once more into guarded buffers, only the first n + 3 rows: the table and the counts beyond them stay untouched
    m = n + 3
    T, C = IntOut(2 * n * W), IntOut(2 * n)
    nat.call("csr_to_ell", _i32(rp), _i32(col), m, W, T.t, C.t)
    _eq(T.get("table", owned=m * W).reshape(m, W), table[:m], "table (raw)")
    _eq(C.get("tail_cnt", owned=m), np.diff(tp)[:m], "tail_cnt")
    if tp[-1]:
        TC = IntOut(int(tp[-1]) + 5)
        nat.call("csr_tail_fill", _i32(rp), _i32(col), _i32(tp), m, W, TC.t)
        _eq(TC.get("tail_col", owned=int(tp[m])), tc[:tp[m]], "tail_col (raw)")


def test_entry_checks_without_a_launch():
    rp, col = _degree_graph(4, 8, 0)
    rpd, cold = _i32(rp), _i32(col)
    T = IntOut(16 * 8)
    assert _rc("csr_to_ell", rpd, cold, 16, 5, T.t, None) == EINVAL
    assert (T.get("table") == IPAT).all()
    for feat in (260, 6):
        x, Y = torch.zeros(16, 264, device="cuda"), Out(16, 264)
        ell = torch.full((16 * 4,), -1, dtype=torch.int32, device="cuda")
        assert _rc("ell_spmm_f32", ell, 4, x, 264, Y.mat, 264, 16, feat, 0.0) == EUNSUPPORTED
        Y.rest_untouched("ell_spmm feat %d" % feat, torch.zeros(16, 264, dtype=torch.bool))
    x, DV, DS = torch.zeros(16, 1028, device="cuda"), Out(1, int(rp[-1])), Out(1, 16)
    assert _rc("sddmm_rows_f32", rpd, cold, x, 1028, x, 1028, 16, 1025, DV.mat, DS.mat) == EUNSUPPORTED
    DV.rest_untouched("sddmm dval", torch.zeros(1, int(rp[-1]), dtype=torch.bool))
    DS.rest_untouched("sddmm dself", torch.zeros(1, 16, dtype=torch.bool))


# ============================================================================= tsgnn_csr_spmm_f32
def _group(feat, vec):
    """lanes per row of the kernel a cell reaches: spmm_vec4<G> by feat / 4; the scalar kernel fetches 64 entries at a time"""
    if not vec:
        return 64
    nvec = feat // 4
    return 4 if nvec <= 4 else 8 if nvec <= 8 else 16 if nvec <= 16 else 32 if nvec <= 32 else 64


def _family(G, n, seed, shift=0):
    """CSR over n rows, the last three of them ghost rows (no entry); row degrees 0, 1, 3, 4, 5, G - 1, G, G + 1, 2G + 3 and 200 in turn;
    columns anywhere in [0, n), weights normal"""
    DEG = [0, 1, 3, 4, 5, G - 1, G, G + 1, 2 * G + 3, 200]
    deg = np.array([DEG[(3 * r + shift) % 10] for r in range(n)])
    deg[max(n - 3, 1):] = 0
    rp = R.scan(deg)
    rng = np.random.default_rng(seed)
    col = rng.integers(0, n, int(rp[-1]))
    val = rng.standard_normal(int(rp[-1])).astype(np.float32)
    return rp, col, val, set(deg.tolist()) >= set(DEG)


def _features(n, feat, seed):
    """normal, with exact zeros and -0.0 (what relu_in must both turn into +0 contributions)"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, feat, generator=g)
    u = torch.rand(n, feat, generator=g)
    x[u < 0.1] = 0.0
    x[u > 0.92] = -0.0
    return x


# (feat, ldx, ldy, lead, kernel): lead = 1 puts x one float off its 16-byte boundary.  Which kernel a cell reaches follows
# tsgnn_csr_spmm_f32's dispatch — feat 1: spmv_rows; feat, ldx, ldy multiples of 4 and x, y 16-byte aligned: spmm_vec4<G>; else
# spmm_scalar — and is asserted from nat.last_kernel().
SPMM_CELLS = [(1, 3, 2, 0, "spmv_rows"),
              (3, 5, 6, 0, "spmm_scalar"), (65, 67, 68, 0, "spmm_scalar"), (89, 92, 90, 0, "spmm_scalar"), (130, 132, 133, 0, "spmm_scalar"),
              (8, 9, 12, 0, "spmm_scalar"), (8, 8, 12, 1, "spmm_scalar")] + \
             [(f, f + 8, f + 4, 0, "spmm_vec4") for f in (4, 8, 16, 20, 32, 36, 64, 68, 128, 132, 256, 260, 320)]
SELF_KINDS = ("none", "scalar", "w", "both")


@pytest.mark.parametrize("feat,ldx,ldy,lead,kernel", SPMM_CELLS, ids=lambda v: str(v))
def test_csr_spmm(feat, ldx, ldy, lead, kernel):
    """every flag combination (weights x relu_in x self term x accumulate) at 1, 7, 8, 9 and 17 blocks: xcd_remap is a permutation of the
    blocks iff every row is written exactly once — a row it skipped still holds the pattern, a row it hit twice is another one skipped"""
    nat = _nat()
    vec = kernel == "spmm_vec4"
    G = _group(feat, vec) if kernel != "spmv_rows" else 4
    rpb = 256 if kernel == "spmv_rows" else 4 if not vec else 256 // G
    worst = Worst()
    for nb in (1, 7, 8, 9, 17):
        n = (nb - 1) * rpb + (rpb + 1) // 2
        assert -(-n // rpb) == nb
        rp, col, val, all_degrees = _family(G, n, 1000 * feat + nb, shift=nb)
        assert all_degrees or nb < 17 or rpb < 2
        x = _features(n, feat, 7 * feat + nb)
        xd = _strided(x, ldx, lead)
        assert (xd.data_ptr() % 16 == 0) == (lead == 0)
        g = torch.Generator().manual_seed(nb)
        self_w = torch.randn(n, generator=g)
        y0 = torch.randn(n, feat, generator=g)
        rpd, cold, vald, swd = _i32(rp), _i32(col), _f32(val), self_w.cuda()
        own = _cols(n, ldy, feat)
        for weighted in (False, True):
            for relu in (0, 1):
                for kind in SELF_KINDS:
                    sw = self_w if kind in ("w", "both") else None
                    sc = 0.75 if kind in ("scalar", "both") else 0.0
                    for acc in (0, 1):
                        what = "feat %d ld %d/%d lead %d blocks %d w%d relu%d self %s acc%d" % (feat, ldx, ldy, lead, nb, weighted, relu,
                                                                                              kind, acc)
                        outs = []
                        for _ in range(2):
                            Y = Out(n, ldy)
                            if acc:
                                Y.mat[:, :feat] = y0.cuda()
                            nat.call("csr_spmm_f32", rpd, cold, vald if weighted else None, swd if sw is not None else None, xd, ldx,
                                     Y.mat, ldy, n, feat, sc, relu, acc)
                            name = nat.last_kernel()
                            Y.rest_untouched(what, own)
                            outs.append(Y)
                        want = {"spmv_rows": "spmv_rows<%s>" % _tf(weighted), "spmm_scalar": "spmm_scalar<%s,%s>" % (_tf(weighted), _tf(relu)),
                                "spmm_vec4": "spmm_vec4<%d,%s,%s>" % (G, _tf(weighted), _tf(relu))}[kernel]
                        assert name == want, (what, name)
                        assert torch.equal(outs[0].bits, outs[1].bits), what + ": two launches differ"
                        args = (rp, col, val if weighted else None, x)
                        kw = dict(self_w=sw, self_scalar=sc, relu_in=bool(relu), y0=y0 if acc else None)
                        worst.check(want.split("<")[0] + ("<%d>" % G if vec else ""), what, outs[0].mat[:, :feat], R.spmm(*args, dtype=D, **kw),
                                    R.spmm(*args, dtype=S32, **kw))
    worst.report()


@pytest.mark.parametrize("feat,weighted,G", [(36, True, 16), (68, False, 32)])
def test_csr_spmm_row_batched(feat, weighted, G):
    """the row-batched kernel at its smallest shape, 262,144 + 3 rows: mean degree 5, every 500th group of four rows with more than G
    neighbours in total (a second index fetch), self term and accumulate; feat 36 leaves lanes of a 16-lane group idle"""
    nat = _nat()
    n = RB_MIN_ROWS + 3
    rng = np.random.default_rng(feat)
    deg = rng.integers(0, 11, n)
    deg[4 * 500 * np.arange(n // 2000) + 1] = G + 9
    deg[4 * 500 * np.arange(n // 2000) + 2] = 12
    deg[-2:] = 0
    rp = R.scan(deg)
    four = np.add.reduceat(deg[:n - n % 4], np.arange(0, n - n % 4, 4))
    assert (four > G).sum() >= 100 and abs(deg.mean() - 5) < 0.2
    nnz = int(rp[-1])
    col = rng.integers(0, n, nnz)
    val = rng.standard_normal(nnz).astype(np.float32) if weighted else None
    g = torch.Generator().manual_seed(feat)
    x = torch.randn(n, feat, generator=g)
    self_w = torch.randn(n, generator=g)
    y0 = torch.randn(n, feat, generator=g)
    ldx, ldy = feat + 8, feat + 4
    xd, rpd, cold, swd = _strided(x, ldx), _i32(rp), _i32(col), self_w.cuda()
    vald = _f32(val) if weighted else None
    own = _cols(n, ldy, feat)
    outs = []
    for _ in range(2):
        Y = Out(n, ldy)
        Y.mat[:, :feat] = y0.cuda()
        nat.call("csr_spmm_f32", rpd, cold, vald, swd, xd, ldx, Y.mat, ldy, n, feat, 0.75, 0, 1)
        assert nat.last_kernel() == "spmm_vec4_rb<%d,4,%s>" % (G, "true" if weighted else "false")
        Y.rest_untouched("row-batched feat %d" % feat, own)
        outs.append(Y)
    assert torch.equal(outs[0].bits, outs[1].bits), "two launches differ"
    kw = dict(self_w=self_w, self_scalar=0.75, y0=y0)
    worst = Worst()
    worst.check("spmm_vec4_rb<%d>" % G, "feat %d weighted %d" % (feat, weighted), outs[0].mat[:, :feat], R.spmm(rp, col, val, x, dtype=D, **kw),
                R.spmm(rp, col, val, x, dtype=S32, **kw))
    worst.report()


# ============================================================================= tsgnn_ell_spmm_f32, mp.spmm_ell
@pytest.mark.parametrize("W", [4, 8, 16])
@pytest.mark.parametrize("feat", [4, 36, 64, 68, 128, 132, 256])
def test_ell_spmm(feat, W):
    """the nine instantiations (G 16 / 32 / 64 by feat, W 4 / 8 / 16): against float64, and bit for bit the CSR kernel's result (no row
    has a tail here); then a hand-made table with -1 in the MIDDLE of a row"""
    nat = _nat()
    G = 16 if feat <= 64 else 32 if feat <= 128 else 64
    n = 9 * (256 // G) - 1                                   # nine blocks, the last one short of a row
    deg = np.array([(7 * r) % (W + 1) for r in range(n)])
    deg[n - 3:] = 0
    rp = R.scan(deg)
    rng = np.random.default_rng(feat * W)
    col = rng.integers(0, n, int(rp[-1]))
    table, tp, tc = R.to_ell(rp, col, W)
    assert tp[-1] == 0 and deg.max() == W
    holes = table.copy()                                     # -1 in the middle: rows keep entries 0, 2, 3, 5, ...
    holes[:, 1::3] = -1
    hrp = R.scan((holes >= 0).sum(1))
    hcol = holes[holes >= 0]
    x = _features(n, feat, feat + W)
    ldx, ldy = feat + 8, feat + 4
    xd, rpd, cold = _strided(x, ldx), _i32(rp), _i32(col)
    own = _cols(n, ldy, feat)
    worst = Worst()
    for sc in (0.0, 1.0):
        for tname, tab, crp, ccol in (("table", table, rp, col), ("holes", holes, hrp, hcol)):
            what = "feat %d W %d self %g %s" % (feat, W, sc, tname)
            td = _i32(tab.reshape(-1))
            outs = []
            for _ in range(2):
                Y = Out(n, ldy)
                nat.call("ell_spmm_f32", td, W, xd, ldx, Y.mat, ldy, n, feat, sc)
                assert nat.last_kernel() == "spmm_ell_vec4<%d,%d>" % (G, W)
                Y.rest_untouched(what, own)
                outs.append(Y)
            assert torch.equal(outs[0].bits, outs[1].bits), what + ": two launches differ"
            worst.check("spmm_ell_vec4<%d,%d>" % (G, W), what, outs[0].mat[:, :feat], R.spmm(crp, ccol, None, x, self_scalar=sc, dtype=D),
                        R.spmm(crp, ccol, None, x, self_scalar=sc, dtype=S32))
            C = Out(n, ldy)                                  # "same summation order as the CSR kernel (bitwise equal)"
            nat.call("csr_spmm_f32", _i32(crp), _i32(ccol) if ccol.size else cold, None, None, xd, ldx, C.mat, ldy, n, feat, sc, 0, 0)
            assert nat.last_kernel().startswith("spmm_vec4<")
            assert torch.equal(C.bits, outs[0].bits), what + ": differs from the CSR kernel"
    worst.report()


@pytest.mark.parametrize("feat", [4, 68, 256])
def test_spmm_ell_with_tail(feat):
    """mp.spmm_ell on degrees up to 40: the W = 16 table, then the accumulating CSR launch over the tail"""
    from two_stage_gnn_amd import message_passing as mp
    n = 37
    rp, col = _degree_graph(40, n, feat)
    x = _features(2 * n, feat, feat)
    ldx, ldy = feat + 8, feat + 4
    xd = _strided(x, ldx)[:, :feat]                          # (the wrapper takes feat and the leading dimensions from the views)
    own = _cols(2 * n, ldy, feat)
    worst = Worst()
    for sc in (0.0, 1.0):
        outs = []
        for _ in range(2):
            g = _GB().from_csr(_i32(rp), _i32(col), None, np.array([n]), n)
            Y = Out(2 * n, ldy)
            yv = Y.mat[:, :feat]
            assert mp.spmm_ell(g, xd, sc, out=yv) is yv
            assert g.ell()[1] == 16 and g.ell()[2] is not None
            Y.rest_untouched("spmm_ell feat %d" % feat, own)
            outs.append(Y)
        assert torch.equal(outs[0].bits, outs[1].bits), "two launches differ"
        worst.check("mp.spmm_ell", "feat %d self %g" % (feat, sc), outs[0].mat[:, :feat], R.spmm(rp, col, None, x, self_scalar=sc, dtype=D),
                    R.spmm(rp, col, None, x, self_scalar=sc, dtype=S32))
        Y = Out(n + 1, ldy)                                  # rows=: only the first rows are produced
        mp.spmm_ell(g, xd, sc, out=Y.mat[:, :feat], rows=n - 2)
        o2 = _cols(n + 1, ldy, feat)
        o2[n - 2:] = False
        Y.rest_untouched("spmm_ell rows=", o2)
        assert torch.equal(_bits(Y.mat[:n - 2, :feat]), _bits(outs[0].mat[:n - 2, :feat]))
    worst.report()


# ============================================================================= tsgnn_gcn_norm_f32
def _gcn_graph(weighted):
    """600 rows (three blocks): random rows of positive weights; row 3 one self loop, row 4 two, row 5 isolated, row 6 one entry (a self
    loop) alone; weighted only: row 7 weights -3, 1 (sum -2: <= 0 even with a self loop of 2 added), row 8 weights 2, -2 on a self loop"""
    n = 600
    rng = np.random.default_rng(5 + weighted)
    rows = [rng.integers(9, n, rng.integers(1, 9)) for _ in range(n)]
    rows[3] = np.array([20, 3, 31])
    rows[4] = np.array([4, 40, 4, 41])
    rows[5] = np.zeros(0, dtype=np.int64)
    rows[6] = np.array([6])
    rows[7] = np.array([50, 51])
    rows[8] = np.array([8, 60])
    rp = R.scan([len(r) for r in rows])
    col = np.concatenate(rows)
    val = None
    if weighted:
        val = (rng.random(col.size) + 0.1).astype(np.float32)
        val[rp[7]:rp[8]] = (-3.0, 1.0)
        val[rp[8]:rp[9]] = (2.0, -2.0)
    return n, rp, col, val


@pytest.mark.parametrize("self_fill", [0.0, 1.0, 2.0])
@pytest.mark.parametrize("weighted", [False, True])
def test_gcn_norm(weighted, self_fill):
    nat = _nat()
    n, rp, col, val = _gcn_graph(weighted)
    nnz = int(rp[-1])
    r64, r32 = R.gcn_norm(rp, col, val, self_fill, dtype=D), R.gcn_norm(rp, col, val, self_fill, dtype=S32)
    if self_fill == 0.0:
        assert r64[0][5] == 0                                # isolated, nothing added: dinv 0
    if weighted:
        assert r64[0][7] == 0 and r64[0][8] == 0             # degree sums <= 0
    assert r64[2][3] == 0 and r64[2][4] == 0 and r64[2][6] == 0
    rpd, cold, vald = _i32(rp), _i32(col), (_f32(val) if weighted else None)
    outs = []
    for _ in range(2):
        DI, VO, SW = Out(1, n + 3), Out(1, nnz + 3), Out(1, n + 3)
        nat.call("gcn_norm_f32", rpd, cold, vald, n, self_fill, DI.mat, VO.mat, SW.mat)
        for O, k in ((DI, n), (VO, nnz), (SW, n)):
            own = torch.zeros(1, O.ld, dtype=torch.bool)
            own[0, :k] = True
            O.rest_untouched("gcn_norm", own)
        outs.append((DI, VO, SW))
    worst = Worst()
    what = "weighted %d fill %g" % (weighted, self_fill)
    for i, (nm, k) in enumerate((("dinv", n), ("val_out", nnz), ("self_w", n))):
        assert torch.equal(outs[0][i].bits, outs[1][i].bits), "two launches differ"
        worst.check("gcn_norm", "%s: %s" % (what, nm), outs[0][i].mat[0, :k], r64[i], r32[i])
    if self_fill <= 1.0:
        assert float(outs[0][0].mat[0, 5]) == self_fill         # the isolated row: dinv 0 without a self loop, 1 with a unit one
    worst.report()


# ============================================================================= tsgnn_sddmm_rows_f32
@pytest.mark.parametrize("feat", [1, 63, 64, 65, 128, 1000, 1024])
def test_sddmm_rows(feat):
    """one wave per row, lane l holds features l, l + 64, ...: under, at and over one and sixteen registers' worth.  Launched over all
    rows but the last five: their entries of dval, and their dself, stay untouched; rows without entries still get their dself"""
    nat = _nat()
    n, m = 41, 36
    deg = np.array([(7 * r) % 10 for r in range(n)])
    deg[10] = 70
    deg[m - 1] = 0                                           # the launch's last row has no entry
    rp = R.scan(deg)
    rng = np.random.default_rng(feat)
    col = rng.integers(0, n, int(rp[-1]))
    col[rp[10] + 1] = col[rp[10]]                            # a repeated entry
    nnz, own_e = int(rp[-1]), int(rp[m])
    g = torch.Generator().manual_seed(feat)
    x, dy = torch.randn(n, feat, generator=g), torch.randn(n, feat, generator=g)
    ldx, lddy = feat + 3, feat + 5
    xd, dyd, rpd, cold = _strided(x, ldx), _strided(dy, lddy), _i32(rp), _i32(col)
    r64, r32 = R.sddmm(rp[:m + 1], col, dy, x, dtype=D), R.sddmm(rp[:m + 1], col, dy, x, dtype=S32)
    worst = Worst()
    for with_self in (True, False):
        outs = []
        for _ in range(2):
            DV, DS = Out(1, nnz), Out(1, n)
            nat.call("sddmm_rows_f32", rpd, cold, dyd, lddy, xd, ldx, m, feat, DV.mat, DS.mat if with_self else None)
            assert nat.last_kernel() == "sddmm_rows_kernel"
            own = torch.zeros(1, nnz, dtype=torch.bool)
            own[0, :own_e] = True
            DV.rest_untouched("dval", own)
            own = torch.zeros(1, n, dtype=torch.bool)
            own[0, :m] = with_self
            DS.rest_untouched("dself", own)
            outs.append((DV, DS))
        assert torch.equal(outs[0][0].bits, outs[1][0].bits) and torch.equal(outs[0][1].bits, outs[1][1].bits), "two launches differ"
        what = "feat %d dself %s" % (feat, "given" if with_self else "NULL")
        worst.check("sddmm_rows", what + ": dval", outs[0][0].mat[0, :own_e], r64[0], r32[0])
        if with_self:
            worst.check("sddmm_rows", what + ": dself", outs[0][1].mat[0, :m], r64[1], r32[1])
    worst.report()
