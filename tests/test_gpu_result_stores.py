"""Placement of the result stores (csrc/common.h st_out: values a launch hands to a LATER launch, written through to memory): the row
panels' v / dX rows, rinv, zout and fill rows, the weight-gradient slabs, slot_post_bwd's dU rows and the head backward's dU role, each
driven through its C entry point on the smallest shapes that reach its paths.

Every test has the same three parts.  Every output lives in a buffer prefilled with one NaN bit pattern and followed by guard words.
After the launch (1) every element the kernel owns matches a float64 torch restatement at the rule of tests/fp32_yardstick.py, K = 8
(the yardstick is the restatement's own fp32 run on the CPU, never the kernel); (2) every other element of the buffer — row padding
between N and the row stride, the columns beside a column block, rows at or beyond the launch's rows, slab rows beyond K_in + 1 — and
(3) every guard word is bit for bit the pattern that was put there."""
import numpy as np
import pytest
import torch

from fp32_yardstick import _check
from gemm_ref import _slab_ref
from guard_buf import GUARD, PAT, Out, _du_ref, _owned  # noqa: F401

pytestmark = pytest.mark.gpu

def _nat():
    from two_stage_gnn_amd import _native as nat
    return nat


def _ell(rows, n_src, ell_w, seed):
    """a neighbour table [rows, ell_w]: row r has r % (ell_w + 1) neighbours (0 .. ell_w: empty, partial and full rows), packed to the
    front, -1 behind"""
    gen = torch.Generator().manual_seed(seed)
    t = torch.randint(0, n_src, (rows, ell_w), generator=gen, dtype=torch.int32)
    deg = torch.arange(rows) % (ell_w + 1)
    t[torch.arange(ell_w)[None, :] >= deg[:, None]] = -1
    return t


def _gather(x, ell, dtype):
    idx = ell.long()
    return (x.to(dtype)[idx.clamp(min=0)] * (idx >= 0)[..., None].to(dtype)).sum(1)


def _panel_ref(x, ell, w, bias, K, N, trans_b, normalize, fill, dtype):
    """-> z [rows, K], v [rows + fill, N], rinv [rows + fill] of a gather row-panel launch"""
    z = _gather(x[:, :K], ell, dtype)
    wm = w.to(dtype)
    u = z @ (wm[:N, :K].t() if trans_b else wm[:K, :N])
    f = torch.zeros(fill, N, dtype=dtype)
    if bias is not None:
        u = u + bias[:N].to(dtype)
        f = f + bias[:N].to(dtype)
    u = torch.cat([u, f])
    if not normalize:
        return z, u, torch.ones(u.size(0), dtype=dtype)
    nrm = u.norm(dim=1).clamp(min=1e-12)
    return z, u / nrm[:, None], 1.0 / nrm


def _panel_operands(rows, fill, seed):
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn(rows + fill, 128, generator=gen)
    w = torch.randn(128, 192, generator=gen)[:, 32:160]        # a view into a wider matrix: ldb = 192
    bias = torch.randn(128, generator=gen)
    return x, w, bias


def _check_panel(what, rows, fill, K, N, c0, V, R, Z, ref64, ref32, rinv_fill=True):
    z64, v64, r64 = ref64
    z32, v32, r32 = ref32
    torch.cuda.synchronize()
    _check(what + " v", V.mat[:rows + fill, c0:c0 + N], v64, v32)
    V.rest_untouched(what + " v", _owned(V.rows, V.ld, 0, rows + fill, c0, c0 + N))
    if R is not None:
        nr = rows + (fill if rinv_fill else 0)
        _check(what + " rinv", R.mat[:nr, 0], r64[:nr], r32[:nr])
        R.rest_untouched(what + " rinv", _owned(R.rows, 1, 0, nr, 0, 1))
    if Z is not None:
        _check(what + " z", Z.mat[:rows, :K], z64, z32)
        # (the float4 that holds column K - 1 is the kernel's to write when K % 4 != 0: the row stride is a multiple of 4)
        Z.rest_untouched(what + " z", _owned(Z.rows, Z.ld, 0, rows, 0, (K + 3) // 4 * 4))


ROWS = [32, 33, 63, 96]                 # a full panel, one row into the next, the last panel one short, three full panels


@pytest.mark.parametrize("zout", [True, False], ids=["z", "noz"])
@pytest.mark.parametrize("K,N,ldc", [(92, 128, 128), (128, 100, 384), (128, 128, 384), (32, 128, 128)])
@pytest.mark.parametrize("rows", ROWS)
def test_layer0_row_panels(rows, K, N, ldc, zout):
    """tsgnn_gather_rowgemm_st_f32 (the two-group kernel at K > 32, the one-group kernel at K = 32), table form: v as a column block of a
    wider buffer, zout with ldz > K, fill rows"""
    nat, fill, c0 = _nat(), 5, (128 if ldc > 128 else 0)
    x, w, bias = _panel_operands(rows, fill, rows * 1000 + K + N)
    ell = _ell(rows, rows, 16, rows + K)
    ref64 = _panel_ref(x, ell, w, bias, K, N, False, True, fill, torch.float64)
    ref32 = _panel_ref(x, ell, w, bias, K, N, False, True, fill, torch.float32)
    V, R = Out(rows + fill + 3, ldc), Out(rows + fill + 3, 1)
    Z = Out(rows + 3, K + 8) if zout else None
    wd = torch.zeros(128, 192).cuda()
    wd[:, 32:160] = w
    row_slot = (torch.arange(rows, dtype=torch.int32) % 7).cuda()
    sums = torch.zeros(2 * 8, dtype=torch.int64, device="cuda")
    ghost = torch.zeros(2, device="cuda")
    nat.call("gather_rowgemm_st_f32", ell.cuda(), 16, None, None, x.cuda(), 128, wd[:, 32:160], 192, bias.cuda(), V.mat[:, c0:], ldc,
             R.mat, Z.mat if zout else None, Z.ld if zout else 0, rows, K, N, fill, row_slot, sums, ghost, 1, None)
    assert nat.last_kernel().startswith("rowgemm_gather_ks2_st_kernel" if K > 32 else "rowgemm_gather_st_kernel<false>")
    _check_panel("layer0 rows=%d K=%d N=%d ldc=%d" % (rows, K, N, ldc), rows, fill, K, N, c0, V, R, Z, ref64, ref32)


@pytest.mark.parametrize("trans_b,K,N,normalize,fill", [(0, 128, 128, 1, 4), (0, 92, 100, 1, 0), (0, 128, 64, 1, 4), (1, 128, 128, 0, 0),
                                                        (1, 128, 100, 0, 0), (1, 64, 128, 0, 0)])
@pytest.mark.parametrize("rows", ROWS)
def test_gather_row_panels(rows, trans_b, K, N, normalize, fill):
    """tsgnn_gather_rowgemm_f32: the forward form (bias, normalised rows, fill rows, zout) and the input-gradient form (W transposed, no
    epilogue: no barrier between the K loop and the stores), widths 128, 100 (masked columns) and 64 (two column tiles)"""
    nat, ldc, c0 = _nat(), 384, 132
    x, w, bias = _panel_operands(rows, fill, rows * 77 + K + N + trans_b)
    if not normalize:
        bias = None
    ell = _ell(rows, rows, 8, rows + N)
    ref64 = _panel_ref(x, ell, w, bias, K, N, trans_b, normalize, fill, torch.float64)
    ref32 = _panel_ref(x, ell, w, bias, K, N, trans_b, normalize, fill, torch.float32)
    V = Out(rows + fill + 2, ldc)
    R = Out(rows + fill + 2, 1) if normalize else None
    Z = Out(rows + 2, K + 4) if normalize else None
    wd = torch.zeros(128, 192).cuda()
    wd[:, 32:160] = w
    nat.call("gather_rowgemm_f32", ell.cuda(), 8, None, None, x.cuda(), 128, wd[:, 32:160], 192, trans_b,
             bias.cuda() if bias is not None else None, V.mat[:, c0:], ldc, R.mat if R is not None else None,
             Z.mat if Z is not None else None, Z.ld if Z is not None else 0, rows, K, N, normalize, fill)
    _check_panel("gather rows=%d tb=%d K=%d N=%d" % (rows, trans_b, K, N), rows, fill, K, N, c0, V, R, Z, ref64, ref32)


@pytest.mark.parametrize("K_in", [89, 92, 128])
def test_linear_wgrad_slabs(K_in):
    """tsgnn_linear_wgrad_f32 leaving its slabs (dw = NULL): K_in = 128 (the unpredicated store path), 92 and 89 (predicated rows, a
    partial float4 of z), a short last slab, bias-only rows"""
    nat, rows, rps, bo = _nat(), 150, 64, 5
    nslab = -(-rows // rps)
    gen = torch.Generator().manual_seed(K_in)
    z = torch.randn(rows + bo, 132, generator=gen)
    du = torch.randn(rows + bo, 128, generator=gen)
    W = Out(nslab * (K_in + 1) + 2, 128)
    nat.call("linear_wgrad_f32", z.cuda(), 132, du.cuda(), 128, rows, K_in, 128, nslab, rps, bo, W.mat, None, None)
    what = "linear_wgrad K_in=%d" % K_in
    torch.cuda.synchronize()
    _check(what, W.mat[:nslab * (K_in + 1)].view(nslab, K_in + 1, 128), _slab_ref(z, du, rows, K_in, nslab, rps, bo, torch.float64),
           _slab_ref(z, du, rows, K_in, nslab, rps, bo, torch.float32))
    W.rest_untouched(what, _owned(W.rows, 128, 0, nslab * (K_in + 1), 0, 128))


def test_ragged_slabs():
    """tsgnn_ragged_tn_f32 at K = N = 128: slabs by slab_row_ptr — a full chunk, a short slab, an empty one, a slab of two chunks"""
    nat = _nat()
    ptr = [0, 32, 45, 45, 109]
    nslab, rows = len(ptr) - 1, ptr[-1]
    gen = torch.Generator().manual_seed(11)
    s, x = torch.randn(rows, 128, generator=gen), torch.randn(rows, 128, generator=gen)
    W = Out(nslab * 129 + 2, 128)
    out = torch.empty(2, 128, 128, device="cuda")
    nat.call("ragged_tn_f32", s.cuda(), 128, x.cuda(), 128, 128, 128, torch.tensor(ptr, dtype=torch.int32).cuda(), nslab,
             torch.tensor([0, 2, 4], dtype=torch.int32).cuda(), 2, W.mat, out)
    torch.cuda.synchronize()

    def ref(dtype):
        o = torch.zeros(nslab, 129, 128, dtype=dtype)
        for k in range(nslab):
            a, b = s[ptr[k]:ptr[k + 1]].to(dtype), x[ptr[k]:ptr[k + 1]].to(dtype)
            o[k, :128], o[k, 128] = a.t() @ b, b.sum(0)
        return o
    _check("ragged slabs", W.mat[:nslab * 129].view(nslab, 129, 128), ref(torch.float64), ref(torch.float32))
    W.rest_untouched("ragged slabs", _owned(W.rows, 128, 0, nslab * 129, 0, 128))


@pytest.mark.parametrize("rows,rps", [(96, 32), (150, 64), (63, 64)])
def test_merged_backward_launch(rows, rps):
    """tsgnn_sage_layer_bwd_f32: the slabs with two blocks per slab and dX = (A dU) W^T in one launch, dX as a column block of a wider
    buffer; a short last slab, a partial last panel, bias-only rows"""
    nat, bo, ldx, c0 = _nat(), 3, 384, 128
    nslab = -(-rows // rps)
    gen = torch.Generator().manual_seed(rows + rps)
    z = torch.randn(rows, 128, generator=gen)
    du = torch.randn(rows + bo, 128, generator=gen)
    w = torch.randn(128, 128, generator=gen)
    ell = _ell(rows, rows, 16, rows)
    X, W = Out(rows + 2, ldx), Out(nslab * 129 + 2, 128)
    nat.call("sage_layer_bwd_f32", ell.cuda(), 16, None, None, du.cuda(), 128, w.cuda(), 128, X.mat[:, c0:], ldx, z.cuda(), 128, rows, nslab,
             rps, bo, W.mat, 1, None)
    what = "sage_layer_bwd rows=%d rps=%d" % (rows, rps)
    torch.cuda.synchronize()
    _check(what + " slabs", W.mat[:nslab * 129].view(nslab, 129, 128), _slab_ref(z, du, rows, 128, nslab, rps, bo, torch.float64),
           _slab_ref(z, du, rows, 128, nslab, rps, bo, torch.float32))
    W.rest_untouched(what + " slabs", _owned(W.rows, 128, 0, nslab * 129, 0, 128))
    _check(what + " dX", X.mat[:rows, c0:c0 + 128], _gather(du[:rows], ell, torch.float64) @ w.double().t(),
           _gather(du[:rows], ell, torch.float32) @ w.t())
    X.rest_untouched(what + " dX", _owned(X.rows, ldx, 0, rows, c0, c0 + 128))


@pytest.mark.parametrize("ghosts", [True, False], ids=["ghost", "noghost"])
def test_slot_post_bwd_rows(ghosts):
    """tsgnn_slot_post_bwd_f32 at B = 6, F = 128, lddu > F: slot 0 is in every graph (its ghost row is unused: a zero row), slots 9 and 10
    only in ghosts, and the batch without ghost rows"""
    import test_gpu_slot_kernels as T
    nat, B, F, lddu = _nat(), 6, 128, 140
    c = T.case(B, F, ghosts)
    L = c.L
    mean, rstd, _ = T.run_fwd(c, True)
    d1, dout = T.dev(c.dxs), T.dev(c.dout)
    D = Out(L.rows + 2, lddu)
    nat.call("slot_post_bwd_f32", *c.dev_struct(), T.dev(c.v32), F, d1, F, None, 0, dout, F, c.arg.cuda(), F, 1, 1, mean, rstd,
             c.rinv32.cuda(), D.mat, lddu)
    torch.cuda.synchronize()
    T.check_bwd("slot_post_bwd B6 F128 %s" % ("ghost" if ghosts else "noghost"), c, D.mat[:L.rows, :F])
    D.rest_untouched("slot_post_bwd du", _owned(D.rows, lddu, 0, L.rows, 0, F))


def test_head_du_role():
    """the dU rows of the head's backward launch (tsgnn_head2_bwd_du_map_f32) at B = 3: a graph shorter than a chunk of 64 rows, a graph
    of one node, a graph that spans two chunks.  The launch is recorded from a step and replayed with dU in a guarded buffer, lddu > F;
    dout — the readout gradient the launch's row blocks write and its dU blocks rebuild — is read back from the launch and is an INPUT
    of the restatement"""
    from two_stage_gnn_amd import dense_encoders as E
    from two_stage_gnn_amd.graph import GraphBatch
    nat, dev = _nat(), torch.device("cuda")
    sizes, nmax, fin = (30, 1, 100), 110, 12
    n = sum(sizes)
    off = np.concatenate([[0], np.cumsum(sizes)])
    nb = [[] for _ in range(n)]
    for b, s in enumerate(sizes):                              # every graph a path
        for i in range(s - 1):
            nb[off[b] + i].append(off[b] + i + 1)
            nb[off[b] + i + 1].append(off[b] + i)
    rowptr = np.zeros(n + nmax + 1, dtype=np.int32)
    rowptr[1:n + 1] = np.cumsum([len(s) for s in nb])
    rowptr[n + 1:] = rowptr[n]
    col = np.concatenate([np.sort(np.asarray(s, dtype=np.int32)) for s in nb]).astype(np.int32)
    g = GraphBatch.from_csr(torch.from_numpy(rowptr).to(dev), torch.from_numpy(col).to(dev), None, np.array(sizes), nmax,
                            assume_symmetric=True)

    class A:
        bias = True
    torch.manual_seed(7)
    model = E.GcnEncoderGraph(fin, 128, 128, 2, 3, bn=True, args=A(), final_dim="number_classes").to(dev)
    x = torch.zeros(g.total_rows, fin, device=dev)
    x[:g.n_rows] = torch.randn(g.n_rows, fin, generator=torch.Generator().manual_seed(3)).to(dev)
    prev, nat.trace = nat.trace, []
    try:
        model.loss(model(x, g)[1], torch.tensor([0, 1, 1], device=dev)).backward()
        torch.cuda.synchronize()
        rec = [r for r in nat.trace if r[0] == "head2_bwd_du_map_f32"]
    finally:
        nat.trace = prev
    assert len(rec) == 1, "the step's head backward did not carry the dU role"
    a = list(rec[0][1])
    # (... dout 14, lddo 15 ... graph_ptr 21, n_real 22, n_ghost_rows 23, max_nodes 24, v 25, ldv 26, rinv 27, arg 28, seg_off 29, F 30, du 31, lddu 32)
    B, F, n_real, n_ghost, off = int(a[10]), int(a[30]), int(a[22]), int(a[23]), int(a[29])
    assert (B, F, n_real) == (3, 128, sum(sizes)) and n_ghost > max(sizes)
    D = Out(n_real + B + 2, F + 12)
    a[31], a[32] = D.mat, D.ld
    nat.call("head2_bwd_du_map_f32", *a)
    torch.cuda.synchronize()
    v, rinv, arg, dout = a[25].cpu()[:, :F], a[27].cpu(), a[28].cpu().view(B, F), a[14].cpu()
    gp = a[21].cpu()
    _check("head dU role", D.mat[:n_real + B, :F], _du_ref(v, rinv, arg, dout, off, gp, n_real, n_ghost, torch.float64),
           _du_ref(v, rinv, arg, dout, off, gp, n_real, n_ghost, torch.float32))
    D.rest_untouched("head dU role", _owned(D.rows, D.ld, 0, n_real + B, 0, F))


def _replay_layer0(a, table, what):
    """the recorded layer-0 launch `a` (arguments of tsgnn_gather_rowgemm_st_f32) with v, rinv and z in guarded buffers — v a column block,
    ldz > K — against the restatement over the batch's neighbour table (ell, ell_w, (tail_ptr, tail_col) or None)"""
    nat = _nat()
    x, w, bias, rows, K, N, fill = a[4].cpu(), a[6].cpu(), a[8].cpu(), int(a[14]), int(a[15]), int(a[16]), int(a[17])
    ell, ell_w, tail = table
    ell = ell.cpu().view(-1, ell_w)[:rows]

    def ref(dtype):
        z, v, r = _panel_ref(x[:, :K], ell, w, bias, K, N, False, True, fill, dtype)
        if tail is not None:
            tp, tc = tail[0].cpu().long(), tail[1].cpu().long()
            dst = torch.repeat_interleave(torch.arange(rows), tp[1:rows + 1] - tp[:rows])
            z = z.index_add(0, dst, x[:, :K].to(dtype)[tc[:dst.numel()]])
            u = torch.cat([z @ w.to(dtype)[:K, :N] + bias[:N].to(dtype), bias[:N].to(dtype).expand(fill, N)])
            nrm = u.norm(dim=1).clamp(min=1e-12)
            v, r = u / nrm[:, None], 1.0 / nrm
        return z, v, r
    V, R, Z = Out(rows + fill + 2, 256), Out(rows + fill + 2, 1), Out(rows + 2, (K + 3) // 4 * 4 + 4)
    a = list(a)
    a[9], a[10], a[11], a[12], a[13] = V.mat[:, 64:], 256, R.mat, Z.mat, Z.ld
    a[19].zero_()
    nat.call("gather_rowgemm_st_f32", *a)
    torch.cuda.synchronize()
    a[19].zero_()                                              # (the sums, as a step leaves them)
    _check_panel(what, rows, fill, K, N, 64, V, R, Z, ref(torch.float64), ref(torch.float32))
    return nat.last_kernel()


def test_layer0_schedule_and_table_forms():
    """a recorded step's layer-0 launch (K = 92: the two-group kernel) in the schedule form it ran in and in the table form"""
    import test_gpu_layer0_direct_b as D
    dev = torch.device("cuda")
    g, x, label = D._batch(92, dev, False)
    a = list(D._layer0(D._record_step(D._model(92, dev), x, g, label))[1])
    ell, ell_w, tail = g.ell()
    assert tail is None and a[2] is None and a[1] not in (4, 8, 16), "the step is expected to run on the schedule"
    table = (ell, ell_w, None)
    _replay_layer0(a, table, "layer 0, schedule form")
    _replay_layer0([ell, ell_w, None, None] + a[4:], table, "layer 0, table form")


@pytest.mark.parametrize("seed", [3, 6], ids=["8-row units", "16-row units"])
def test_layer0_unit_panels(seed):
    """the full-size batches whose layer-0 launch is cut into 8- / 16-row units behind one full panel per compute unit"""
    import test_gpu_layer0_direct_b as D
    from two_stage_gnn_amd import synthetic
    dev = torch.device("cuda")
    g, x, label = synthetic.to_device(synthetic.host_batch(seed=seed, B=32, shape="DD", nmax=1000), dev)
    a = list(D._layer0(D._record_step(D._model(synthetic.SHAPES["DD"][2], dev), x, g, label))[1])
    ell, ell_w, tail = g.ell()
    kern = _replay_layer0([ell, ell_w] + (list(tail) if tail is not None else [None, None]) + a[4:], (ell, ell_w, tail),
                          "layer 0, DD b32 seed %d" % seed)
    npan = -(-int(g.n_rows) // 32)
    ncu = torch.cuda.get_device_properties(dev).multi_processor_count
    assert kern.endswith("<true>") == (ncu < npan <= ncu + ncu // 2), kern


def test_layer0_capacity_padded_batch():
    """an ingest slot's batch: plain panels, rows that belong to no graph behind the real ones (they are rows of the launch)"""
    import test_gpu_layer0_direct_b as D
    from two_stage_gnn_amd import ingest
    dev = torch.device("cuda")
    ds = ingest.synthetic_dataset(seed=9, n_graphs=24, shape="DD", nmax=600)
    ids = np.array([3, 17, 5, 11, 20, 8])
    n = int(ds.sizes[ids].sum())
    nnz = int(sum(ds.rowptr[ds.graph_ptr[i + 1]] - ds.rowptr[ds.graph_ptr[i]] for i in ids))
    slot = ingest.CapacityBatch(len(ids), 600, (n + 200 + 31) // 32 * 32, nnz + 500, ds.num_node_labels, dev)
    slot.collate(ds, ids)
    slot.pull()
    torch.cuda.synchronize()
    a = list(D._layer0(D._record_step(D._model(ds.num_node_labels, dev, seed=2), slot.x, slot.g, slot.label))[1])
    assert bool((a[18][:int(a[14])] < 0).any()), "no padding rows in the launch"
    ell, ell_w, tail = slot.g.ell()
    _replay_layer0([ell, ell_w] + (list(tail) if tail is not None else [None, None]) + a[4:], (ell, ell_w, tail), "layer 0, capacity-padded")
