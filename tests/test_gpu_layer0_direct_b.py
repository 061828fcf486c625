"""Layer 0's launch with its weight operands straight from W (csrc/rowgemm_body.h BDIR; tsgnn_gather_rowgemm_st_mode_f32 in
include/tsgnn.h): the launch recorded from a step, replayed on the same operands with W staged through LDS (b_mode = 1) and direct
(b_mode = 2), leaves every output the same bit for bit — v, rinv, z, the integer sums, the ghost row's numbers — over the kernel
shapes (one-group, two-group, 16- / 8-row units), K with and without a partial / an all-zero chunk, N with masked columns, both
gather forms; and a step does not depend on the switch.  (The host-side refusals: test_layer0_direct_b_host.py.)"""
import numpy as np
import pytest
import torch


class _A:
    bias = True


SIZES = (40, 1, 33, 70, 5)     # 149 rows = 5 panels: panel 1 holds the tail of graph 0, the one-node graph and the head of graph 2,
NMAX = 80                      # panel 4 is partial (21 rows)
K_ONE_GROUP = (4, 12, 32)                  # K <= 32: the one-group kernel
K_TWO_GROUPS = (36, 64, 92, 96, 128)       # 36, 92: a partial last chunk; 92, 96: group 1's all-zero chunk; 64, 128: no padding


def _batch(fin, dev, long_row):
    """-> (GraphBatch, x, label).  Symmetric edges; graph 3 has rows of 16, 9, 8, 7, 1 and 0 neighbours, its 16-hub's row of x is -0.0
    (its leaves' ONLY neighbour value) and so are the 8 neighbours of the 8-hub (a sum the table path leaves at -0.0).  long_row: node 0
    of graph 0 has 35 neighbours — a table with a CSR tail, no schedule."""
    from two_stage_gnn_amd.graph import GraphBatch
    off = np.concatenate([[0], np.cumsum(SIZES)])
    nb = [set() for _ in range(off[-1])]

    def edge(a, b):
        nb[a].add(b); nb[b].add(a)
    for i in range(SIZES[0] - 1):                              # graph 0: a path (+ a star of 35 around node 0)
        edge(off[0] + i, off[0] + i + 1)
    if long_row:
        for j in range(2, 36):
            edge(off[0], off[0] + j)
    for i in range(SIZES[2]):                                  # graph 2: a ring
        edge(off[2] + i, off[2] + (i + 1) % SIZES[2])
    o = off[3]
    for hub, n in ((0, 16), (20, 9), (30, 8), (40, 7)):
        for j in range(1, n + 1):
            edge(o + hub, o + hub + j)
    edge(o + 50, o + 51); edge(o + 51, o + 52)                 # (rows 53..69 of graph 3 have no neighbour)
    for i in range(SIZES[4] - 1):                              # graph 4: a path
        edge(off[4] + i, off[4] + i + 1)
    deg = np.array([len(s) for s in nb])
    assert {0, 1, 7, 8, 9, 16} <= set(deg.tolist()) and deg.max() == (35 if long_row else 16) and deg[off[1]] == 0
    n = int(off[-1])
    rowptr = np.zeros(n + NMAX + 1, dtype=np.int32)
    rowptr[1:n + 1] = np.cumsum(deg)
    rowptr[n + 1:] = rowptr[n]
    col = np.concatenate([np.sort(np.fromiter(s, dtype=np.int32, count=len(s))) for s in nb]).astype(np.int32)
    g = GraphBatch.from_csr(torch.from_numpy(rowptr).to(dev), torch.from_numpy(col).to(dev), None, np.array(SIZES), NMAX,
                            assume_symmetric=True)
    gen = torch.Generator(device="cpu").manual_seed(fin)
    x = torch.zeros(g.total_rows, fin, dtype=torch.float32)
    x[:n] = torch.randn(n, fin, generator=gen)
    x[o] = -0.0
    x[o + 31:o + 39] = -0.0
    return g, x.to(dev), torch.tensor([0, 1, 1, 0, 1], device=dev)


def _model(fin, dev, seed=1234):
    from two_stage_gnn_amd import dense_encoders as E
    torch.manual_seed(seed)
    return E.GcnEncoderGraph(fin, 128, 128, 2, 3, bn=True, args=_A(), final_dim="number_classes").to(dev)


def _record_step(model, x, g, label):
    from two_stage_gnn_amd import _native as nat
    prev, nat.trace = nat.trace, []
    try:
        model.loss(model(x, g)[1], label).backward()
        torch.cuda.synchronize()
        return nat.trace
    finally:
        nat.trace = prev


def _bits(t):
    return t.contiguous().view(torch.int32) if t.dtype == torch.float32 else t


def _layer0(rec):
    st = [r for r in rec if r[0] == "gather_rowgemm_st_f32"]
    assert len(st) == 1, [r[0] for r in rec]
    return st[0]


def _staged_and_direct(a, what):
    """the launch with arguments `a` (those of tsgnn_gather_rowgemm_st_f32) through the mode entry at 1 and 2; every output compared
    as int32 bits.  -> the staged launch's outputs"""
    from two_stage_gnn_amd import _native as nat
    v, rinv, z, rows, fill, sums, ghost = a[9], a[11], a[12], int(a[14]), int(a[17]), a[19], a[20]
    outs = []
    for mode in (1, 2):
        for t in (v[:rows + fill], rinv[:rows + fill], z[:rows], ghost):
            t.fill_(float("nan"))
        sums.zero_()
        nat.call("gather_rowgemm_st_mode_f32", *a, mode)
        torch.cuda.synchronize()
        outs.append([_bits(t).clone() for t in (v[:rows + fill], rinv[:rows + fill], z[:rows], sums, ghost)])
    for name, p, q in zip(("v", "rinv", "z", "sums", "ghost"), *outs):
        assert torch.equal(p, q), (what, name, int((p != q).sum()))
    sums.zero_()                                               # (as a step leaves them)
    return outs[0]


@pytest.mark.gpu
@pytest.mark.parametrize("long_row", [False, True], ids=["schedule+table", "table+tail"])
def test_direct_launch_equals_staged_launch_on_hand_made_batches(long_row):
    """one step at fin = 128 is recorded; its layer-0 launch is replayed at every K (the leading rows of W and columns of x), N = 128
    and 100 (masked columns), with and without fill rows, in every gather form the batch has; at K = 92 also without bias and with W
    a view into a wider matrix"""
    from two_stage_gnn_amd import _native as nat
    dev = torch.device("cuda")
    g, x, label = _batch(128, dev, long_row)
    rec = _record_step(_model(128, dev), x, g, label)          # (kept: the launch's pack riders write the images the record holds)
    a0 = list(_layer0(rec)[1])
    ell, ell_w, tail = g.ell()
    assert ell_w == 16 and (tail is not None) == long_row
    rows, fill0 = int(a0[14]), int(a0[17])
    assert rows == sum(SIZES) and fill0 > 0 and int(a0[15]) == 128 and int(a0[16]) == 128
    gen = torch.Generator(device="cpu").manual_seed(5)
    wide = torch.randn(128, 192, generator=gen).to(dev)        # W as a view: ldb = 192
    ran = set()
    for K in K_ONE_GROUP + K_TWO_GROUPS:
        for fill in (fill0, 0):
            forms = [("table", [ell, ell_w] + (list(tail) if tail is not None else [None, None]))]
            code = int(nat.lib().tsgnn_gather_sched_slots(rows, fill, K, int(g.panel_units), 1))
            assert code == (32 if K <= 32 else 24), (K, code)  # (a small batch: the two-group kernel from K = 33)
            sched = g.gather_schedule((16, 24) if code == 24 else (8, 32))
            assert (sched is None) == long_row
            if sched is not None:
                forms.append(("schedule", [sched, code, None, None]))
            for form, head in forms:
                variants = [("N=128", {}), ("N=100", {16: 100})]
                if K == 92:
                    variants += [("no bias", {8: None}), ("no bias N=100", {8: None, 16: 100}),
                                 ("W strided", {6: wide[:, 32:160], 7: wide.stride(0)}),
                                 ("W strided N=100", {6: wide[:, 32:132], 7: wide.stride(0), 16: 100})]
                for vname, sub in variants:
                    a = head + a0[4:]
                    a[15], a[17] = K, fill
                    for k_, v_ in sub.items():
                        a[k_] = v_
                    what = "K=%d fill=%d %s %s" % (K, fill, form, vname)
                    out = _staged_and_direct(a, what)
                    assert nat.last_kernel() == ("rowgemm_gather_st_kernel<false>" if K <= 32 else "rowgemm_gather_ks2_st_kernel"), what
                    assert not torch.isnan(out[0].view(torch.float32)[:rows, :int(a[16])]).any(), what
                    ran.add((K, form))
                    if K == 128 and not sub and not long_row:   # the -0.0 rows (test_gpu_gather_schedule.py)
                        o = sum(SIZES[:3])
                        assert (out[2][o + 1] == 0).all() and (out[2][o + 30] == torch.iinfo(torch.int32).min).all(), what
    assert len(ran) == 8 * (1 if long_row else 2)


@pytest.mark.gpu
@pytest.mark.parametrize("seed,tag", [(3, "DD b32 seed 3: 271 panels, 8-row units"), (6, "DD b32 seed 6: 288 panels, 16-row units")])
def test_direct_launch_equals_staged_launch_on_unit_panels(seed, tag):
    """the full-size batches whose layer-0 launch is cut into 8- / 16-row units (the only way to those instances)"""
    from two_stage_gnn_amd import synthetic
    dev = torch.device("cuda")
    hb = synthetic.host_batch(seed=seed, B=32, shape="DD", nmax=1000)
    g, x, label = synthetic.to_device(hb, dev)
    npan = -(-int(g.n_rows) // 32)
    ncu = torch.cuda.get_device_properties(dev).multi_processor_count
    if not (ncu < npan <= ncu + ncu // 2):
        tag = tag.replace("units", "rows")                     # (this device hosts every panel at once: plain panels)
    rec = _record_step(_model(synthetic.SHAPES["DD"][2], dev), x, g, label)
    r = _layer0(rec)
    assert ("units" in tag) == r[2].endswith("<true>"), (tag, r[2])
    _staged_and_direct(list(r[1]), tag)


@pytest.mark.gpu
def test_direct_launch_equals_staged_launch_on_a_capacity_padded_batch():
    """an ingest slot's batch: plain panels, rows with row_slot < 0 behind the real ones"""
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
    assert slot.row_cap > n
    rec = _record_step(_model(ds.num_node_labels, dev, seed=2), slot.x, slot.g, slot.label)
    a = list(_layer0(rec)[1])
    assert bool((a[18][:int(a[14])] < 0).any()), "no padding rows in the launch"
    _staged_and_direct(a, "capacity-padded batch")


@pytest.mark.gpu
def test_step_is_bitwise_the_same_with_and_without_direct_b(monkeypatch):
    from two_stage_gnn_amd import sage_stack as S
    dev = torch.device("cuda")
    g, x, label = _batch(92, dev, False)
    model = _model(92, dev)
    res = []
    for on in (True, False):
        monkeypatch.setattr(S, "L0_DIRECT_B", on)
        model.zero_grad(set_to_none=True)
        rec = _record_step_keep(model, x, g, label)
        assert [r[0] for r in rec[1] if r[0].startswith("gather_rowgemm_st")] == ["gather_rowgemm_st_f32" if on else "gather_rowgemm_st_mode_f32"]
        res.append(rec[0])
    assert len(res[0]) == len(res[1]) >= 3 + 10                # (three conv layers and the two Linear of the head: weight and bias each)
    for i, (p, q) in enumerate(zip(*res)):
        assert torch.equal(_bits(p), _bits(q)), i


def _record_step_keep(model, x, g, label):
    """one step -> ([loss, both head outputs, every parameter gradient], the recorded launches)"""
    from two_stage_gnn_amd import _native as nat
    prev, nat.trace = nat.trace, []
    try:
        vec, y = model(x, g)
        loss = model.loss(y, label)
        loss.backward()
        torch.cuda.synchronize()
        return ([loss.detach().clone(), vec.detach().clone(), y.detach().clone()]
                + [p.grad.clone() for p in model.parameters() if p.grad is not None]), nat.trace
    finally:
        nat.trace = prev
