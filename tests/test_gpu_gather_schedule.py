"""The row panels' gather schedule on the device (csrc/rowgemm_body.h SCHED; format: include/tsgnn.h): the three fused layer entries
launched with the schedule produce, bit for bit, what they produce with the neighbour table — every output, with and without the
weight image —, a step does not depend on the switch, and the default step hands the schedule to all five gather launches.
(The packer itself: test_gather_schedule_host.py.)"""
import numpy as np
import pytest
import torch


class _A:
    bias = True


SIZES = (5, 33, 70)            # 108 rows = 4 panels: panel 0 holds graph 0 and the head of graph 1, panel 3 is partial (12 rows)
NMAX = 80


def _small_batch(fin, dev):
    """-> (GraphBatch, x, label).  Symmetric edges; graph 2 has rows of 16, 9, 8, 7, 1 and 0 neighbours.  x: the row of the 16-hub is
    -0.0 (its leaves' ONLY neighbour value), and so are the 8 neighbours of the 8-hub (a sum the table path leaves at -0.0)."""
    from two_stage_gnn_amd.graph import GraphBatch
    off = np.concatenate([[0], np.cumsum(SIZES)])
    nb = [set() for _ in range(off[-1])]

    def edge(a, b):
        nb[a].add(b); nb[b].add(a)
    for i in range(SIZES[0] - 1):                              # graph 0: a path
        edge(off[0] + i, off[0] + i + 1)
    for i in range(SIZES[1]):                                  # graph 1: a ring
        edge(off[1] + i, off[1] + (i + 1) % SIZES[1])
    o = off[2]
    for hub, n in ((0, 16), (20, 9), (30, 8), (40, 7)):
        for j in range(1, n + 1):
            edge(o + hub, o + hub + j)
    edge(o + 50, o + 51); edge(o + 51, o + 52)                 # (rows 53..69 of graph 2 have no neighbour)
    deg = np.array([len(s) for s in nb])
    assert {0, 1, 7, 8, 9, 16} <= set(deg.tolist()) and deg.max() == 16
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
    return g, x.to(dev), torch.tensor([0, 1, 1], device=dev)


def _model(fin, dev):
    from two_stage_gnn_amd import dense_encoders as E
    torch.manual_seed(1234)
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


def _poison(*ts):
    for t in ts:
        if t is not None:
            t.fill_(float("nan")) if t.is_floating_point() else t.fill_(-7)


def _same(outs, what):
    for k, o in enumerate(outs[1:]):
        for i, (p, q) in enumerate(zip(outs[0], o)):
            assert torch.equal(p, q), (what, "form", k + 1, "output", i)


@pytest.mark.gpu
@pytest.mark.parametrize("fin,code0", [(12, 32), (92, 24)])
def test_schedule_launches_equal_table_launches(fin, code0):
    """layer 0 at K = fin (12: the one-group kernel, 8 x 32; 92: the two-group kernel, 16 x 24), the hidden layers at K = N = 128:
    schedule form against table form on the same operands, every output bitwise"""
    from two_stage_gnn_amd import _native as nat
    dev = torch.device("cuda")
    g, x, label = _small_batch(fin, dev)
    rec = _record_step(_model(fin, dev), x, g, label)
    st = [r for r in rec if r[0] == "gather_rowgemm_st_f32"]
    fwd = [r for r in rec if r[0] == "sage_layer_fwd_bn_f32"]
    bwd = [r for r in rec if r[0] == "sage_layer_bwd_f32"]
    assert len(st) == 1 and len(fwd) == 2 and len(bwd) == 2, [r[0] for r in rec]
    for r in st + fwd + bwd:                                   # the step itself ran on the schedule
        assert r[1][1] == (code0 if r in st else 32) and r[1][2] is None and r[1][3] is None, (r[0], r[1][1])
    ell, ell_w, tail = g.ell()
    ell_s, tcol_s = g.ell_slots()
    assert ell_w == 16 and tail is None and tcol_s is None
    # ---- layer 0 (plain gather of x: the -0.0 rows)
    a = list(st[0][1])
    assert int(a[15]) == fin and int(a[14]) == sum(SIZES)
    v, rinv, z, rows, fill, sums, ghost = a[9], a[11], a[12], int(a[14]), int(a[17]), a[19], a[20]
    outs = []
    for head in ([a[0], a[1], None, None], [ell, ell_w, None, None]):
        _poison(v[:rows + fill], rinv[:rows + fill], z[:rows], ghost)
        sums.zero_()
        nat.call(st[0][0], *(head + a[4:]))
        torch.cuda.synchronize()
        outs.append([_bits(t).clone() for t in (v[:rows + fill], rinv[:rows + fill], z[:rows], sums, ghost)])
    _same(outs, "layer 0")
    zb = outs[0][2]
    o = sum(SIZES[:2])
    assert (zb[o + 1] == 0).all(), "a row whose only neighbour is -0.0 aggregates to +0.0 (the table path adds an empty entry)"
    assert (zb[o + 30] == torch.iinfo(torch.int32).min).all(), "eight -0.0 neighbours sum to -0.0 (no empty entry is added)"
    # ---- hidden layers forward, in the step's order (each leaves the sums the next one reads)
    for r in fwd:
        a = list(r[1])
        v, rinv, z, packed, packed_out, mean, rstd, sums_out, ghost_out = a[9], a[11], a[12], a[22], a[23], a[27], a[28], a[30], a[31]
        rows, fill = int(a[14]), int(a[16])
        assert a[-1] is not None
        outs = []
        for head in ([a[0], a[1], None, None], [ell_s, ell_w, None, None]):
            for img in (a[-1], None):
                _poison(v[:rows + fill], rinv[:rows + fill], z[:rows], mean, rstd, ghost_out)
                for t in (packed, packed_out, sums_out):
                    if t is not None:
                        t.zero_()
                nat.call(r[0], *(head + a[4:-1] + [img]))
                torch.cuda.synchronize()
                outs.append([_bits(t).clone() for t in (v[:rows + fill], rinv[:rows + fill], z[:rows], packed, packed_out, mean, rstd, sums_out,
                                                        ghost_out) if t is not None])
        _same(outs, r[2])
    # ---- hidden layers backward (operands as the step's backward left them): dX and the slabs
    for r in bwd:
        a = list(r[1])
        dxs, ws, rows = a[8], a[16], int(a[12])
        assert a[-1] is not None
        outs = []
        for head in ([a[0], a[1], None, None], [ell, ell_w, None, None]):
            for img in (a[-1], None):
                _poison(dxs[:rows], ws)
                nat.call(r[0], *(head + a[4:-1] + [img]))
                torch.cuda.synchronize()
                outs.append([_bits(dxs[:rows]).clone(), _bits(ws).clone()])
        _same(outs, r[2])
    # leave the batch's accumulators as a step leaves them
    for r in fwd:
        for t in (r[1][22], r[1][23], r[1][30], r[1][25]):
            if t is not None:
                t.zero_()
    torch.cuda.synchronize()


@pytest.mark.gpu
def test_entries_refuse_a_schedule_they_cannot_run():
    """a code that names another kernel's shape, a CSR tail beside a schedule, a misaligned schedule: refused before any launch"""
    from two_stage_gnn_amd import _native as nat
    dev = torch.device("cuda")
    g, x, label = _small_batch(12, dev)
    rec = _record_step(_model(12, dev), x, g, label)
    st = [r for r in rec if r[0] == "gather_rowgemm_st_f32"][0]
    bwd = [r for r in rec if r[0] == "sage_layer_bwd_f32"][0]

    def refused(r, **kw):
        a = list(r[1])
        for k, v in kw.items():
            a[int(k[1:])] = v
        try:
            return nat.try_call(r[0], *a) is False             # (TSGNN_EUNSUPPORTED)
        except RuntimeError:
            return True                                        # (TSGNN_EINVAL)
    bogus = torch.zeros(8, dtype=torch.int32, device=dev)
    assert st[1][1] == 32 and bwd[1][1] == 32
    assert refused(st, a1=24)                                  # K = 12 runs the one-group kernel: 8 x 32 only
    assert refused(st, a2=bogus, a3=bogus) and refused(bwd, a2=bogus, a3=bogus)
    assert refused(bwd, a1=24)
    assert refused(bwd, a0=bwd[1][0].view(-1)[1:])             # 4 bytes off a 16-byte boundary
    torch.cuda.synchronize()


@pytest.mark.gpu
def test_step_is_bitwise_the_same_with_and_without_the_schedule(monkeypatch):
    from two_stage_gnn_amd import sage_stack as S
    dev = torch.device("cuda")
    g, x, label = _small_batch(92, dev)
    model = _model(92, dev)
    res = []
    for on in (True, False):
        monkeypatch.setattr(S, "GATHER_SCHED", on)
        model.zero_grad(set_to_none=True)
        vec, y = model(x, g)
        loss = model.loss(y, label)
        loss.backward()
        torch.cuda.synchronize()
        res.append([loss.detach().clone(), vec.detach().clone(), y.detach().clone()] + [p.grad.clone() for p in model.parameters() if p.grad is not None])
    assert len(res[0]) == len(res[1]) >= 3 + 10                # (three conv layers and the two Linear of the head: weight and bias each)
    for i, (p, q) in enumerate(zip(*res)):
        assert torch.equal(_bits(p), _bits(q)), i


@pytest.mark.gpu
def test_default_step_passes_the_schedule_to_all_five_gather_launches():
    from two_stage_gnn_amd import _native as nat, synthetic
    dev = torch.device("cuda")
    hb = synthetic.host_batch(seed=0, B=32, shape="DD", nmax=1000)
    g, x, label = synthetic.to_device(hb, dev)
    rec = _record_step(_model(89, dev), x, g, label)
    gl = [r for r in rec if r[0] in ("gather_rowgemm_st_f32", "sage_layer_fwd_bn_f32", "sage_layer_bwd_f32")]
    assert [r[0] for r in gl] == ["gather_rowgemm_st_f32"] + 2 * ["sage_layer_fwd_bn_f32"] + 2 * ["sage_layer_bwd_f32"]
    st = gl[0][1]
    want0 = nat.lib().tsgnn_gather_sched_slots(int(g.n_rows), int(st[17]), int(st[15]), int(g.panel_units), 1)
    assert want0 in (24, 32)
    npan = -(-int(g.n_rows) // 32)
    for r in gl:
        code = want0 if r is gl[0] else 32
        a = r[1]
        assert a[1] == code and a[2] is None and a[3] is None, (r[0], a[1])
        assert a[0].dtype == torch.int32 and tuple(a[0].shape) == (npan, 16 if code == 24 else 8, 4 + code) and a[0].data_ptr() % 16 == 0
