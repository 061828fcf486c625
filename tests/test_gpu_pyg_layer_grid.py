"""The fused GATConv (csrc/gatconv.hip) and SAGEConv / GraphConv (csrc/sageconv.hip, sageconv_body.h) layers over the shapes their
kernels take, against fp64 runs of oracle/pyg_ref.py (arbitrated as in test_gpu_pyg_fused.py).

Every case records the kernels it dispatched (_native.trace): a case meant for a fused kernel fails if it took the composed path, and
each test asserts the instantiations / table widths it covered — a template instance or table width that never runs can hide a bad
lane index from the whole suite."""
import contextlib
import itertools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import pyg_ref as P
from test_gpu_pyg import grads, rand_graph, tie_free
from test_gpu_pyg_fused import _D, _hub_graph, assert_arbitrated

pytestmark = pytest.mark.gpu

GAT_SHAPES = [(H, Co) for H in (1, 2, 4, 8) for Co in (4, 8, 16, 32, 64) if H * Co <= 256]


@contextlib.contextmanager
def _traced():
    from two_stage_gnn_amd import _native as nat
    prev, nat.trace = nat.trace, []
    try:
        yield nat.trace
    finally:
        nat.trace = prev


def _oracle(fn, tensors, gy, dtype):
    """fn(*tensors) in dtype on the CPU: (output, gradient of <output, gy> w.r.t. every tensor)"""
    ts = [t.detach().cpu().to(dtype).requires_grad_(True) if t is not None else None for t in tensors]
    out = fn(*ts)
    live = [t for t in ts if t is not None]
    gs = grads((out * gy.to(dtype)).sum(), live)
    return out.detach(), gs


def _check(what, out, ps_hip, r32, g32, r64, g64, names):
    assert torch.isfinite(out).all(), (what, "non-finite output")
    assert_arbitrated(out, r32, r64, (what, "out"))
    for name, a, b, c in zip(names, ps_hip, g32, g64):
        assert torch.isfinite(a).all(), (what, name, "non-finite gradient")
        assert_arbitrated(a, b, c, (what, name))


# ------------------------------------------------------------------------------------------------ GATConv
def _gat_graphs(n):
    """edge lists of n nodes (targets = row 1): directed; hub targets with 100, 70, 20 and 9 sources; input self loops and
    duplicated edges (GATConv drops the loops and adds one per node; a duplicate counts twice in the softmax)"""
    directed = rand_graph(21, n, 4 * n, sym=False)
    g = torch.Generator().manual_seed(22)
    hub = [directed]
    for node, deg in ((0, 100), (1, 70), (2, 20), (3, 9)):
        src = torch.randperm(n, generator=g)[:deg]
        hub.append(torch.stack([src, torch.full_like(src, node)]))
    hub = torch.cat(hub, dim=1)
    loops = torch.randint(0, n, (n // 8,), generator=g)
    dup = directed[:, torch.randint(0, directed.size(1), (n // 4,), generator=g)]
    messy = torch.cat([directed, torch.stack([loops, loops]), dup, dup[:, :5]], dim=1)
    return {"directed": directed, "hub": hub, "loops+dups": messy}


def _gat_run(conv, x, ei, gy, apply_elu, trace, att_inert=False):
    """the fused layer against its fp32 / fp64 oracle; returns the (forward, backward) kernel names.  att_inert: every softmax has
    one entry (alpha = 1), so the att_l / att_r gradients are zero up to rounding: bounded by 1e-6 max |d lin_l.weight| instead"""
    H, Co = conv.heads, conv.out_channels
    has_bias = conv.bias is not None
    ps = [conv.lin_l.weight, conv.att_l, conv.att_r] + ([conv.bias] if has_bias else [])
    names = ["dx", "lin_l.weight", "att_l", "att_r"] + (["bias"] if has_bias else [])

    def fn(xr, w, al, ar, b=None):
        y = P.gat_conv(xr, ei, w, al, ar, b, H, concat=conv.concat, slope=conv.negative_slope)
        return F.elu(y) if apply_elu else y

    r32, g32 = _oracle(fn, [x] + ps, gy, torch.float32)
    r64, g64 = _oracle(fn, [x] + ps, gy, torch.float64)
    del trace[:]
    xg = x.cuda().requires_grad_(True)
    out = conv(xg, ei.cuda(), apply_elu=apply_elu)
    gg = grads((out * gy.cuda()).sum(), [xg] + ps)
    what = ("GATConv", H, Co, "concat" if conv.concat else "mean", "elu" if apply_elu else "-", conv.in_channels, has_bias,
            conv.negative_slope)
    fwd = [t for t in trace if t[0] == "gatconv_fwd_f32"]
    bwd = [t for t in trace if t[0] == "gatconv_bwd_rows_f32"]
    assert len(fwd) == 1 and len(bwd) == 1, (what, "did not take the fused GATConv kernels", [t[0] for t in trace])
    assert fwd[0][2] == "gatconv_fwd_kernel<%d>" % (Co // 4) and bwd[0][2] == "gatconv_bwd_rows_kernel<%d>" % (Co // 4), what
    assert fwd[0][1][5] == H and bwd[0][1][9] == H, what
    if att_inert:
        for a in gg[2:4]:
            assert float(a.abs().max()) <= 1e-6 * float(g64[1].abs().max()), what
        gg, g32, g64, names = gg[:2] + gg[4:], g32[:2] + g32[4:], g64[:2] + g64[4:], names[:2] + names[4:]
    _check(what, out, gg, r32, g32, r64, g64, names)
    return fwd[0][2], bwd[0][2]


def _gat_conv(fin, H, Co, concat, bias, slope, seed):
    from two_stage_gnn_amd import pyg
    torch.manual_seed(seed)
    conv = pyg.GATConv(fin, Co, heads=H, concat=concat, negative_slope=slope, bias=bias).cuda()
    if bias:
        with torch.no_grad():
            conv.bias.copy_(0.3 * torch.randn_like(conv.bias))
    return conv


def test_gatconv_grid():
    """every (H, Co) the kernels take, concatenated and averaged heads, ELU folded in and not (each LPH instantiation both ways),
    Fin 1 / 3 (padded rows) / 92 / 512, bias on and off, two negative slopes, over a directed list, hub targets of 9 .. 100 sources
    (several 8-entry batches) and a list with self loops and duplicates"""
    n = 240
    graphs = list(_gat_graphs(n).items())
    fins = (1, 3, 92, 512)
    heads, elus = set(), set()
    with _traced() as trace:
        k = 0
        for p, (H, Co) in enumerate(GAT_SHAPES):
            for concat in (True, False):
                fin = fins[k % 4]
                gname, ei = graphs[k % len(graphs)]
                elu = concat == (p % 2 == 0)
                conv = _gat_conv(fin, H, Co, concat, bias=k % 3 != 2, slope=0.05 if k % 5 == 3 else 0.2, seed=100 + k)
                out_w = H * Co if concat else Co
                x, gy = tie_free(200 + k, n, fin), tie_free(300 + k, n, out_w)
                kf, kb = _gat_run(conv, x, ei, gy, elu, trace)
                heads.update([(kf, H), (kb, H)])
                elus.add((kf, elu))
                k += 1
    for lph in (1, 2, 4, 8, 16):
        for kern in ("gatconv_fwd_kernel<%d>" % lph, "gatconv_bwd_rows_kernel<%d>" % lph):
            assert {h for (kk, h) in heads if kk == kern} == ({1, 2, 4, 8} if lph < 16 else {1, 2, 4}), kern
        assert {e for (kk, e) in elus if kk == "gatconv_fwd_kernel<%d>" % lph} == {True, False}, lph


@pytest.mark.parametrize("rows", [1, 3, 5])
def test_gatconv_few_rows(rows):
    """1, 3 and 5 target rows: a partly filled 4-wave block (and a graph whose only edges are the added self loops)"""
    ei = rand_graph(7, rows, 3 * rows, sym=False) if rows > 1 else torch.zeros(2, 0, dtype=torch.int64)
    with _traced() as trace:
        for i, (H, Co, concat) in enumerate([(1, 4, True), (8, 32, False), (2, 64, True), (4, 8, False)]):
            conv = _gat_conv(5, H, Co, concat, bias=True, slope=0.2, seed=40 + i)
            _gat_run(conv, tie_free(41 + i, rows, 5), ei, tie_free(42 + i, rows, H * Co if concat else Co), i % 2 == 0, trace,
                     att_inert=rows == 1)


def test_gatconv_logits_spread_60():
    """attention logits spread over about +-60: most exp terms of a row underflow; outputs and gradients stay finite and close"""
    n = 240
    ei = _gat_graphs(n)["hub"]
    with _traced() as trace:
        for i, (H, Co, concat) in enumerate([(1, 16, True), (2, 8, False), (4, 64, True), (8, 4, False), (8, 32, True)]):
            conv = _gat_conv(24, H, Co, concat, bias=True, slope=0.2, seed=60 + i)
            x = tie_free(61 + i, n, 24)
            with torch.no_grad():
                h = (x @ conv.lin_l.weight.cpu().t()).view(n, H, Co)
                for att in (conv.att_l, conv.att_r):
                    s = (h * att.cpu()).sum(-1)
                    att.mul_((30.0 / s.std(dim=0).clamp(min=1e-6)).view(1, H, 1).cuda())
                e = (h * conv.att_l.cpu()).sum(-1)
                assert float(e.max() - e.min()) > 100.0
            _gat_run(conv, x, ei, tie_free(62 + i, n, H * Co if concat else Co), i % 2 == 1, trace)


def test_gatconv_layers_packed_together():
    """1 to 4 layers of different (H, Co) packed in ONE pack launch (and unpacked in ONE launch): output and the gradients of
    lin_l.weight, att_l, att_r and bias of every layer"""
    from two_stage_gnn_amd import pyg
    from two_stage_gnn_amd import pyg_gat as pgat
    n = 200
    ei = _gat_graphs(n)["hub"]
    stack = [(2, 8, True), (8, 4, True), (1, 64, True), (4, 32, False)]
    for L in (1, 2, 3, 4):
        specs = stack[4 - L:]
        fin0 = 12
        convs, fin = [], fin0
        for l, (H, Co, concat) in enumerate(specs):
            convs.append(_gat_conv(fin, H, Co, concat, bias=True, slope=0.2, seed=80 + 10 * L + l))
            fin = H * Co if concat else Co
        x, gy = tie_free(90 + L, n, fin0), tie_free(91 + L, n, fin)
        ps = [t for c in convs for t in (c.lin_l.weight, c.att_l, c.att_r, c.bias)]
        names = ["dx"] + ["%d.%s" % (l, k) for l in range(L) for k in ("lin_l.weight", "att_l", "att_r", "bias")]

        def fn(xr, *pr):
            for l, (H, Co, concat) in enumerate(specs):
                w, al, ar, b = pr[4 * l:4 * l + 4]
                xr = P.gat_conv(xr, ei, w, al, ar, b, H, concat=concat)
                if l < L - 1:
                    xr = F.elu(xr)
            return xr

        r32, g32 = _oracle(fn, [x] + ps, gy, torch.float32)
        r64, g64 = _oracle(fn, [x] + ps, gy, torch.float64)
        with _traced() as trace:
            xg = x.cuda().requires_grad_(True)
            g = pyg.GATConv._loop_graph(ei.cuda(), n)
            wps = pgat.pack_layers(convs)
            h = xg
            for l, c in enumerate(convs):
                h = c(h, g, wp=wps[l], apply_elu=l < L - 1)
            gg = grads((h * gy.cuda()).sum(), [xg] + ps)
            names_run = [t[0] for t in trace]
            assert names_run.count("gatconv_pack_f32") == 1 and names_run.count("gatconv_unpack_f32") == 1, names_run
            assert names_run.count("gatconv_fwd_f32") == L, names_run
        _check(("packed", L), h, gg, r32, g32, r64, g64, names)


@pytest.mark.parametrize("L", [2, 5, 6])
def test_gat_net_depth(L):
    """GatNet at any depth: groups of up to 4 layers share a pack / unpack launch (2 layers: ONE launch each way); log-probabilities
    and every parameter gradient against P.gat_net, fp64-arbitrated"""
    from two_stage_gnn_amd import pyg
    from test_gpu_pyg_fused import _batch
    sizes = (30, 52, 17, 41)
    x, ei, batch = _batch(51, sizes, 2.5, 10)
    lab = torch.arange(len(sizes)) % 2
    torch.manual_seed(12)
    net = pyg.GatNet(10, 8, 2, heads=4, num_layers=L).cuda().train()
    with torch.no_grad():
        for c in net.convs:
            c.bias.copy_(0.1 * torch.randn_like(c.bias))
    d = _D(); d.x, d.edge_index, d.batch = x.cuda(), ei.cuda(), batch.cuda()
    names = [k for k, _ in net.named_parameters()]
    params = [p for _, p in net.named_parameters()]

    def oracle(dtype):
        p = {k: v.detach().cpu().to(dtype).requires_grad_(True) for k, v in net.state_dict().items()}
        yy = P.gat_net(p, x.to(dtype), ei, batch, L, 4)
        return yy, grads(F.nll_loss(yy, lab), [p[k] for k in names])

    y32, g32 = oracle(torch.float32)
    y64, g64 = oracle(torch.float64)
    with _traced() as trace:
        y = net(d)
        gg = grads(F.nll_loss(y, lab.cuda()), params)
        run = [t[0] for t in trace]
    groups = -(-L // 4)
    assert run.count("gatconv_pack_f32") == groups and run.count("gatconv_unpack_f32") == groups, run
    assert run.count("gatconv_fwd_f32") == L, run
    assert_arbitrated(y, y32, y64, "log-probabilities")
    for k, a, b, c in zip(names, gg, g32, g64):
        assert torch.isfinite(a).all(), k
        assert_arbitrated(a, b, c, k)


# ------------------------------------------------------------------------------------------------ SAGEConv / GraphConv
def _in_degree_list(seed, n, dmax, extra=None):
    """directed edge list (targets = row 1) whose largest in-degree is dmax (sources drawn with repetition: duplicates and self
    loops stay, PyG's SAGEConv counts them as edges); extra: edges appended"""
    g = torch.Generator().manual_seed(seed)
    deg = torch.randint(0, dmax + 1, (n,), generator=g)
    deg[n // 2] = dmax
    dst = torch.repeat_interleave(torch.arange(n), deg)
    src = torch.randint(0, n, (dst.numel(),), generator=g)
    ei = torch.stack([src, dst])
    return torch.cat([ei, extra], dim=1) if extra is not None else ei


def _sage_graphs(n):
    """(name, edge list, forward table width, forward tail): widths 4, 8, 16 without and with tail; a symmetric hub graph"""
    return [("deg<=4", _in_degree_list(1, n, 4), 4, False), ("deg5-8", _in_degree_list(2, n, 7), 8, False),
            ("deg9-16", _in_degree_list(3, n, 13), 16, False), ("deg>16", _in_degree_list(4, n, 40), 16, True),
            ("sym hub", _hub_graph(5, n, 2 * n, hubs=2, hub_deg=30), 16, True)]


def _sage_module(K, N, aggr, normalize, bias, seed):
    from two_stage_gnn_amd import pyg
    torch.manual_seed(seed)
    m = pyg.GraphConv(K, N, bias=bias) if aggr == "add" else pyg.SAGEConv(K, N, normalize=normalize, bias=bias)
    m = m.cuda()
    if bias:
        with torch.no_grad():
            m.lin_l.bias.copy_(0.2 * torch.randn_like(m.lin_l.bias))
    return m


def _sage_fn(m, ei):
    def fn(xr, wl, wr, bl=None):
        y = (P.sage_conv if m.aggr == "mean" else P.graph_conv)(xr, ei, wl, bl, wr)
        return F.normalize(y, p=2.0, dim=-1) if m.normalize else y
    return fn


def _sage_run(m, x, ei, gy, trace, fused=True, skip_rows=None):
    """the layer and its fp32 / fp64 oracle; returns the (width, has tail) of each sage_conv_kernel launch (forward first)"""
    has_bias = m.lin_l.bias is not None
    ps = [m.lin_l.weight, m.lin_r.weight] + ([m.lin_l.bias] if has_bias else [])
    names = ["dx", "lin_l.weight", "lin_r.weight"] + (["lin_l.bias"] if has_bias else [])
    fn = _sage_fn(m, ei)
    r32, g32 = _oracle(fn, [x] + ps, gy, torch.float32)
    r64, g64 = _oracle(fn, [x] + ps, gy, torch.float64)
    del trace[:]
    xg = x.cuda().requires_grad_(True)
    out = m(xg, ei.cuda())
    gg = grads((out * gy.cuda()).sum(), [xg] + ps)
    what = (type(m).__name__, m.in_channels, m.out_channels, m.aggr, m.normalize, has_bias, x.size(0))
    launches = [(t[1][1], t[1][2] is not None) for t in trace if t[0] == "sage_conv_f32"]
    assert all(t[2] == "sage_conv_kernel" for t in trace if t[0] == "sage_conv_f32")
    if fused:
        assert len(launches) == 2, (what, "did not take the fused SAGEConv kernel both ways", [t[0] for t in trace])
    else:
        assert not launches, what
    chk = list(gg)
    if skip_rows is not None:              # rows checked by the caller (F.normalize's eps branch: dx ~ 1e12)
        keep = torch.ones(x.size(0), dtype=torch.bool)
        keep[skip_rows] = False
        chk[0], g32[0], g64[0] = gg[0][keep.cuda()], g32[0][keep], g64[0][keep]
    _check(what, out, chk, r32, g32, r64, g64, names)
    return launches, out, gg


def test_sage_conv_grid():
    """K in {1, 3, 31, 33, 128} x N in {1, 3, 31, 33, 97, 128}, mean and add aggregation, over neighbour tables of width 4, 8 and
    16 (without and with the CSR tail).  Output widths that are no multiple of 4 take the composed path of pyg.SAGEConv (the fused
    backward needs 16-byte gradient rows): there the module is checked on that path and the fused FORWARD kernel on its own"""
    from two_stage_gnn_amd import pyg_sage as ps
    n = 180
    graphs = _sage_graphs(n)
    widths = set()
    with _traced() as trace:
        for k, (K, N, aggr) in enumerate(itertools.product((1, 3, 31, 33, 128), (1, 3, 31, 33, 97, 128), ("mean", "add"))):
            gname, ei, W, tail = graphs[k % len(graphs)]
            normalize = aggr == "mean" and k % 7 == 3
            m = _sage_module(K, N, aggr, normalize, bias=not (normalize and k % 2), seed=500 + k)
            x, gy = tie_free(600 + k, n, K), tie_free(700 + k, n, N)
            fused = N % 4 == 0
            launches, _, _ = _sage_run(m, x, ei, gy, trace, fused=fused)
            if fused:
                assert launches[0] == (W, tail), (gname, launches)
                widths.update(launches)
                continue
            # the fused forward kernel at this N: out rows of N floats (no padding)
            del trace[:]
            with torch.no_grad():
                y = ps.sage_conv(x.cuda(), m._graph(x, ei.cuda()), m.lin_l.weight, m.lin_l.bias, m.lin_r.weight, mean=aggr == "mean",
                                 normalize=normalize)
            assert [(t[1][1], t[1][2] is not None) for t in trace if t[0] == "sage_conv_f32"] == [(W, tail)], gname
            fn = _sage_fn(m, ei)
            pr = [m.lin_l.weight, m.lin_r.weight] + ([m.lin_l.bias] if m.lin_l.bias is not None else [])
            with torch.no_grad():
                r32 = fn(*[t.detach().cpu() for t in [x] + pr])
                r64 = fn(*[t.detach().cpu().double() for t in [x] + pr])
            assert_arbitrated(y, r32, r64, ("fused forward", K, N, aggr, gname))
    assert widths >= {(4, False), (8, False), (16, False), (16, True)}, widths


def test_sage_conv_transposed_table_width():
    """a directed list whose forward table is 4 wide and whose transposed table (the input gradient's) is 16 wide with a tail"""
    n = 160
    fan = torch.stack([torch.zeros(24, dtype=torch.int64), torch.arange(1, 25)])
    ei = _in_degree_list(8, n, 3, extra=fan)
    with _traced() as trace:
        for k, (K, N, aggr) in enumerate([(31, 64, "mean"), (3, 32, "add"), (128, 128, "mean")]):
            m = _sage_module(K, N, aggr, False, True, seed=900 + k)
            launches, _, _ = _sage_run(m, tie_free(910 + k, n, K), ei, tie_free(920 + k, n, N), trace)
            assert launches == [(4, False), (16, True)], launches


def test_sage_conv_normalize_zero_row():
    """normalize=True without bias: an isolated node with zero features has an exactly zero output row, and its input gradient is
    F.normalize's eps branch (the row gradient divided by eps, no norm term)"""
    n = 150
    ei = _in_degree_list(9, n, 6)
    z = n - 3
    ei = ei[:, (ei[0] != z) & (ei[1] != z)]                       # node z: isolated
    with _traced() as trace:
        for k, (K, N) in enumerate([(33, 64), (128, 128), (3, 4)]):
            m = _sage_module(K, N, "mean", True, False, seed=950 + k)
            x = tie_free(960 + k, n, K)
            x[z] = 0.0
            gy = tie_free(970 + k, n, N)
            _, out, gg = _sage_run(m, x, ei, gy, trace, skip_rows=[z])
            assert float(out[z].detach().abs().max()) == 0.0
            xr = x.double().requires_grad_(True)
            y = F.normalize(P.sage_conv(xr, ei, m.lin_l.weight.detach().cpu().double(), None, m.lin_r.weight.detach().cpu().double()),
                            p=2.0, dim=-1)
            dx64 = grads((y * gy.double()).sum(), [xr])[0]
            assert float(dx64[z].abs().max()) > 1e9
            torch.testing.assert_close(gg[0][z].cpu().double(), dx64[z], rtol=1e-4, atol=0.0)


@pytest.mark.parametrize("rows", [1, 31, 32, 33, 8300])
def test_sage_conv_row_counts(rows):
    """row panels of 32: a single row, one short panel, one exact panel, one row into the second panel, and more panels than CUs"""
    ei = _in_degree_list(10, rows, min(rows, 20)) if rows > 1 else torch.zeros(2, 0, dtype=torch.int64)
    with _traced() as trace:
        for k, (K, N, aggr) in enumerate([(33, 64, "mean"), (128, 32, "add")]):
            m = _sage_module(K, N, aggr, False, True, seed=980 + k)
            _sage_run(m, tie_free(990 + k, rows, K), ei, tie_free(995 + k, rows, N), trace)


# ------------------------------------------------------------------------------------------------ SageNet: the post epilogue
def _sage_net_case(sizes, fin, hid, L, seed):
    from two_stage_gnn_amd import pyg
    from two_stage_gnn_amd import pyg_sage as ps
    from test_gpu_pyg_fused import _batch
    x, ei, batch = _batch(seed, sizes, 1.5, fin)
    lab = torch.arange(len(sizes)) % 2
    torch.manual_seed(seed)
    net = pyg.SageNet(fin, hid, 2, num_layers=L).cuda().eval()
    d = _D(); d.x, d.edge_index, d.batch = x.cuda(), ei.cuda(), batch.cuda()
    assert ps.stack_ok(net.graph(d), list(net.convs), d.x)
    names = [k for k, _ in net.named_parameters()]
    params = [p for _, p in net.named_parameters()]

    def oracle(dtype):
        p = {k: v.detach().cpu().to(dtype).requires_grad_(True) for k, v in net.state_dict().items()}
        y = P.sage_net(p, x.to(dtype), ei, batch, L)
        return y, grads(F.nll_loss(y, lab), [p[k] for k in names])

    y32, g32 = oracle(torch.float32)
    y64, g64 = oracle(torch.float64)
    with _traced() as trace:
        y = net(d)
        gg = grads(F.nll_loss(y, lab.cuda()), params)
        posts = [t for t in trace if t[0] == "sage_conv_f32" and t[1][26] is not None]
    assert len(posts) == L - 1, [t[0] for t in trace]
    assert_arbitrated(y, y32, y64, "log-probabilities")
    for k, a, b, c in zip(names, gg, g32, g64):
        assert_arbitrated(a, b, c, k)
    net.fused = False
    y2 = net(d)
    g2 = grads(F.nll_loss(y2, lab.cuda()), params)
    torch.testing.assert_close(y2, y, rtol=1e-5, atol=1e-5)
    for k, a, b in zip(names, gg, g2):
        torch.testing.assert_close(a, b, rtol=1e-4, atol=1e-5, msg=k)


def _graphs_per_panel(sizes):
    gp = np.concatenate([[0], np.cumsum(sizes)])
    R = int(gp[-1])
    first = lambda r: int(np.searchsorted(gp, r, side="right")) - 1         # the graph that holds row r
    return [first(min(p + 32, R) - 1) - first(p) + 1 for p in range(0, R, 32)]


@pytest.mark.parametrize("fin,hid,L", [(5, 32, 3), (16, 64, 2)])
def test_sage_net_many_small_graphs(fin, hid, L):
    """a batch of 1- to 6-node graphs: 32-row panels that span 4 to 32 graphs (the post epilogue's loop beyond its first three
    prefetched graphs), with one panel of exactly 3 graphs followed by one of 4"""
    rng = np.random.default_rng(3)
    sizes = [10, 11, 11, 8, 8, 8, 8] + [1] * 32 + list(rng.integers(1, 7, size=150))
    per = _graphs_per_panel(sizes)
    assert per[0] == 3 and per[1] == 4 and per[2] == 32 and max(per[3:]) >= 8, per
    _sage_net_case(tuple(int(s) for s in sizes), fin, hid, L, seed=70 + L)
