"""pyg.SagePoolNet as ONE sync-free node: the GraphConv-scorer forms of the per-graph SAGPool kernels (csrc/sagpool.hip,
tsgnn_sag_pool_graph_gc_f32 / _gc_bwd_f32), sag_stack_sage._SagSageStack(scorer="graphconv") and the routing of SagePoolNet onto it.

  - the kernel pair against a torch restatement (float64) on graphs of 1 .. 1,100 nodes, every lane-group width;
  - fused == composed (fused=False) on the config-4 batch and a small multi-feature batch: log-probabilities, last_perms, gradients;
  - three replayed optimiser steps (FlatTrainer + GraphedStep) against oracle/pyg_ref.sage_pool_net + Adam (fp32, fp64);
  - a resident input refilled between graph replays is followed (SagePoolNet and sag_layers.Net(conv="sage"));
  - inputs the node does not take (min_score, multiplier, directed edge lists, graphs above the kernel's node limit) stay composed.
PARITY UNPINNED (no torch_geometric in the reference tree): the oracle restates PyG's documented formulas."""
import numpy as np
import pytest
import torch

from oracle import pyg_ref as P
from test_gpu_pyg import grads, rand_graph, tie_free

pytestmark = pytest.mark.gpu


class _D:
    pass


def _data(x, ei, batch, dev="cuda", x_grad=False):
    d = _D()
    d.x = x.to(dev).requires_grad_(x_grad)
    d.edge_index, d.batch = ei.to(dev), batch.to(dev)
    return d


def _small_batch(seed, sizes, fin, e_per_node=2.2):
    n = int(sum(sizes))
    ei = rand_graph(seed, n, int(e_per_node * n), True, list(sizes))
    batch = torch.repeat_interleave(torch.arange(len(sizes)), torch.tensor(list(sizes)))
    return tie_free(seed + 1, n, fin), ei, batch


def _imdb(x_seed=5):
    from test_gpu_fullsize import _imdb_batch
    _, x, ei, batch, lab = _imdb_batch(x_seed)
    return x, ei, batch, lab


# ------------------------------------------------------------------------------------------------ 1. the kernel pair
def _level_case(case, F):
    """sizes, symmetric edge list with a few self loops (GraphConv sums them as neighbours), tie-free y"""
    if case == "mixed":
        sizes = [1, 2, 37, 300, 1100]                       # > 256 nodes: 1,024-thread blocks; > 1,024: the bitonic sort
    else:
        sizes = list(1 + (np.arange(600) * 7919) % 40)      # > 2 workgroups per CU, all <= 256 nodes: 256-thread blocks
    n = int(sum(sizes))
    ei = rand_graph(100 + F, n, 3 * n, True, sizes)
    loops = torch.arange(0, n, 7)
    ei = torch.cat([ei, torch.stack([loops, loops])], 1)
    y = tie_free(200 + F, n, F)
    return np.asarray(sizes, dtype=np.int64), ei, y


@pytest.mark.parametrize("case,F", [("mixed", 8), ("mixed", 32), ("mixed", 64), ("mixed", 128), ("many", 32)])
def test_graphconv_pool_kernels_vs_torch(case, F):
    from two_stage_gnn_amd import _native as nat, message_passing as mp, sag_stack as SS
    from two_stage_gnn_amd.graph import GraphBatch
    dev = torch.device("cuda")
    sizes, ei, y = _level_case(case, F)
    n = int(sizes.sum())
    g = GraphBatch.from_edge_index(ei.to(dev), n, ghosts=False)
    plan = SS.SagPlan.get(sizes, 0.5, dev, depth=1)
    L, Ln = plan.levels[0], plan.levels[1]
    B, K = L.B, Ln.N
    gen = torch.Generator().manual_seed(F)
    w_rel, w_root, b = torch.randn(F, generator=gen), torch.randn(F, generator=gen), torch.randn(1, generator=gen)
    yd = y.to(dev)
    i32 = lambda *s: torch.empty(*s, dtype=torch.int32, device=dev)
    score = torch.empty(n, device=dev); perm, new_id, cnt = i32(K), i32(n), i32(K)
    xp = torch.empty(K, F, device=dev); out = torch.empty(B, 2 * F, device=dev); arg = i32(B, F)
    rp_n, re_n = i32(K), i32(K)
    col_n = torch.full((int(g.col.numel()),), -7, dtype=torch.int32, device=dev)
    nat.call("sag_pool_graph_gc_f32", yd, F, g.rowptr, None, g.col, w_rel.to(dev), w_root.to(dev), b.to(dev), L.gp, Ln.gp, B, L.max_seg, F,
             score, perm, new_id, xp, F, cnt, out, 2 * F, arg, 0, rp_n, re_n, col_n)
    torch.cuda.synchronize()
    src, dst = ei[0], ei[1]
    # score = w_rel . sum_{j -> i} relu(y_j) + w_root . relu(y_i) + b
    r64 = torch.relu(y.double())
    t, u = r64 @ w_rel.double(), r64 @ w_root.double()
    s_ref = torch.zeros(n, dtype=torch.float64).index_add_(0, dst, t[src]) + u + b.double()
    sc = score.cpu()
    scale = float((torch.zeros(n, dtype=torch.float64).index_add_(0, dst, t[src].abs()) + u.abs()).max())
    assert float((sc.double() - s_ref).abs().max()) <= 1e-5 * scale
    # top-k from the kernel's own fp32 scores: descending inside a graph, ties -> smaller row
    graph = np.repeat(np.arange(B), sizes)
    order = np.lexsort((np.arange(n), -sc.numpy().astype(np.float64), graph))
    gp, gpn = L.gp.cpu().numpy(), Ln.gp.cpu().numpy()
    perm_ref = np.concatenate([order[gp[i]: gp[i] + (gpn[i + 1] - gpn[i])] for i in range(B)])
    assert np.array_equal(perm.cpu().numpy(), perm_ref)
    nid_ref = np.full(n, -1); nid_ref[perm_ref] = np.arange(K)
    assert np.array_equal(new_id.cpu().numpy(), nid_ref)
    # gated gather and the max || mean readout (arg: the kept row holding the max, ties -> smallest)
    pr = torch.from_numpy(perm_ref)
    xp_ref = torch.relu(y)[pr] * torch.tanh(sc[pr]).unsqueeze(1)
    torch.testing.assert_close(xp.cpu(), xp_ref, rtol=1e-6, atol=1e-6)
    xh, oh, ah = xp.cpu(), out.cpu(), arg.cpu()
    for i in range(B):
        rows = xh[gpn[i]: gpn[i + 1]]
        mx = rows.max(0).values
        assert torch.equal(oh[i, :F], mx)
        torch.testing.assert_close(oh[i, F:], rows.double().mean(0).float(), rtol=1e-5, atol=1e-6)
        first = (rows == mx.unsqueeze(0)).int().argmax(0) + int(gpn[i])
        assert torch.equal(ah[i].long(), first)
    # filter_adj: row p = the kept neighbours of perm[p], relabelled, in their original order; cnt = row lengths
    rp, col = g.rowptr.cpu().numpy(), g.col.cpu().numpy()
    rpn, ren, cn, cnth = rp_n.cpu().numpy(), re_n.cpu().numpy(), col_n.cpu().numpy(), cnt.cpu().numpy()
    for p in range(K):
        r = perm_ref[p]
        ids = nid_ref[col[rp[r]: rp[r + 1]]]
        want = ids[ids >= 0]
        assert np.array_equal(cn[rpn[p]: ren[p]], want), p
        assert cnth[p] == want.size
    iv = sorted(zip(rpn.tolist(), ren.tolist()))                        # rows inside col_new, none overlapping another
    assert iv[0][0] >= 0 and iv[-1][1] <= len(cn) and all(e0 <= s1 for (_, e0), (s1, _) in zip(iv, iv[1:]))
    # backward against autograd on the restatement with the kernel's discrete choices (perm, arg)
    gen = torch.Generator().manual_seed(F + 1)
    dxp, dread = torch.randn(K, F, generator=gen), torch.randn(B, 2 * F, generator=gen)
    du = torch.empty(n, F, device=dev)
    part = torch.full((B * (2 * F + 4),), float("nan"), device=dev)
    nat.call("sag_pool_graph_gc_bwd_f32", yd, F, score, new_id, L.gp, Ln.gp, arg, dxp.to(dev), F, dread.to(dev), 2 * F, g.rowptr, None,
             g.col, w_rel.to(dev), w_root.to(dev), B, L.max_seg, F, du, F, part)
    dwrel, dwroot, db = torch.zeros(1, F, device=dev), torch.zeros(1, F, device=dev), torch.zeros(1, device=dev)
    mp.wgrad_reduce([mp.wgrad_set(part, B, 0, 2 * F + 4, dwroot, dwrel, n_db=F, tail=db, lddw=F + 4)])
    torch.cuda.synchronize()
    yv = y.double().requires_grad_(True)
    wl, wr, bb = w_rel.double().requires_grad_(True), w_root.double().requires_grad_(True), b.double().requires_grad_(True)
    r = torch.relu(yv)
    s = torch.zeros(n, dtype=torch.float64).index_add(0, dst, (r @ wl)[src]) + r @ wr + bb
    xq = r[pr] * torch.tanh(s[pr]).unsqueeze(1)
    mxq = xq.gather(0, ah.long())
    kb = torch.from_numpy(np.diff(gpn)).double()
    mean = torch.zeros(B, F, dtype=torch.float64).index_add(0, torch.from_numpy(np.repeat(np.arange(B), np.diff(gpn))), xq) / kb.unsqueeze(1)
    loss = (xq * dxp.double()).sum() + (mxq * dread[:, :F].double()).sum() + (mean * dread[:, F:].double()).sum()
    gy, gwl, gwr, gb = torch.autograd.grad(loss, [yv, wl, wr, bb])
    for name, got, want in (("du", du, gy), ("dw_rel", dwrel.view(-1), gwl), ("dw_root", dwroot.view(-1), gwr), ("db", db, gb)):
        err = float((got.cpu().double() - want).abs().max())
        assert err <= 2e-5 * (float(want.abs().max()) + 1e-30), (name, err, float(want.abs().max()))


# ------------------------------------------------------------------------------------------------ helpers: the oracle's ambiguous graphs
def _ambiguous_graphs_gc(p, x, ei, batch, ratio, tol=1e-4, twins_ok=True):
    """fp64 oracle, level by level: the graphs whose top-k has no defined answer for SagePoolNet (GraphConv scorer): scores within
    `tol` of the last kept score (relative to the graph's largest |score|) on both sides of the cut — unless the tied nodes are true
    twins (equal feature rows and closed neighbourhoods: either choice gives the same outputs) and twins_ok"""
    B = int(batch.max()) + 1
    bad = torch.zeros(B, dtype=torch.bool)
    for i in range(3):
        x = torch.relu(P.sage_conv(x, ei, p["convs.%d.lin_l.weight" % i], p["convs.%d.lin_l.bias" % i], p["convs.%d.lin_r.weight" % i]))
        wl, bl, wr = p["pools.%d.gnn.lin_l.weight" % i], p["pools.%d.gnn.lin_l.bias" % i], p["pools.%d.gnn.lin_r.weight" % i]
        score = P.graph_conv(x, ei, wl, bl, wr).view(-1)
        n = x.size(0)
        A = torch.eye(n, dtype=torch.bool)
        A[ei[1], ei[0]] = True
        for b in range(B):
            idx = (batch == b).nonzero().view(-1)
            s = score[idx]
            k = int(np.ceil(np.float32(ratio) * np.float32(s.numel())))
            if k >= s.numel():
                continue
            order = torch.argsort(s, descending=True)
            rank = torch.empty_like(order)
            rank[order] = torch.arange(order.numel())
            near = (s - s[order[k - 1]]).abs() <= tol * (float(s.abs().max()) + 1e-30)
            if not (int(rank[near].min()) < k <= int(rank[near].max())):
                continue
            tied = idx[near]
            xs = x[tied]
            twins = (float((xs - xs[0]).abs().max()) <= 1e-9 * (float(xs.abs().max()) + 1e-30)) and bool((A[tied] == A[tied[0]]).all())
            if not (twins and twins_ok):
                bad[b] = True
        x, ei, batch, _, _ = P.sag_pooling(x, ei, batch, ratio, wl, bl, wr)
    return bad


def _params64(net):
    return {k: v.detach().cpu().double() for k, v in net.state_dict().items()}


# ------------------------------------------------------------------------------------------------ 2. fused == composed
@pytest.mark.parametrize("which", ["imdb_b128", "small_f7"])
def test_sagepoolnet_fused_equals_composed(which):
    from two_stage_gnn_amd import pyg
    if which == "imdb_b128":
        x, ei, batch, lab = _imdb()
        fin, hid, need = 1, 128, 80
    else:
        x, ei, batch = _small_batch(51, (18, 30, 9, 41, 17, 26, 60, 5), 7)
        lab = torch.arange(8) % 2
        fin, hid, need = 7, 64, 5
    B = int(batch.max()) + 1
    torch.manual_seed(3)
    net = pyg.SagePoolNet(fin, hid, 2, pooling_ratio=0.5).cuda().train()
    d = _data(x, ei, batch, x_grad=True)
    assert net.fused_route(d) is not None
    with torch.no_grad():
        bad = _ambiguous_graphs_gc(_params64(net), x.double(), ei, batch, 0.5, twins_ok=False)
    ok = ~bad
    assert int(ok.sum()) >= need, int(ok.sum())
    w = ok.float().cuda()
    names = [k for k, _ in net.named_parameters()]
    params = [p for _, p in net.named_parameters()]
    runs = []
    for fused in (True, False):
        net.fused = fused
        y = net(d)
        perms = net.last_perms
        loss = -(y.gather(1, lab.cuda().view(-1, 1)).squeeze(1) * w).sum() / w.sum()
        runs.append((y.detach(), perms, grads(loss, params + [d.x])))
    (yf, pf, gf), (yc, pc, gc) = runs
    assert all(p.dtype == torch.int64 for p in pf)
    torch.testing.assert_close(yf[ok.cuda()], yc[ok.cuda()], rtol=1e-5, atol=1e-5)
    # last_perms: the same kept rows per graph (as sets), grouped by graph, descending score inside a graph on both paths
    bf = bc = batch
    for lvl, (a, c) in enumerate(zip(pf, pc)):
        a, c = a.cpu(), c.cpu()
        assert a.shape == c.shape, lvl
        assert torch.equal(bf[a], bc[c]), lvl                              # the same graph layout
        for b in ok.nonzero().view(-1).tolist():
            assert set(a[bf[a] == b].tolist()) == set(c[bc[c] == b].tolist()), (lvl, b)
        bf, bc = bf[a], bc[c]
    for k, a, c in zip(names + ["x"], gf, gc):
        scale = float(c.abs().max()) + 1e-30
        err = float((a - c).abs().max())
        assert err <= 1e-4 * scale, (which, k, err, scale)


# ------------------------------------------------------------------------------------------------ 3. replayed steps vs the oracle
def test_sagepoolnet_graphed_steps_vs_oracle():
    """BASELINE config 4 as PyG words it (SAGPooling with its GraphConv scorer + SAGEConv, IMDB-B b128, h 128) as the timed step:
    FlatTrainer + GraphedStep, three replayed optimiser steps against oracle/pyg_ref.sage_pool_net + clip + Adam in fp32 / fp64.
    Graphs whose top-k is ambiguous for the fp64 oracle's current parameters get weight 0 on both sides; >= 80 of 128 must count."""
    from test_gpu_fullsize import _run
    from two_stage_gnn_amd import pyg
    dev = torch.device("cuda")
    torch.manual_seed(0)
    net = pyg.SagePoolNet(1, 128, 2, pooling_ratio=0.5).to(dev).train()
    x, ei, batch, lab = _imdb()
    d = _data(x, ei, batch)
    # the one-node route BEFORE any capture: the composed path's host round trips cannot be captured
    assert net.fused_route(d) is not None
    label = lab.to(dev)
    w_cpu = torch.ones(128, dtype=torch.float64)
    w_dev = torch.ones(128, dtype=torch.float32, device=dev)
    counted = []

    def weighted(dtype):
        xx = x.to(dtype)

        def f(p):
            y = P.sage_pool_net(p, xx, ei, batch, 0.5)
            w = w_cpu.to(dtype)
            return -(y.gather(1, lab.view(-1, 1)).squeeze(1) * w).sum() / w.sum(), y * w.view(-1, 1)
        return f

    def loss_fn(stash):
        y = net(d)
        stash["logits"] = y * w_dev.view(-1, 1)
        return -(y.gather(1, label.view(-1, 1)).squeeze(1) * w_dev).sum() / w_dev.sum()

    def mask(i, p64):
        with torch.no_grad():
            bad = _ambiguous_graphs_gc({k: v.detach() for k, v in p64.items()}, x.double(), ei, batch, 0.5)
        w_cpu.copy_((~bad).double())
        w_dev.copy_((~bad).float().to(dev))
        torch.cuda.synchronize()
        counted.append(int((~bad).sum()))
        assert counted[-1] >= 80, counted

    _run(net, loss_fn, weighted(torch.float32), weighted(torch.float64), lr=5e-4, max_frac=0.05,
         tag="SagePoolNet IMDB-B b128 (tie-free features)", pre_step=mask)
    print("graphs counted per step:", counted)


# ------------------------------------------------------------------------------------------------ 4. refilled inputs
@pytest.mark.parametrize("model", ["sag_layers_sage", "sagepoolnet"])
def test_refilled_features_are_followed_by_replays(model):
    """GraphedStep's contract: refill the resident input between replays.  The replayed steps must see each new x: losses and
    parameters after every replay equal those of an eager twin fed the same sequence"""
    from two_stage_gnn_amd import pyg, sag_layers as S
    from two_stage_gnn_amd.data_parallel import FlatTrainer, GraphedStep
    dev = torch.device("cuda")
    sizes = (18, 30, 9, 41, 17, 26)
    x0, ei, batch = _small_batch(61, sizes, 7)
    lab = (torch.arange(len(sizes)) % 2).to(dev)

    def make():
        torch.manual_seed(7)
        if model == "sagepoolnet":
            return pyg.SagePoolNet(7, 64, 2, pooling_ratio=0.5).to(dev).train()
        return S.Net(7, 64, 2, 0.5, 0.0, use_batch=True, conv="sage").to(dev).train()
    nets = [make(), make()]
    ds = [_data(x0, ei, batch), _data(x0, ei, batch)]
    if model == "sagepoolnet":
        assert all(n.fused_route(d) is not None for n, d in zip(nets, ds))
    else:
        assert all(n._fused_ok() for n in nets)
    trainers = [FlatTrainer(n, lr=1e-2, clip=2.0) for n in nets]
    fns = [lambda n=n, d=d: torch.nn.functional.nll_loss(n(d), lab) for n, d in zip(nets, ds)]
    gs = GraphedStep(trainers[0], fns[0], warmup=3)
    assert gs.describe().startswith("one graph"), gs.describe()
    for i in range(4):
        xi = tie_free(300 + i, x0.size(0), 7).to(dev) * (1.0 + i)
        for d in ds:
            d.x.copy_(xi)
        gs.step()
        l_graph = gs.loss_value()
        l_eager = float(trainers[1].step(fns[1]))
        assert abs(l_graph - l_eager) <= 1e-5 * max(1.0, abs(l_eager)), (model, i, l_graph, l_eager)
        for (k, a), b in zip(nets[0].named_parameters(), nets[1].parameters()):
            scale = float(b.detach().abs().max()) + 1e-30
            assert float((a.detach() - b.detach()).abs().max()) <= 1e-5 * scale, (model, i, k)


# ------------------------------------------------------------------------------------------------ 5. routing
@pytest.mark.parametrize("case", ["min_score", "multiplier", "directed", "large_graph"])
def test_sagepoolnet_unsupported_inputs_stay_composed(case):
    from two_stage_gnn_amd import _native as nat, pyg
    if case == "large_graph":
        big = int(nat.lib().tsgnn_sag_pool_graph_max_nodes()) + 37
        sizes = (big, 12, 30)
        x, ei, batch = _small_batch(71, sizes, 3, e_per_node=1.5)
    else:
        sizes = (18, 30, 9, 41)
        n = sum(sizes)
        x, ei, batch = _small_batch(71, sizes, 3)
        if case == "directed":
            ei = rand_graph(72, n, 2 * n, False, list(sizes))
    torch.manual_seed(9)
    net = pyg.SagePoolNet(3, 32, 2, pooling_ratio=0.5).cuda().eval()
    if case == "min_score":
        net.pools[1].min_score = 0.05
    elif case == "multiplier":
        net.pools[2].multiplier = 2
    d = _data(x, ei, batch)
    assert net.fused_route(d) is None
    y1 = net(d)
    p1 = [p.clone() for p in net.last_perms]
    net.fused = False
    y2 = net(d)
    if case == "min_score":                                # (the composed softmax's segment sums: index_add, atomics)
        torch.testing.assert_close(y1, y2, rtol=1e-6, atol=1e-7)
    else:
        assert torch.equal(y1, y2)
    assert all(torch.equal(a, b) for a, b in zip(p1, net.last_perms))
