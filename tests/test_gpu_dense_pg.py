"""The pooled-level GCN layers under per-graph statistics (csrc/dense_stack_pg.hip, dense_stack_pg.py) and DiffPool's two-stage path
on them: the kernels one by one through the C ABI against the float64 reference (tests/dense_pg_ref.py, yardstick: the same code
in CPU float32, fp32_yardstick.py), the autograd node against the composed per-op path and float64, the triplet step against the
oracle's three B = 1 forwards, the replayed step against eager steps, and embed_dataset against the oracle's eval forwards."""
import copy
import itertools

import numpy as np
import pytest
import torch

import dense_pg_ref as PG
import fp32_yardstick as Y
from guard_buf import Out, _owned
from oracle import dense_ref as R
from util_graphs import dense_batch

pytestmark = pytest.mark.gpu

BK = [(1, 4), (3, 20), (2, 36), (3, 100)]               # (3, 20): a partial second tile; (3, 100): the two-stage default K
FN = [(4, 4), (12, 8), (20, 100), (192, 64)]


def _nat():
    from two_stage_gnn_amd import _native as nat
    return nat


def _wide(t, ld):
    """the rows of t inside a wider device matrix (leading dimension ld)"""
    buf = torch.zeros(t.size(0), ld, device="cuda")
    buf[:, :t.size(1)] = t.cuda()
    return buf


def _full(rows, ld):
    return torch.ones(rows, ld, dtype=torch.bool)


def _refs(seed, B, K, fin, n, bias, hidden):
    """(operands, forward outputs) in float64 and in CPU float32"""
    out = []
    for dt in (torch.float64, torch.float32):
        ops = PG.inputs(seed, B, K, fin, n, bias, dt)
        out.append((ops, PG.layer_fwd(*ops, hidden)))
    return out


@pytest.mark.parametrize("fin,n", FN)
@pytest.mark.parametrize("B,K", BK)
def test_layer_forward_kernel_against_fp64(B, K, fin, n):
    nat = _nat()
    R_ = B * K
    for hidden, bias in itertools.product((True, False), (True, False)):
        (ops64, f64), (ops32, f32) = _refs(B * 1000 + K + fin + n, B, K, fin, n, bias, hidden)
        x, adj, w, b = ops64
        u = f64[0] @ w + (b if b is not None else 0.0)
        assert u.norm(dim=2).min().item() >= 1e-3                     # the reference's rounding is the yardstick, not a cancellation
        tag = "fwd B%d K%d fin%d n%d hidden%d bias%d " % (B, K, fin, n, hidden, bias)
        xd, wd = _wide(x.float().reshape(R_, fin), fin + 4), _wide(w.float(), n + 4)
        y, agg, v, rinv, mean, rstd = Out(R_, n + 8), Out(R_, fin), Out(R_, n), Out(R_, 1), Out(R_, 1), Out(R_, 1)
        nat.call("dense_pg_layer_fwd_f32", xd, fin + 4, adj.float().cuda(), wd, n + 4, None if b is None else b.float().cuda(), B, K, fin, n,
                 int(hidden), agg.mat, v.mat if hidden else None, rinv.mat, mean.mat if hidden else None, rstd.mat if hidden else None,
                 y.mat[:, 4:], n + 8)
        y.rest_untouched(tag + "y", _owned(R_, n + 8, 0, R_, 4, 4 + n))
        for name, o, i, width in (("agg", agg, 0, fin), ("v", v, 1, n), ("rinv", rinv, 2, 1), ("mean", mean, 3, 1), ("rstd", rstd, 4, 1)):
            kept = hidden or name in ("agg", "rinv")
            o.rest_untouched(tag + name, _full(R_, width) if kept else torch.zeros(R_, width, dtype=torch.bool))
            if kept:
                Y._check(tag + name, o.mat, f64[i].reshape(R_, width), f32[i].reshape(R_, width))
        Y._check(tag + "y", y.mat[:, 4:4 + n], f64[5].reshape(R_, n), f32[5].reshape(R_, n))


def _bwd_ref(dt, seed, B, K, fin, n, bias, hidden, dcat, dnext, base):
    x, adj, w, b = PG.inputs(seed, B, K, fin, n, bias, dt)
    leaves = [t for t in (x, adj, w, b) if t is not None]
    for t in leaves:
        t.requires_grad_(True)
    agg, v, rinv, mean, rstd, y = PG.layer_fwd(x, adj, w, b, hidden)
    agg.retain_grad()
    dy = dcat.to(dt)
    if dnext is not None:
        dy = dy + adj.detach().transpose(1, 2) @ dnext.to(dt)        # the input gradient of the layer above
    y.backward(dy)
    dadj = adj.grad if base is None else adj.grad + base.to(dt)
    return {"dagg": agg.grad, "dadj": dadj, "dw": w.grad, "db": None if b is None else b.grad, "dx": x.grad}


@pytest.mark.parametrize("fin,n", FN)
@pytest.mark.parametrize("B,K", BK)
def test_layer_backward_kernels_against_fp64(B, K, fin, n):
    nat = _nat()
    from two_stage_gnn_amd import message_passing as mp
    R_ = B * K
    nslab = B * ((K + 15) // 16)
    gen = torch.Generator().manual_seed(B + K + fin + n)
    seed = B * 1000 + K + fin + n
    for hidden, bias in itertools.product((True, False), (True, False)):
        (ops64, f64), _ = _refs(seed, B, K, fin, n, bias, hidden)
        x, adj, w, b = ops64
        agg, v, rinv, mean, rstd, _y = f64
        dev = lambda t: t.float().cuda().contiguous()
        xd, wd, adjd = _wide(x.float().reshape(R_, fin), fin + 4), _wide(w.float(), n + 4), dev(adj)
        aggd, vd, rinvd = dev(agg.reshape(R_, fin)), _wide(v.float().reshape(R_, n), n + 4), dev(rinv.reshape(R_))
        meand, rstdd = (dev(mean.reshape(R_)), dev(rstd.reshape(R_))) if hidden else (None, None)
        for above, acc, want_dx in itertools.product((False, True), (False, True), (False, True)):
            dcat = torch.randn(B, K, n, generator=gen).double()
            dnext = torch.randn(B, K, n, generator=gen).double() if above else None
            base = torch.randn(B, K, K, generator=gen).double() if acc else None
            r64 = _bwd_ref(torch.float64, seed, B, K, fin, n, bias, hidden, dcat, dnext, base)
            r32 = _bwd_ref(torch.float32, seed, B, K, fin, n, bias, hidden, dcat, dnext, base)
            tag = "bwd B%d K%d fin%d n%d hidden%d bias%d above%d acc%d dx%d " % (B, K, fin, n, hidden, bias, above, acc, want_dx)
            dcatd = Out(R_, n + 8)
            dcatd.mat.zero_()
            dcatd.mat[:, 4:4 + n] = dcat.float().reshape(R_, n).cuda()
            dagg = Out(R_, fin) if want_dx else None
            slab, dadj = Out(nslab * (fin + 1), n), Out(R_, K)
            if acc:
                dadj.mat.copy_(base.float().reshape(R_, K).cuda())
            nat.call("dense_pg_layer_bwd_f32", adjd, wd, n + 4, aggd, vd, n + 4, rinvd, meand, rstdd, xd, fin + 4, dcatd.mat[:, 4:], n + 8,
                     None if dnext is None else dev(dnext.reshape(R_, n)), B, K, fin, n, int(hidden), None if dagg is None else dagg.mat,
                     slab.mat, dadj.mat, int(acc))
            slab.rest_untouched(tag + "slab", _full(nslab * (fin + 1), n))
            dadj.rest_untouched(tag + "dadj", _full(R_, K))
            Y._check(tag + "dadj", dadj.mat, r64["dadj"].reshape(R_, K), r32["dadj"].reshape(R_, K))
            dw, db = Out(fin, n), (Out(1, n) if bias else None)
            mp.wgrad_reduce([mp.wgrad_set(slab.mat, nslab, fin, n, dw.mat, None if db is None else db.mat, kn=1, lddw=n)])
            dw.rest_untouched(tag + "dw", _full(fin, n))
            Y._check(tag + "dw", dw.mat, r64["dw"], r32["dw"])
            if bias:
                db.rest_untouched(tag + "db", _full(1, n))
                Y._check(tag + "db", db.mat, r64["db"].reshape(1, n), r32["db"].reshape(1, n))
            if want_dx:
                dagg.rest_untouched(tag + "dagg", _full(R_, fin))
                Y._check(tag + "dagg", dagg.mat, r64["dagg"].reshape(R_, fin), r32["dagg"].reshape(R_, fin))
                dx = Out(R_, fin + 4)
                nat.call("dense_pg_dx_f32", adjd, dev(r64["dagg"].reshape(R_, fin)), B, K, fin, dx.mat, fin + 4)
                dx.rest_untouched(tag + "dx", _owned(R_, fin + 4, 0, R_, 0, fin))
                Y._check(tag + "dx", dx.mat[:, :fin], r64["dx"].reshape(R_, fin), r32["dx"].reshape(R_, fin))


# ----------------------------------------------------------------------------- the node
class _A:
    bias = True


def _encoder(nmax, fin, L, num_pooling=1, seed=4, ratio=0.25):
    from two_stage_gnn_amd import dense_encoders as E
    torch.manual_seed(seed)
    m = E.SoftPoolingGcnEncoder(nmax, fin, 8, 8, 2, L, 8, assign_ratio=ratio, num_pooling=num_pooling, bn=True, linkpred=False, args=_A(),
                                assign_input_dim=fin, final_dim="output_dim")
    with torch.no_grad():
        for k, p in m.named_parameters():
            if "conv" in k and k.endswith("bias"):
                p.copy_(torch.randn_like(p) * 0.3)
    return m.cuda()


def _pooled_run(m, x, adj, G, flag):
    """the pooled-level embedding stack of m on (x, adj) with per-graph statistics -> (out, dx, dadj, parameter gradients, trace)"""
    from two_stage_gnn_amd import dense_encoders as E
    nat = _nat()
    convs = m.conv_stack(1)
    params = [p for c in convs for p in (c.weight, c.bias)]
    xg, ag = x.clone().requires_grad_(True), adj.clone().requires_grad_(True)
    old, m.per_graph_bn, nat.trace = E.PER_GRAPH_DENSE, True, []
    E.PER_GRAPH_DENSE = flag
    try:
        out, _ = m.gcn_forward_dense(xg, ag, convs[0], convs[1:-1], convs[-1])
        grads = torch.autograd.grad((out * G).sum(), [xg, ag] + params)
        trace = [t[0] for t in nat.trace]
    finally:
        E.PER_GRAPH_DENSE, m.per_graph_bn, nat.trace = old, False, None
    return out.detach(), grads[0], grads[1], grads[2:], trace, convs


@pytest.mark.parametrize("L", [2, 3, 4])
def test_node_equals_the_composed_path_and_fp64(L):
    B, K = 3, 20
    m = _encoder(80, 12, L)
    fin = m.pred_input_dim
    gen = torch.Generator().manual_seed(L)
    x = torch.randn(B, K, fin, generator=gen).cuda()
    adj = (torch.rand(B, K, K, generator=gen) * 0.9 + 0.1).cuda()
    G = torch.randn(B, K, fin, generator=gen).cuda()
    out, dx, dadj, gp, trace, convs = _pooled_run(m, x, adj, G, True)
    assert trace.count("dense_pg_layer_fwd_f32") == L and trace.count("dense_pg_layer_bwd_f32") == L and trace.count("dense_pg_dx_f32") == 1
    node = [t for t in trace if t != "row_maps"]                    # (row_maps: the uniform GraphBatch gcn_forward_dense returns beside the output)
    assert trace.count("wgrad_reduce_sets_f32") == 1 and len(node) == 2 * L + 2         # L forward, L + 1 backward launches + one reduction
    out0, dx0, dadj0, gp0, trace0, _ = _pooled_run(m, x, adj, G, False)
    assert "dense_pg_layer_fwd_f32" not in trace0 and "row_ln_fwd_f32" in trace0
    print("L = %d: library launches of the pooled stack, forward + backward: %d (node) / %d (composed)" % (L, len(trace), len(trace0)))
    torch.testing.assert_close(out, out0, rtol=1e-5, atol=1e-6)
    refs = []
    for dt in (torch.float64, torch.float32):
        leaves = [x.cpu().to(dt).requires_grad_(True), adj.cpu().to(dt).requires_grad_(True)]
        ps = [(c.weight.detach().cpu().to(dt).requires_grad_(True), c.bias.detach().cpu().to(dt).requires_grad_(True)) for c in convs]
        y = PG.stack_fwd(leaves[0], leaves[1], ps)
        refs.append((y.detach(), torch.autograd.grad((y * G.cpu().to(dt)).sum(), leaves + [t for wb in ps for t in wb])))
    (y64, g64), (y32, g32) = refs
    Y._check("L%d out" % L, out, y64, y32)
    names = ["dx", "dadj"] + ["%s%d" % (k, l) for l in range(L) for k in ("dW", "db")]
    for name, got, a, b in zip(names, (dx, dadj) + tuple(gp), g64, g32):
        Y._check("L%d %s" % (L, name), got, a, b)
    with torch.no_grad():                                            # forward only: nothing is kept for a backward
        from two_stage_gnn_amd import dense_stack_pg
        y = dense_stack_pg.dense_gcn_stack_pg(x, adj, convs)
    assert y.grad_fn is None and torch.equal(y, out)


def test_node_writes_weight_gradients_into_the_flat_bucket():
    """under a FlatTrainer every weight and bias gradient of the node lands in the parameter's slice of the flat bucket: nothing
    reaches ``.grad`` (no AccumulateGrad copy), the slices hold what a plain backward returns"""
    from two_stage_gnn_amd import dense_stack_pg, message_passing as mp
    from two_stage_gnn_amd.data_parallel import FlatTrainer
    B, K, L = 3, 20, 3
    m = _encoder(80, 12, L)
    convs = torch.nn.ModuleList(m.conv_stack(1))
    gen = torch.Generator().manual_seed(9)
    x = torch.randn(B, K, m.pred_input_dim, generator=gen).cuda().requires_grad_(True)
    adj = (torch.rand(B, K, K, generator=gen) * 0.9 + 0.1).cuda().requires_grad_(True)
    G = torch.randn(B, K, m.pred_input_dim, generator=gen).cuda()
    loss = lambda: (dense_stack_pg.dense_gcn_stack_pg(x, adj, list(convs)) * G).sum()
    params = list(convs.parameters())
    plain = torch.autograd.grad(loss(), params)
    tr = FlatTrainer(convs, lr=1e-3, clip=2.0)
    try:
        tr.zero_grad()
        tr.backward(loss())
        assert mp.GRAD_SINK is tr.sink
        for p, want in zip(tr.params, plain):
            assert p.grad is None and p.data_ptr() in tr.sink.written
            assert torch.equal(tr.sink.views[p.data_ptr()], want)
        assert x.grad is not None and adj.grad is not None
    finally:
        tr.gather_grads()
        mp.GRAD_SINK = None


# ----------------------------------------------------------------------------- the triplet step
class _G:                       # stand-in for the networkx graphs cross_val.split_train_val prepares (cross_val.py:158-184)
    def __init__(self, adj, feats, n, label=0):
        self.graph = {"adj": adj, "feats": feats, "num_nodes": n, "assign_feats": feats, "label": label}


def _triplet_trace(net, gs, stack, dense):
    from two_stage_gnn_amd import dense_encoders as E
    nat = _nat()
    old = (E.PER_GRAPH_STACK, E.PER_GRAPH_DENSE)
    E.PER_GRAPH_STACK, E.PER_GRAPH_DENSE, nat.trace = stack, dense, []
    try:
        net.model.zero_grad(set_to_none=True)
        dp, dn, ea, ep, en = net(*gs)
        torch.nn.MarginRankingLoss(margin=1.0)(dp, dn, torch.tensor([-1.0]).cuda()).backward()
        trace = list(nat.trace)
    finally:
        (E.PER_GRAPH_STACK, E.PER_GRAPH_DENSE), nat.trace = old, None
    return (dp, dn, ea, ep, en), trace


@pytest.mark.parametrize("nmax,num_pooling,sizes", [(32, 1, [32, 11, 17]), (64, 2, [64, 23, 37])])
def test_triplet_step_equals_three_b1_forwards(nmax, num_pooling, sizes):
    """triplet.tripletnet over SoftPoolingGcnEncoder (K = 8; with two levels K = 16, 4) against the oracle's three B = 1 forwards at
    test_triplet_batched_equals_three_b1_forwards' own bounds, on the per-graph launches of every pooled stack"""
    from two_stage_gnn_amd.triplet import tripletnet
    fin = 8
    x, adj, sizes = dense_batch(41 + num_pooling, 3, nmax, fin, sizes=sizes, p_edge=0.2)
    m = _encoder(nmax, fin, 3, num_pooling=num_pooling)
    p_ref = {k: v.detach().cpu().clone().requires_grad_(True) for k, v in m.state_dict().items()}
    embeds = [R.diffpool_encoder(p_ref, x[b:b + 1], adj[b:b + 1], sizes[b:b + 1], num_pooling, assign_x=x[b:b + 1], final_dim="output_dim")[1]
              for b in range(3)]
    dp_ref = torch.nn.functional.pairwise_distance(embeds[0], embeds[1], 2)
    dn_ref = torch.nn.functional.pairwise_distance(embeds[0], embeds[2], 2)
    torch.nn.MarginRankingLoss(margin=1.0)(dp_ref, dn_ref, torch.tensor([-1.0])).backward()
    net = tripletnet(m)
    gs = [_G(adj[b].numpy(), x[b].numpy(), int(sizes[b])) for b in range(3)]
    (dp, dn, ea, ep, en), trace = _triplet_trace(net, gs, True, True)
    torch.testing.assert_close(dp.cpu(), dp_ref.detach(), rtol=1e-4, atol=1e-4)
    torch.testing.assert_close(dn.cpu(), dn_ref.detach(), rtol=1e-4, atol=1e-4)
    for got, want in zip((ea, ep, en), embeds):
        torch.testing.assert_close(got.cpu(), want.detach(), rtol=1e-4, atol=1e-4)
    checked = 0
    for k, p in m.named_parameters():
        ref = p_ref[k].grad
        if ref is None or p.grad is None:
            continue
        err = (p.grad.cpu() - ref).abs().max().item()
        assert err <= 5e-3 * ref.abs().max().item() + 1e-6, (k, err, ref.abs().max().item())
        checked += 1
    assert checked >= 12
    names = [t[0] for t in trace]
    pooled_stacks = 1 if num_pooling == 1 else 3                       # the level's embedding stack (+ the next level's assignment stack)
    assert names.count("dense_pg_layer_fwd_f32") == 3 * pooled_stacks and names.count("dense_pg_layer_bwd_f32") == 3 * pooled_stacks
    pooled_rows = {3 * int(nmax * 0.25 ** (i + 1)) for i in range(num_pooling)}
    assert not [t for t in trace if t[0] == "row_ln_bwd_f32" and int(t[1][4]) in pooled_rows]     # (v, ldv, dy, lddy, rows, ...)
    _, trace_off = _triplet_trace(net, gs, False, False)
    assert "dense_pg_layer_fwd_f32" not in [t[0] for t in trace_off]
    print("num_pooling %d: library launches of the triplet step: %d with the per-graph routes, %d with both flags off"
          % (num_pooling, len(trace), len(trace_off)))
    assert len(trace) < len(trace_off)


def test_resident_triplet_replayed_equals_eager_steps():
    """the resident triplet under GraphedStep(FlatTrainer(...)): three replays move the parameters as three eager steps of the same
    route do, and no kernel reported an error"""
    from two_stage_gnn_amd import message_passing as mp, triplet as T3
    from two_stage_gnn_amd.data_parallel import FlatTrainer, GraphedStep
    nmax, fin = 32, 8
    x, adj, sizes = dense_batch(47, 3, nmax, fin, sizes=[32, 11, 17], p_edge=0.2)
    m1 = _encoder(nmax, fin, 3)
    m2 = copy.deepcopy(m1)
    dev = next(m1.parameters()).device
    net1, net2 = T3.tripletnet(m1), T3.tripletnet(m2)
    gs = [_G(adj[b].numpy(), x[b].numpy(), int(sizes[b])) for b in range(3)]
    g, xr, xa, sz = T3.assemble([T3.resident_graph(o, dev, net1._resident) for o in gs], dev)
    assert xa is None
    tgt = torch.full((1,), -1.0, device=dev)
    crit = T3.MarginRankingLoss(margin=10.0)
    nat = _nat()
    tr2 = FlatTrainer(m2, lr=1e-3, clip=2.0)
    nat.trace = []
    try:
        for _ in range(3):
            tr2.step(lambda: crit(*net2._embed(xr, g, sz, xr)[:2], tgt))
        names = [t[0] for t in nat.trace]
    finally:
        nat.trace = None
    assert names.count("dense_pg_layer_fwd_f32") == 9 and names.count("dense_pg_layer_bwd_f32") == 9
    tr1 = FlatTrainer(m1, lr=1e-3, clip=2.0)
    step = GraphedStep(tr1, lambda: crit(*net1._embed(xr, g, sz, xr)[:2], tgt), warmup=3)       # (warm-up steps are rolled back)
    for _ in range(3):
        step.step()
    assert np.isfinite(step.loss_value())
    mp.check_device_errors()
    moved = 0
    start = _encoder(nmax, fin, 3).state_dict()
    for (k, p1), (_, p2) in zip(m1.named_parameters(), m2.named_parameters()):
        torch.testing.assert_close(p1.detach(), p2.detach(), rtol=1e-5, atol=1e-6, msg=lambda s_, k=k: k + ": " + s_)
        moved += int(not torch.equal(p2.detach(), start[k]))
    assert moved >= 12


def test_embed_dataset_rows_equal_the_oracle_eval_forwards():
    """two_stage.embed_dataset with the DiffPool model, five graphs in chunks of two (a short last chunk): every row equals the fp64
    oracle's eval-mode B = 1 forward; the pooled level ran on the per-graph launches; the model's mode is restored"""
    from two_stage_gnn_amd import two_stage as TS
    nmax, fin = 32, 8
    x, adj, sizes = dense_batch(53, 5, nmax, fin, sizes=[32, 1, 9, 20, 27], p_edge=0.2)
    m = _encoder(nmax, fin, 3)
    m.eval()
    p = {k: v.detach().cpu().double() for k, v in m.state_dict().items()}
    want = torch.stack([R.diffpool_encoder(p, x[b:b + 1].double(), adj[b:b + 1].double(), sizes[b:b + 1], 1, assign_x=x[b:b + 1].double(),
                                           final_dim="output_dim")[1][0] for b in range(5)]).float()
    graphs = [_G(adj[b].numpy(), x[b].numpy(), int(sizes[b]), label=b % 2) for b in range(5)]
    nat = _nat()
    nat.trace = []
    try:
        got = TS.embed_dataset(m, graphs, chunk=2)
        names = [t[0] for t in nat.trace]
    finally:
        nat.trace = None
    assert names.count("dense_pg_layer_fwd_f32") == 3 * 3 and "dense_pg_layer_bwd_f32" not in names       # three chunks, three layers
    assert not m.training and m.per_graph_bn is False and got.shape == want.shape and not got.requires_grad
    print("embed_dataset, DiffPool: max |row - fp64 B=1| = %.3g (scale %.3g)" % ((got.cpu() - want).abs().max().item(), want.abs().max().item()))
    torch.testing.assert_close(got.cpu(), want, rtol=1e-4, atol=1e-4)
