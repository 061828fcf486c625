"""eigen_triplet.tripletnet — the drop-in for Code/eigengcn/tripletnet.py on eigen_encoders.WavePoolingGcnEncoder — on the GPU:

  5. the tail kernels alone (csrc/mlp2_triplet.hip) against torch in fp64 on the same inputs: embeddings, distances, dr, all four
     parameter gradients; every subset of unused outputs; a is p; widths that are no multiple of a wave or a tile; a single-Linear
     pred_model takes csrc/triplet.hip's tail and a three-Linear one torch, both against the same reference; and
     tsgnn_row_post_nodes_bwd_f32 alone against autograd in fp64 (masked and unmasked ghost rows, a strided gradient block);
  6. the whole step against every fixture of the reference's own tripletnet (the tolerances of tests/test_gpu_eigen_golden.py);
  7. larger triplets (150 / 420 / 290 nodes at Nmax 500, h128) against the fp64 restatement run three times at B = 1;
  8. the fused step equals three B = 1 forwards of the drop-in model itself + the torch tail, with the fused level-0 node under
     per-graph statistics on and off (tsgnn_row_post_nodes_bwd_f32 against the per-op row layer norm);
  9. concat_batches of three cached graphs = batch_from_dense of the stacked dense tensors = collate of the coarsen() results;
 10. the resident cache: no host-to-device copy in a second step on the same objects; same result with it off;
 11. FlatTrainer steps equal torch.optim.Adam + clip_grad_norm_ on the composed route; a GraphedStep over a resident triplet replays
     bitwise-identically and follows refilled features.

Bounds of 5, 7 and 8 (the arbitration rule of tests/test_gpu_sag_triplet.py::_bound): 1e-5 of a tensor's largest entry on outputs,
1e-4 on gradients, or 10 x what the same computation in fp32 on the CPU itself misses fp64 by; both figures are printed.  One tensor —
pred_model's last bias while only the distances carry gradient, whose exact gradient is zero — has an absolute floor (_db2_floor)."""
import copy
import itertools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import test_eigen_triplet_host as H

pytestmark = pytest.mark.gpu

MARGIN = 1.5


def _bound(ref64, ref32, rel, floor_abs=0.0):
    """allowed |hip - fp64|: `rel` of the tensor's largest entry (+ floor_abs), or 10 x what the fp32 CPU computation itself misses by"""
    e_cpu = float((ref32.double() - ref64).abs().max())
    return max(rel * float(ref64.abs().max()) + floor_abs, 10.0 * e_cpu), e_cpu


EPS32 = 1.1920929e-07


def _db2_floor(g_dp, g_dn):
    """ONE tensor gets an absolute floor, and only while no gradient arrives on the embeddings: the last bias' gradient
    db2 = de_a + de_p + de_n is then exactly zero in exact arithmetic (de_a = t_p + t_n, de_p = -t_p, de_n = -t_n: both distances are
    differences of embeddings, a common shift cancels), so the rule "1e-4 of the tensor's largest entry" allows nothing, while any fp32
    evaluation leaves the rounding of the cancelling terms.  Every entry of t_p / t_n is a component of a unit vector times the
    distance's gradient, so |t| <= |g_dp| + |g_dn|; forming t_p + t_n and adding the two negatives rounds twice: 4 fp32 eps of that."""
    return 4.0 * EPS32 * (abs(float(g_dp)) + abs(float(g_dn)))


def _check(what, got, ref64, ref32, rel, against=None, floor=0.0):
    """got within the bound of (ref64, ref32) of fp64 — or, with `against`, of that tensor (two GPU routes compared with each other)"""
    b, e_cpu = _bound(ref64, ref32, rel, floor)
    err = float((got.detach().double().cpu() - (ref64 if against is None else against.detach().double().cpu())).abs().max())
    print("%-34s |hip - fp64| %.3e   fp32 cpu %.3e   bound %.3e" % (what, err, e_cpu, b))
    assert err <= b, (what, err, b)


def _model(c, fin=7):
    from two_stage_gnn_amd import eigen_encoders as EE
    return EE.WavePoolingGcnEncoder(c["nmax"], fin, c["hidden"], c["emb"], c["label_dim"], c["num_layers"], num_pool_matrix=c["J"],
                                    num_pool_final_matrix=c["Jf"], pool_sizes=c["pool_sizes"], pred_hidden_dims=c["pred_hidden"],
                                    mask=c["mask"], args=H.args_of(c))


def _node_names(t):
    seen, todo, names = set(), [t.grad_fn], set()
    while todo:
        f = todo.pop()
        if f is None or f in seen:
            continue
        seen.add(f)
        names.add(type(f).__name__)
        todo += [n for n, _ in f.next_functions]
    return names


# ------------------------------------------------------------------------------------------------ 5. the tail kernels alone
def _tail_ref(r, w1, b1, w2, b2, dtype, used, go):
    """torch: Linear-ReLU-Linear on three rows + both pairwise distances; the loss touches the outputs in `used` with weights `go`"""
    ts = [t.to(dtype).clone().requires_grad_(True) for t in (r, w1, b1, w2, b2)]
    r_, w1_, b1_, w2_, b2_ = ts
    e = F.linear(torch.relu(F.linear(r_, w1_, b1_)), w2_, b2_)
    outs = (F.pairwise_distance(e[0:1], e[1:2], 2), F.pairwise_distance(e[0:1], e[2:3], 2), e[0:1], e[1:2], e[2:3])
    loss = sum((outs[i] * go[i].to(dtype)).sum() for i in used)
    loss.backward()
    return [o.detach() for o in outs], [t.grad if t.grad is not None else torch.zeros_like(t) for t in ts]


def _tail_inputs(D, Hd, E, seed, same_ap=False):
    g = torch.Generator().manual_seed(seed)
    r = torch.randn(3, D, generator=g)
    if same_ap:
        r[1] = r[0]
    w1, b1 = torch.randn(Hd, D, generator=g) / np.sqrt(D), torch.randn(Hd, generator=g) * 0.1
    w2, b2 = torch.randn(E, Hd, generator=g) / np.sqrt(Hd), torch.randn(E, generator=g) * 0.1
    go = [torch.randn(1, generator=g), torch.randn(1, generator=g)] + [torch.randn(1, E, generator=g) for _ in range(3)]
    return r, w1, b1, w2, b2, go


def _run_tail(r, w1, b1, w2, b2, used, go):
    from two_stage_gnn_amd import eigen_triplet as ET
    ts = [t.cuda().requires_grad_(True) for t in (r, w1, b1, w2, b2)]
    outs = ET._Mlp2TripletTail.apply(*ts)
    sum((outs[i] * go[i].cuda()).sum() for i in used).backward()
    return outs, [t.grad if t.grad is not None else torch.zeros_like(t) for t in ts]


SUBSETS = [s for k in range(1, 6) for s in itertools.combinations(range(5), k)]


@pytest.mark.parametrize("D,Hd,E", [(1156, 50, 6), (2048, 512, 512), (8, 3, 5), (260, 65, 130)])
def test_tail_kernels_vs_torch_fp64(D, Hd, E):
    r, w1, b1, w2, b2, go = _tail_inputs(D, Hd, E, D + Hd)
    for used in ([tuple(range(5))] + (SUBSETS if D <= 1156 else [(0,), (1, 3), (2,), (0, 1)])):
        o64, g64 = _tail_ref(r, w1, b1, w2, b2, torch.float64, used, go)
        o32, g32 = _tail_ref(r, w1, b1, w2, b2, torch.float32, used, go)
        outs, grads = _run_tail(r, w1, b1, w2, b2, used, go)
        tag = "D%d H%d E%d used%s " % (D, Hd, E, "".join(str(i) for i in used))
        for k, name in enumerate(("dist_p", "dist_n", "embed_a", "embed_p", "embed_n")):
            _check(tag + name, outs[k], o64[k], o32[k], 1e-5)
        only_dist = not any(i >= 2 for i in used)
        for k, name in enumerate(("dr", "dw1", "db1", "dw2", "db2")):
            fl = _db2_floor(go[0] if 0 in used else 0.0, go[1] if 1 in used else 0.0) if (name == "db2" and only_dist) else 0.0
            _check(tag + name, grads[k], g64[k], g32[k], 1e-4, floor=fl)


def test_tail_anchor_equals_positive():
    D, Hd, E = 1156, 50, 6
    r, w1, b1, w2, b2, go = _tail_inputs(D, Hd, E, 5, same_ap=True)
    used = (0, 1, 2, 3, 4)
    o64, g64 = _tail_ref(r, w1, b1, w2, b2, torch.float64, used, go)
    o32, g32 = _tail_ref(r, w1, b1, w2, b2, torch.float32, used, go)
    outs, grads = _run_tail(r, w1, b1, w2, b2, used, go)
    assert abs(float(outs[0].detach()) - 1e-6 * np.sqrt(E)) <= 1e-9
    assert all(bool(torch.isfinite(t).all()) for t in list(outs) + grads)
    for k, name in enumerate(("dist_p", "dist_n", "embed_a", "embed_p", "embed_n")):
        _check("a is p " + name, outs[k], o64[k], o32[k], 1e-5)
    for k, name in enumerate(("dr", "dw1", "db1", "dw2", "db2")):
        _check("a is p " + name, grads[k], g64[k], g32[k], 1e-4)


@pytest.mark.parametrize("pred_hidden,node", [([], "_TripletTailBackward"), ([50], "_Mlp2TripletTailBackward"), ([50, 20], None)])
def test_tail_routes(pred_hidden, node):
    """a single Linear takes the existing one-Linear tail, Linear-ReLU-Linear the new kernels, anything longer torch; all three match
    torch's own composition in fp64"""
    from two_stage_gnn_amd import eigen_triplet as ET
    c = dict(J=2, Jf=1, con_final=1, mask=1, nmax=30, num_layers=3, hidden=32, emb=32, label_dim=6, pred_hidden=pred_hidden, pool_sizes=[4])
    torch.manual_seed(3)
    m = _model(c)
    net = ET.tripletnet(m, H.args_of(c))
    D = 96 * 3
    r0 = torch.randn(3, D, generator=torch.Generator().manual_seed(9))
    r = r0.cuda().requires_grad_(True)
    outs = net._tail(r)
    names = _node_names(outs[0])
    if node is None:
        assert not any("TripletTail" in n for n in names), names
    else:
        assert node in names, names
    (outs[0] - outs[1] + outs[2].sum() + 2 * outs[3].sum() - outs[4].sum()).backward()
    res = {}
    for dt in (torch.float64, torch.float32):
        pm = copy.deepcopy(m.pred_model).cpu().to(dt)
        rr = r0.to(dt).requires_grad_(True)
        e = pm(rr)
        o = (F.pairwise_distance(e[0:1], e[1:2], 2), F.pairwise_distance(e[0:1], e[2:3], 2), e[0:1], e[1:2], e[2:3])
        (o[0] - o[1] + o[2].sum() + 2 * o[3].sum() - o[4].sum()).backward()
        res[dt] = ([t.detach() for t in o], rr.grad, [q.grad for q in pm.parameters()])
    for k in range(5):
        _check("route %s out%d" % (pred_hidden, k), outs[k], res[torch.float64][0][k], res[torch.float32][0][k], 1e-5)
    _check("route %s dr" % pred_hidden, r.grad, res[torch.float64][1], res[torch.float32][1], 1e-4)
    for q, g64, g32, (k, _) in zip(m.pred_model.parameters(), res[torch.float64][2], res[torch.float32][2], m.pred_model.named_parameters()):
        _check("route %s %s" % (pred_hidden, k), q.grad, g64, g32, 1e-4)


# ------------------------------------------------------------------------------------------------ the new row-local backward alone
@pytest.mark.parametrize("F_,ln,relu,with_dxs,ghost_zero", [(128, 1, 1, True, 1), (12, 1, 1, True, 1), (200, 1, 1, False, 0),
                                                           (128, 0, 0, True, 0), (64, 1, 1, True, 0)])
def test_row_post_nodes_bwd_against_autograd(F_, ln, relu, with_dxs, ghost_zero):
    """tsgnn_row_post_nodes_bwd_f32 against torch autograd in fp64 through [L2 normalise ; ReLU ; per-row layer norm]: real rows take
    the next layer's gradient + the gradient of their block of the node output (a strided view of a wider buffer), ghost rows only the
    latter, or nothing when the output is masked (tolerances of test_gpu_kernels.py::test_row_post_bwd_against_autograd)"""
    from two_stage_gnn_amd import _native as nat
    gen = torch.Generator().manual_seed(F_ + ln + ghost_zero)
    n_real, n_ghost = 23, 6
    R = n_real + n_ghost
    u = torch.randn(R, F_, generator=gen, dtype=torch.float64, requires_grad=True)
    nrm = u.norm(dim=1, keepdim=True).clamp_min(1e-12)
    v = u / nrm
    y = torch.relu(v) if relu else v
    if ln:
        mu = y.mean(1, keepdim=True)
        y = (y - mu) / torch.sqrt(((y - mu) ** 2).mean(1, keepdim=True) + 1e-5)
    dcat = torch.randn(R, F_ + 8, generator=gen, dtype=torch.float64)         # the gradient of the concatenated node output
    dxs = torch.randn(R, F_, generator=gen, dtype=torch.float64)
    dy = dcat[:, 4:4 + F_].clone()
    if with_dxs:
        dy[:n_real] += dxs[:n_real]
    if ghost_zero:
        dy[n_real:] = 0.0
    (y * dy).sum().backward()
    vg = v.detach().float().cuda()
    yr = torch.relu(vg) if relu else vg
    mean = yr.mean(1).contiguous() if ln else None
    rstd = (1.0 / torch.sqrt(((yr - yr.mean(1, keepdim=True)) ** 2).mean(1) + 1e-5)).contiguous() if ln else None
    rinv = (1.0 / nrm.detach().float().view(-1)).cuda()
    du = torch.full((R, F_), float("nan"), device="cuda")
    dx_g = dxs.float().cuda() if with_dxs else None
    dnode = dcat.float().cuda()[:, 4:4 + F_]
    nat.call("row_post_nodes_bwd_f32", n_real, R, vg, vg.stride(0), dx_g, dx_g.stride(0) if with_dxs else 0, dnode, dnode.stride(0),
             ghost_zero, F_, relu, ln, mean, rstd, rinv, du, du.stride(0))
    torch.testing.assert_close(du.cpu().double(), u.grad, rtol=2e-4, atol=2e-5)


# ------------------------------------------------------------------------------------------------ 6. the reference's own fixtures
@pytest.mark.parametrize("name", H.NAMES)
def test_drop_in_matches_the_reference_tripletnet(name):
    from two_stage_gnn_amd import eigen_triplet as ET
    g = H.load(name)
    c = H.cfg(g)
    m = _model(c)
    m.load_state_dict({k[2:]: torch.tensor(v) for k, v in g.items() if k.startswith("p.")}, strict=True)
    dicts, _ = H.graph_dicts(g)
    objs = [H.GraphObj(d) for d in dicts]
    if c["same_ap"]:
        objs[1] = objs[0]
    net = ET.tripletnet(m, H.args_of(c))
    dp, dn, ea, e_p, en = net(*objs)
    loss = ET.MarginRankingLoss(margin=c["margin"])(dp, dn, torch.full_like(dp, -1.0))
    loss.backward()
    np.testing.assert_allclose(dp.detach().cpu().numpy(), g["dist_p"], rtol=1e-4, atol=1e-4)
    np.testing.assert_allclose(dn.detach().cpu().numpy(), g["dist_n"], rtol=1e-4, atol=1e-4)
    np.testing.assert_allclose(torch.cat([ea, e_p, en]).detach().cpu().numpy(), g["embed"], rtol=1e-4, atol=1e-4)
    assert abs(float(loss.detach()) - float(g["loss"])) < 1e-4
    for k, p in m.named_parameters():
        ref = g["g." + k]
        got = p.grad.cpu().numpy() if p.grad is not None else np.zeros_like(ref)
        np.testing.assert_allclose(got, ref, rtol=2e-3, atol=2e-4, err_msg=k)


# ------------------------------------------------------------------------------------------------ larger triplets, built here
BIG = {
    # name: (sizes, nmax, features, config)
    "dd": ([150, 420, 290], 500, 89, dict(J=2, Jf=1, con_final=1, mask=1, pool_sizes=[10])),
    "dd_nomask": ([150, 420, 290], 500, 89, dict(J=2, Jf=1, con_final=1, mask=0, pool_sizes=[10])),
    "dd_two_levels": ([150, 420, 290], 500, 89, dict(J=2, Jf=1, con_final=1, mask=1, pool_sizes=[10, 4])),
    "mid": ([40, 90, 63], 96, 12, dict(J=2, Jf=1, con_final=1, mask=1, pool_sizes=[6])),
}


def _chunks(A, k, level):
    return np.arange(A.shape[0]) * k // A.shape[0]


def _rand_adj(rng, n, extra=1.5):
    A = np.zeros((n, n))
    i = np.arange(n)
    A[i, (i + 1) % n] = 1
    a, b = rng.integers(0, n, int(extra * n)), rng.integers(0, n, int(extra * n))
    A[a[a != b], b[a != b]] = 1
    return np.maximum(A, A.T)


def big_triplet(name, hidden=128, label_dim=6, pred_hidden=(50,)):
    """(config, three ``.graph`` dicts, the coarsen() results): chunk-clustered random graphs through eigen_pool.coarsen and
    eigen_pool.dense_inputs at B = 1 per graph"""
    from two_stage_gnn_amd import eigen_pool as ep
    sizes, nmax, fin, base = BIG[name]
    c = dict(base, nmax=nmax, num_layers=3, hidden=hidden, emb=hidden, label_dim=label_dim, pred_hidden=list(pred_hidden), same_ap=0,
             margin=MARGIN)
    rng = np.random.default_rng(len(name) + 7)
    L = len(c["pool_sizes"])
    dicts, results = [], []
    for n in sizes:
        r = ep.coarsen(_rand_adj(rng, n), c["pool_sizes"], labels=_chunks)
        assert r is not None
        adj, pooled, n0, nl, pm = ep.dense_inputs([r], nmax, c["J"], c["Jf"])
        feats = np.zeros((nmax, fin), dtype=np.float32)
        feats[:n] = rng.standard_normal((n, fin)).astype(np.float32)
        d = {"adj": adj[0].numpy(), "feats": feats, "num_nodes": n}
        for i in range(L):
            d["adj_pool_%d" % (i + 1)] = pooled[i][0].numpy()
            d["num_nodes_%d" % (i + 1)] = int(nl[i][0])
            for j in range(c["J"]):
                d["pool_adj_%d_%d" % (i, j)] = pm[i][j][0].numpy()
        for j in range(c["Jf"]):
            d["pool_adj_%d_%d" % (L, j)] = pm[L][j][0].numpy()
        dicts.append(d)
        results.append(r)
    return c, fin, dicts, results


def seeded_state(m, seed):
    """every parameter drawn from a CPU generator: the same numbers on any machine"""
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for k, v in m.state_dict().items():
        sd[k] = torch.randn(v.shape, generator=g) * (1.0 / np.sqrt(max(v.shape)) if v.dim() > 1 else 0.1)
    return sd


def _big_model(c, fin, seed=11):
    m = _model(c, fin)
    m.load_state_dict(seeded_state(m, seed))
    return m


def _cpu_params(m, dtype):
    return {k: v.detach().cpu().to(dtype).clone().requires_grad_(True) for k, v in m.state_dict().items()}


# ------------------------------------------------------------------------------------------------ 7. against the fp64 restatement
@pytest.mark.parametrize("name", ["dd", "dd_nomask", "dd_two_levels"])
def test_step_vs_three_single_graph_restatements(name):
    from two_stage_gnn_amd import eigen_triplet as ET
    c, fin, dicts, _ = big_triplet(name)
    m = _big_model(c, fin)
    p64, p32 = _cpu_params(m, torch.float64), _cpu_params(m, torch.float32)
    r64 = H.ref_step(p64, dicts, c, torch.float64)
    r32 = H.ref_step(p32, dicts, c, torch.float32)
    assert float(r64[3]) > 0.0, "the hinge of this triplet is not active: the gradients would all be zero"
    net = ET.tripletnet(m, H.args_of(c))
    outs = net(*[H.GraphObj(d) for d in dicts])
    loss = ET.MarginRankingLoss(margin=MARGIN)(outs[0], outs[1], torch.full_like(outs[0], -1.0))
    loss.backward()
    assert "_SageStackBackward" in _node_names(outs[0])
    _check(name + " dist_p", outs[0], r64[0], r32[0], 1e-5)
    _check(name + " dist_n", outs[1], r64[1], r32[1], 1e-5)
    for b in range(3):
        _check(name + " embed %d" % b, outs[2 + b], r64[2][b], r32[2][b], 1e-5)
    _check(name + " loss", loss, r64[3], r32[3], 1e-5)
    last_bias = [k for k in p64 if k.startswith("pred_model") and k.endswith("bias")][-1]
    for k, q in m.named_parameters():
        assert q.grad is not None, k
        # (the loss touches the distances only, each with gradient +-1: the last bias' exact gradient is zero)
        _check(name + " " + k, q.grad, p64[k].grad, p32[k].grad, 1e-4, floor=_db2_floor(1.0, 1.0) if k == last_bias else 0.0)


# ------------------------------------------------------------------------------------------------ 8. fused step = composed B = 1 forwards
def _composed(m, dicts, c):
    """three B = 1 forwards of the drop-in model itself from the dense tensors + the torch tail"""
    es = []
    for d in dicts:
        x, adj, pooled, n0, nl, pm = H.dense_inputs(d, c, torch.float32)
        f = lambda t: t.cuda()
        es.append(m(f(x), f(adj), [f(a) for a in pooled], n0, nl, {i: [f(t) for t in v] for i, v in pm.items()}))
    return F.pairwise_distance(es[0], es[1], 2), F.pairwise_distance(es[0], es[2], 2), es[0], es[1], es[2]


@pytest.mark.parametrize("stack", [True, False])
@pytest.mark.parametrize("name", ["mid", "dd"])
def test_fused_step_equals_three_single_graph_forwards(name, stack, monkeypatch):
    from two_stage_gnn_amd import dense_encoders as DE, eigen_triplet as ET
    monkeypatch.setattr(DE, "PER_GRAPH_STACK", stack)
    c, fin, dicts, _ = big_triplet(name, hidden=128 if name == "dd" else 32)
    m1 = _big_model(c, fin)
    m2 = copy.deepcopy(m1)
    p64, p32 = _cpu_params(m1, torch.float64), _cpu_params(m1, torch.float32)
    r64 = H.ref_step(p64, dicts, c, torch.float64)
    r32 = H.ref_step(p32, dicts, c, torch.float32)
    net = ET.tripletnet(m1, H.args_of(c))
    o1 = net(*[H.GraphObj(d) for d in dicts])
    names = _node_names(o1[0])
    assert ("_SageStackBackward" in names) == stack, names        # on: level 0 ran as the fused node; off: the per-op row layer norm
    assert "_Mlp2TripletTailBackward" in names
    ET.MarginRankingLoss(margin=MARGIN)(o1[0], o1[1], torch.full_like(o1[0], -1.0)).backward()
    o2 = _composed(m2, dicts, c)
    torch.nn.MarginRankingLoss(margin=MARGIN)(o2[0], o2[1], torch.full_like(o2[0], -1.0)).backward()
    tag = "%s stack=%d " % (name, stack)
    refs = [r64[0], r64[1]] + r64[2], [r32[0], r32[1]] + r32[2]
    for k in range(5):
        _check(tag + "out%d" % k, o1[k], refs[0][k], refs[1][k], 1e-5, against=o2[k])
    last_bias = [k for k in p64 if k.startswith("pred_model") and k.endswith("bias")][-1]
    for (k, q1), q2 in zip(m1.named_parameters(), m2.parameters()):
        assert q1.grad is not None and q2.grad is not None, k
        _check(tag + k, q1.grad, p64[k].grad, p32[k].grad, 1e-4, against=q2.grad, floor=_db2_floor(1.0, 1.0) if k == last_bias else 0.0)


# ------------------------------------------------------------------------------------------------ 9. the three routes to one batch
def _same_graph(a, b, what):
    assert (a.B, a.nmax, a.n_rows, a.n_ghost, a.nnz) == (b.B, b.nmax, b.n_rows, b.n_ghost, b.nnz), what
    assert torch.equal(a.rowptr, b.rowptr), what
    assert torch.equal(a.col[:a.nnz], b.col[:b.nnz]), what
    va = a.val[:a.nnz] if a.val is not None else torch.ones(a.nnz, device=a.col.device)
    vb = b.val[:b.nnz] if b.val is not None else torch.ones(b.nnz, device=b.col.device)
    assert torch.equal(va, vb), what
    assert torch.equal(a.graph_ptr, b.graph_ptr) and np.array_equal(np.asarray(a.sizes), np.asarray(b.sizes)), what


def _same_batch(a, b, what):
    _same_graph(a.g0, b.g0, what + " g0")
    assert len(a.levels) == len(b.levels)
    g = a.g0
    for i, (la, lb) in enumerate(zip(a.levels, b.levels)):
        R = g.n_rows
        w = "%s level %d" % (what, i)
        assert torch.equal(la.cluster_of[:R], lb.cluster_of[:R]), w
        assert torch.equal(la.coef[:R], lb.coef[:R]), w
        assert torch.equal(la.bptr.long(), lb.bptr.long()), w
        assert torch.equal(la.members[:R].long(), lb.members[:R].long()), w
        _same_graph(la.g, lb.g, w)
        g = la.g
    if a.final_coef is None:
        assert b.final_coef is None
    else:
        assert torch.equal(a.final_coef[:g.n_rows], b.final_coef[:g.n_rows]), what + " final"


@pytest.mark.parametrize("name", ["mid", "dd_two_levels"])
def test_concat_batches_equals_the_dense_conversion_and_collate(name):
    from two_stage_gnn_amd import eigen_pool as ep, eigen_triplet as ET
    c, fin, dicts, results = big_triplet(name, hidden=32)
    L, J, Jf = len(c["pool_sizes"]), c["J"], c["Jf"]
    m = _big_model(c, fin)
    net = ET.tripletnet(m, H.args_of(c))
    b = net.batch(*[H.GraphObj(d) for d in dicts])
    st = lambda key: torch.as_tensor(np.stack([np.asarray(d[key], dtype=np.float32) for d in dicts])).cuda()
    pm = {i: [st("pool_adj_%d_%d" % (i, j)) for j in range(J if i < L else Jf)] for i in range(L + (1 if Jf else 0))}
    sizes = [int(d["num_nodes"]) for d in dicts]
    sizes_l = [[int(d["num_nodes_%d" % (i + 1)]) for d in dicts] for i in range(L)]
    eb_dense = ep.batch_from_dense(st("adj"), sizes, [st("adj_pool_%d" % (i + 1)) for i in range(L)], sizes_l, pm, J, Jf, L)
    eb_coll = ep.collate(results, c["nmax"], J, Jf, device=torch.device("cuda", torch.cuda.current_device()))
    _same_batch(b.eb, eb_dense, "concat vs batch_from_dense")
    _same_batch(b.eb, eb_coll, "concat vs collate")
    m.per_graph_bn = True
    with torch.no_grad():
        outs = [m(b.x, eb) for eb in (b.eb, eb_dense, eb_coll)]
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])


# ------------------------------------------------------------------------------------------------ 10. the resident cache
def test_second_step_on_the_same_objects_uploads_nothing(monkeypatch):
    from two_stage_gnn_amd import eigen_triplet as ET, triplet as T3
    c, fin, dicts, _ = big_triplet("mid", hidden=32)
    m = _big_model(c, fin).eval()
    objs = [H.GraphObj(d) for d in dicts]
    net = ET.tripletnet(m, H.args_of(c))
    with torch.no_grad():
        first = net(*objs)
        cc = net.cache
        per_graph = cc.h2d // 3
        assert (cc.hits, cc.misses, len(cc)) == (0, 3, 3) and cc.h2d == 3 * per_graph and per_graph > 0
        second = net(*objs)
        assert (cc.hits, cc.misses, cc.h2d, len(cc)) == (3, 3, 3 * per_graph, 3)
        again = net(objs[0], objs[0], objs[2])               # anchor and positive the same object
        assert cc.h2d == 3 * per_graph and abs(float(again[0]) - 1e-6 * np.sqrt(c["label_dim"])) <= 1e-5
        monkeypatch.setattr(T3, "RESIDENT", False)           # TSGNN_TRIPLET_CACHE=0
        off = ET.tripletnet(m, H.args_of(c))
        third = off(*objs)
        assert len(off.cache) == 0 and off.cache.h2d == 3 * per_graph
        off(*objs)
        assert off.cache.h2d == 6 * per_graph
    for a, b, d in zip(first, second, third):
        assert torch.equal(a, b) and torch.equal(a, d)


# ------------------------------------------------------------------------------------------------ 11. trainer integration
def _reg_loss(crit, outs, tgt):
    """the margin loss + norm regularisers on the three embeddings (as the dense family's loop adds them): gradients reach the tail on
    the distances AND on the embeddings, and the last bias has a gradient that is not pure rounding (the distances alone do not
    depend on it, and Adam normalises whatever noise it is given to a full-size update)"""
    dp, dn, ea, e_p, en = outs
    return crit(dp, dn, tgt) + 1e-2 * (ea.norm(2) + e_p.norm(2) + en.norm(2))


LR = 1e-4          # (a first Adam step at 1e-3 moves every coordinate against a gradient of l1 norm ~2e3: the hinge is satisfied at once)

def test_flat_trainer_steps_equal_torch_adam_on_the_composed_route():
    """three optimiser steps: the fused triplet under FlatTrainer (gradients straight into the flat bucket, clip 2.0 + Adam in the
    library's kernels, one hipGraph) against autograd + clip_grad_norm_ + torch.optim.Adam on three B = 1 forwards and the torch tail"""
    from two_stage_gnn_amd import eigen_triplet as ET
    from two_stage_gnn_amd.data_parallel import FlatTrainer, GraphedStep
    c, fin, dicts, _ = big_triplet("mid", hidden=32)
    m1 = _big_model(c, fin).train()
    m2 = copy.deepcopy(m1)
    tgt = torch.full((1,), -1.0, device="cuda")
    crit2 = torch.nn.MarginRankingLoss(margin=MARGIN)
    params2 = list(m2.parameters())
    opt = torch.optim.Adam(params2, lr=LR)
    for _ in range(3):
        opt.zero_grad(set_to_none=True)
        _reg_loss(crit2, _composed(m2, dicts, c), tgt).backward()
        torch.nn.utils.clip_grad_norm_([q for q in params2 if q.grad is not None], 2.0)
        opt.step()
    net1, crit1 = ET.tripletnet(m1, H.args_of(c)), ET.MarginRankingLoss(margin=MARGIN)
    b1 = net1.batch(*[H.GraphObj(d) for d in dicts])
    tr = FlatTrainer(m1, lr=LR, clip=2.0)
    gs = GraphedStep(tr, lambda: _reg_loss(crit1, net1.embed(b1), tgt), warmup=3)          # (warm-up steps are rolled back)
    assert gs.describe().startswith("one graph"), gs.describe()
    for _ in range(3):
        gs.step()
    assert gs.loss_value() > 0.5                       # (the hinge is still active: the regularisers alone are ~1e-2)
    for (k, q1), (_, q2) in zip(m1.named_parameters(), m2.named_parameters()):
        assert q2.grad is not None, k
        torch.testing.assert_close(q1.detach(), q2.detach(), rtol=2e-4, atol=2e-6, msg=lambda s_, k=k: k + ": " + s_)


def test_resident_triplet_replays_bitwise_and_follows_refilled_features():
    """two GraphedSteps on twin models replay bitwise-identically; with the features refilled between replays the losses and
    parameters equal those of an eager twin fed the same sequence"""
    from two_stage_gnn_amd import eigen_triplet as ET
    from two_stage_gnn_amd.data_parallel import FlatTrainer, GraphedStep
    c, fin, dicts, _ = big_triplet("mid", hidden=32)
    objs = [H.GraphObj(d) for d in dicts]
    tgt = torch.full((1,), -1.0, device="cuda")
    base = _big_model(c, fin).train()
    nets = [ET.tripletnet(copy.deepcopy(base), H.args_of(c)) for _ in range(3)]
    crit = ET.MarginRankingLoss(margin=MARGIN)
    bs = [t.batch(*objs) for t in nets]
    trainers = [FlatTrainer(t.model, lr=LR, clip=2.0) for t in nets]
    fns = [lambda t=t, b=b: _reg_loss(crit, t.embed(b), tgt) for t, b in zip(nets, bs)]
    g0, g1 = GraphedStep(trainers[0], fns[0], warmup=3), GraphedStep(trainers[1], fns[1], warmup=3)
    assert g0.describe().startswith("one graph"), g0.describe()
    n_real = int(bs[0].eb.g0.n_rows)
    ld = bs[0].x.size(1)
    for i in range(4):
        xi = torch.randn(n_real, ld, generator=torch.Generator().manual_seed(300 + i)).cuda() * (1.0 + 0.25 * i)
        xi[:, fin:] = 0.0
        for b in bs:
            b.x[:n_real].copy_(xi)
        g0.step()
        g1.step()
        l_graph = g0.loss_value()
        assert l_graph == g1.loss_value()
        for a, b in zip(nets[0].model.parameters(), nets[1].model.parameters()):
            assert torch.equal(a.detach(), b.detach())                       # two replays of the same step: bitwise
        l_eager = float(trainers[2].step(fns[2]).detach())
        assert abs(l_graph - l_eager) <= 1e-5 * max(1.0, abs(l_eager)), (i, l_graph, l_eager)
        for (k, a), b in zip(nets[0].model.named_parameters(), nets[2].model.parameters()):
            scale = float(b.detach().abs().max()) + 1e-30
            assert float((a.detach() - b.detach()).abs().max()) <= 1e-5 * scale, (i, k)
