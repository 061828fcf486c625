"""sag_triplet.tripletnet — the drop-in for Code/sag/tripletnet.py on sag_layers.Net — on the GPU:

  1. the tail kernels alone (csrc/mlp_head.hip, tsgnn_mlp3_triplet_fwd_f32 / _bwd_f32) against torch in fp64 on the same inputs and the
     regenerated dropout mask: embeddings, distances, dx, all six parameter gradients; every subset of unused embedding outputs; a is p;
  2. the whole step against oracle/pyg_ref run three times at B = 1 (fp64; fp32 on the CPU as the yardstick of what fp32 can give):
     distances, embeddings, every parameter gradient after MarginRankingLoss(margin=1.5); both conv kinds, use_batch both ways,
     eval and training mode (the oracle's head then applies the regenerated mask);
  3. top-k ties: a triplet whose pooling cut the fp64 oracle itself finds ambiguous is skipped LOUDLY (the seeds below give none);
  4. the fused step equals the hand composition (three fused Net(use_batch=True) B = 1 forwards + torch tail), and the composed route;
  5. FlatTrainer steps equal torch.optim.Adam on the composed route; a GraphedStep over a resident triplet follows refilled features;
  6. the resident cache: no host-to-device copy of graph structure in a second step on the same objects; same result with it off.
PARITY UNPINNED (no torch_geometric in the reference tree): the oracle restates PyG's documented formulas.

Tolerances are the ones tests/test_gpu_sagepoolnet_fused.py uses for the same node against the same oracle: rtol = atol = 1e-5 on outputs,
1e-4 of a tensor's largest entry on gradients; where fp32 itself cannot give that (the CPU oracle in fp32 against fp64), 10 x the fp32
oracle's own error (the arbitration rule of tests/test_gpu_fullsize.py) — both figures are printed."""
import copy

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import pyg_ref as P
from test_gpu_pyg import rand_graph, tie_free

pytestmark = pytest.mark.gpu

RATIO = 0.5


class _D:
    """stands for torch_geometric.data.Data"""

    def __init__(self, x, ei, dev="cuda"):
        self.x, self.edge_index = x.to(dev), ei.to(dev)
        self.y = torch.tensor([0])                         # (ignored, as network.py:32 ignores everything but x and edge_index)


def _graph(seed, n, fin, e_per_node=2.2, sym=True):
    ei = rand_graph(seed, n, int(e_per_node * n), sym) if (n > 1 and e_per_node > 0) else torch.zeros(2, 0, dtype=torch.long)
    return tie_free(seed + 1000, n, fin), ei


NET_SEED = 21
CASES = {
    # name: (fin, nhid, C, [(n, edges per node)] for anchor / positive / negative, graph seed).  The graph seeds were searched on the
    # CPU so that, with the parameters of NET_SEED and either conv kind, the fp64 oracle's scores on both sides of every pooling cut
    # differ by more than 5e-4 of the graph's largest |score| (sparse random graphs pool into two-node components, whose GCN
    # scores tie exactly): test_case_list_has_no_ambiguous_triplet
    "n1_noedges": (5, 32, 8, [(1, 0), (7, 0), (13, 2.2)], 0),        # a single node; a graph without edges
    "odd": (5, 32, 8, [(9, 2.0), (31, 2.5), (17, 1.5)], 6),          # odd n: k = ceil(ratio n)
    "spread": (3, 64, 64, [(3, 1.0), (64, 3.0), (250, 2.0)], 48),    # three very different sizes
    "dd": (89, 128, 64, [(150, 2.5), (420, 2.5), (290, 2.5)], 74),   # DD-shaped (89 features, a few hundred nodes), nhid 128
}


def _triplet(name):
    fin, nhid, C, spec, seed = CASES[name]
    return fin, nhid, C, [_graph(100 * (i + 1) + seed + len(name), n, fin, e) for i, (n, e) in enumerate(spec)]


def _net(fin, nhid, C, conv, use_batch, p_drop, seed, dev="cuda"):
    """sag_layers.Net with every parameter drawn from a CPU generator (the same numbers on any machine: the seeds below were checked
    for top-k ambiguity against the fp64 oracle on the CPU)"""
    from two_stage_gnn_amd import sag_layers as S
    net = S.Net(fin, nhid, C, RATIO, p_drop, use_batch=use_batch, conv=conv)
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for k, v in net.state_dict().items():
        sd[k] = torch.randn(v.shape, generator=g) * (1.0 / np.sqrt(max(v.shape)) if v.dim() > 1 else 0.1)
    net.load_state_dict(sd)
    return net.to(dev)


def _params(net, dtype):
    return {k: v.detach().cpu().to(dtype).clone().requires_grad_(True) for k, v in net.state_dict().items()}


def _oracle_embed(p, x, ei, conv, keep=None, scale=1.0):
    """one graph alone -> log-probabilities [1, C].  Eval: pyg_ref.sag_net as it is.  Training: sag_net is eval-only, so its levels are
    composed here from the same pyg_ref functions and the head applies the mask (keep [1, D1] of 0 / 1, survivors * scale)"""
    if keep is None:
        return P.sag_net(p, x, ei, RATIO, batch=None, conv=conv)
    outs, batch = [], None
    for i in (1, 2, 3):
        if conv == "sage":
            x = F.relu(P.sage_conv(x, ei, p["conv%d.lin_l.weight" % i], p["conv%d.lin_l.bias" % i], p["conv%d.lin_r.weight" % i]))
        else:
            x = F.relu(P.gcn_conv(x, ei, p["conv%d.weight" % i], p["conv%d.bias" % i]))
        x, ei, batch, _ = P.sag_pool(x, ei, batch, RATIO, p["pool%d.score_layer.weight" % i], p["pool%d.score_layer.bias" % i])
        outs.append(torch.cat([P.global_max_pool(x, batch, 1), P.global_mean_pool(x, batch, 1)], dim=1))
    h = outs[0] + outs[1] + outs[2]
    h = F.relu(F.linear(h, p["lin1.weight"], p["lin1.bias"])) * keep.to(h.dtype) * scale
    h = F.relu(F.linear(h, p["lin2.weight"], p["lin2.bias"]))
    return F.log_softmax(F.linear(h, p["lin3.weight"], p["lin3.bias"]), dim=-1)


def _oracle_step(p, graphs, conv, keep=None, scale=1.0):
    """three B = 1 forwards, both distances, the margin loss and its backward (Code/sag/train_triplet.py:207-212)"""
    dt = next(iter(p.values())).dtype
    e = [_oracle_embed(p, x.to(dt), ei, conv, None if keep is None else keep[b:b + 1], scale) for b, (x, ei) in enumerate(graphs)]
    dp, dn = F.pairwise_distance(e[0], e[1], 2), F.pairwise_distance(e[0], e[2], 2)
    loss = torch.nn.MarginRankingLoss(margin=1.5)(dp, dn, torch.full_like(dp, -1.0))
    loss.backward()
    return dp.detach(), dn.detach(), [t.detach() for t in e], float(loss.detach())


def _ambiguous(p64, x, ei, conv, tol=1e-4):
    """fp64 oracle, level by level: is the pooling cut of this graph undefined — the last kept and the first dropped score within `tol`
    of the graph's largest |score| (the rule of test_gpu_sagepoolnet_fused._ambiguous_graphs_gc, one graph, the GCNConv scorer)"""
    x, batch = x.double(), None
    with torch.no_grad():
        for i in (1, 2, 3):
            if conv == "sage":
                x = F.relu(P.sage_conv(x, ei, p64["conv%d.lin_l.weight" % i], p64["conv%d.lin_l.bias" % i], p64["conv%d.lin_r.weight" % i]))
            else:
                x = F.relu(P.gcn_conv(x, ei, p64["conv%d.weight" % i], p64["conv%d.bias" % i]))
            w, b = p64["pool%d.score_layer.weight" % i], p64["pool%d.score_layer.bias" % i]
            s = P.gcn_conv(x, ei, w, b).view(-1)
            n = s.numel()
            k = int(np.ceil(np.float32(RATIO) * np.float32(n)))
            if k < n:
                o = torch.sort(s, descending=True).values
                if float(o[k - 1] - o[k]) <= tol * (float(s.abs().max()) + 1e-30):
                    return True
            x, ei, batch, _ = P.sag_pool(x, ei, batch, RATIO, w, b)
    return False


def _bound(ref64, ref32, rel, floor_abs=0.0):
    """allowed |hip - fp64|: `rel` of the tensor's largest entry (+ floor_abs), or 10 x what the fp32 CPU oracle itself misses by"""
    e_cpu = float((ref32.double() - ref64).abs().max())
    return max(rel * float(ref64.abs().max()) + floor_abs, 10.0 * e_cpu), e_cpu


# ------------------------------------------------------------------------------------------------ 1. the tail kernels alone
def _tail_ref(r, w, keep, scale, dtype, used):
    """torch: head on three rows + log_softmax + both pairwise distances; loss touches the distances and the embeddings in `used`"""
    r = r.to(dtype).clone().requires_grad_(True)
    w = [t.to(dtype).clone().requires_grad_(True) for t in w]
    h = F.relu(F.linear(r, w[0], w[1]))
    if keep is not None:
        h = h * keep.to(dtype) * scale
    h = F.relu(F.linear(h, w[2], w[3]))
    e = F.log_softmax(F.linear(h, w[4], w[5]), dim=-1)
    dp, dn = F.pairwise_distance(e[0:1], e[1:2], 2), F.pairwise_distance(e[0:1], e[2:3], 2)
    loss = _tail_loss(dp, dn, [e[0:1], e[1:2], e[2:3]], used)
    g = torch.autograd.grad(loss, [r] + w)
    return e.detach(), torch.cat([dp, dn]).detach(), g


def _tail_loss(dp, dn, es, used):
    loss = torch.nn.MarginRankingLoss(margin=1.5)(dp, dn, torch.full_like(dp, -1.0)) + 0.3 * dn.sum()
    coef = (0.05, -0.07, 0.11)
    for i in used:
        loss = loss + coef[i] * es[i].norm(2) + 0.01 * es[i].sum()
    return loss


SUBSETS = [(), (0,), (1,), (2,), (0, 1), (0, 2), (1, 2), (0, 1, 2)]


@pytest.mark.parametrize("p_drop", [0.0, 0.5])
@pytest.mark.parametrize("nhid,C", [(128, 64), (128, 2), (64, 64), (64, 2)])
def test_tail_kernels_vs_torch_fp64(nhid, C, p_drop):
    from two_stage_gnn_amd import message_passing as mp, sag_triplet as ST
    dev = torch.device("cuda")
    D0, D1, D2 = 2 * nhid, nhid, nhid // 2
    assert ST.nat.lib().tsgnn_mlp3_triplet_supported(D0, D1, D2, C) == 1
    gen = torch.Generator().manual_seed(nhid + C)
    r = torch.randn(3, D0, generator=gen)
    w = [torch.randn(D1, D0, generator=gen) / np.sqrt(D0), torch.randn(D1, generator=gen) * 0.1,
         torch.randn(D2, D1, generator=gen) / np.sqrt(D1), torch.randn(D2, generator=gen) * 0.1,
         torch.randn(C, D2, generator=gen) / np.sqrt(D2), torch.randn(C, generator=gen) * 0.1]
    torch.manual_seed(17)
    for used in SUBSETS:
        rg = r.to(dev).requires_grad_(True)
        wg = [t.to(dev).requires_grad_(True) for t in w]
        drop = ST._in_kernel_dropout(p_drop, rg.device) if p_drop > 0 else None
        dp, dn, ea, ep, en = ST._SagTripletTail.apply(rg, *wg, drop)
        assert dp.shape == dn.shape == (1,) and ea.shape == ep.shape == en.shape == (1, C)
        g = torch.autograd.grad(_tail_loss(dp, dn, [ea, ep, en], used), [rg] + wg)
        keep, scale = None, 1.0
        if drop is not None:
            keep, scale = mp.mlp3_dropout_mask(drop[0], drop[1], drop[3], 3, D1).cpu(), 1.0 / (1.0 - p_drop)
            assert 0.25 < float(keep.mean()) < 0.75
        e64, d64, g64 = _tail_ref(r, w, keep, scale, torch.float64, used)
        e32, d32, g32 = _tail_ref(r, w, keep, scale, torch.float32, used)
        torch.testing.assert_close(torch.cat([ea, ep, en]).detach().cpu().double(), e64, rtol=1e-5, atol=1e-5)
        torch.testing.assert_close(torch.cat([dp, dn]).detach().cpu().double(), d64, rtol=1e-5, atol=1e-5)
        for name, a, c64, c32 in zip(["dx", "dw1", "db1", "dw2", "db2", "dw3", "db3"], g, g64, g32):
            bound, e_cpu = _bound(c64, c32, 1e-4)
            err = float((a.cpu().double() - c64).abs().max())
            assert err <= bound, (used, name, err, e_cpu, float(c64.abs().max()))
    if p_drop > 0:                                         # a second launch draws another mask (the device counter moved on)
        k1 = mp.mlp3_dropout_mask(drop[0], drop[1], drop[3], 3, D1)
        d2 = ST._in_kernel_dropout(p_drop, rg.device)
        ST._SagTripletTail.apply(rg, *wg, d2)
        assert not torch.equal(k1, mp.mlp3_dropout_mask(d2[0], d2[1], d2[3], 3, D1))


def test_tail_anchor_equals_positive_gives_torchs_finite_values():
    """a is p: dist_p = ||eps||, and its gradient is torch's finite one, not NaN"""
    from two_stage_gnn_amd import sag_triplet as ST
    dev = torch.device("cuda")
    D0, D1, D2, C = 128, 64, 32, 64
    gen = torch.Generator().manual_seed(4)
    r = torch.randn(3, D0, generator=gen)
    r[1] = r[0]
    w = [torch.randn(D1, D0, generator=gen) / np.sqrt(D0), torch.randn(D1, generator=gen) * 0.1,
         torch.randn(D2, D1, generator=gen) / np.sqrt(D1), torch.randn(D2, generator=gen) * 0.1,
         torch.randn(C, D2, generator=gen) / np.sqrt(D2), torch.randn(C, generator=gen) * 0.1]
    rg = r.to(dev).requires_grad_(True)
    wg = [t.to(dev).requires_grad_(True) for t in w]
    dp, dn, ea, ep, en = ST._SagTripletTail.apply(rg, *wg, None)
    assert torch.equal(ea, ep)
    g = torch.autograd.grad(_tail_loss(dp, dn, [ea, ep, en], (0,)), [rg] + wg)
    e64, d64, g64 = _tail_ref(r, w, None, 1.0, torch.float64, (0,))
    e32, d32, g32 = _tail_ref(r, w, None, 1.0, torch.float32, (0,))
    assert abs(float(dp) - 1e-6 * np.sqrt(C)) <= 1e-11 and abs(float(d64[0]) - 1e-6 * np.sqrt(C)) <= 1e-11
    torch.testing.assert_close(torch.cat([dp, dn]).detach().cpu().double(), d64, rtol=1e-5, atol=1e-5)
    for name, a, c64, c32 in zip(["dx", "dw1", "db1", "dw2", "db2", "dw3", "db3"], g, g64, g32):
        assert bool(torch.isfinite(a).all()), name
        bound, e_cpu = _bound(c64, c32, 1e-4)
        err = float((a.cpu().double() - c64).abs().max())
        assert err <= bound, (name, err, e_cpu)


class _Head(torch.nn.Module):
    def __init__(self, nhid, C, p):
        super().__init__()
        self.lin1, self.lin2, self.lin3 = torch.nn.Linear(2 * nhid, nhid), torch.nn.Linear(nhid, nhid // 2), torch.nn.Linear(nhid // 2, C)
        self.dropout_ratio = p


def test_tail_shape_outside_supported_takes_the_torch_tail():
    from two_stage_gnn_amd import _native as nat, sag_triplet as ST
    nhid, C = 66, 4                                        # lin1: 132 -> 66 (66 % 4 != 0: no 16-byte rows for lin2)
    assert nat.lib().tsgnn_mlp3_triplet_supported(2 * nhid, nhid, nhid // 2, C) == 0
    torch.manual_seed(2)
    head = _Head(nhid, C, 0.0).cuda().eval()
    net = ST.tripletnet(head)
    r = torch.randn(3, 2 * nhid).cuda().requires_grad_(True)
    assert not ST.tail_ok(head, r)
    names = []
    prev, nat.trace = nat.trace, names
    try:
        dp, dn, ea, ep, en = net._tail(r)
    finally:
        nat.trace = prev
    assert "mlp3_triplet_fwd_f32" not in [t[0] for t in names]
    w = [t.detach().cpu() for t in (head.lin1.weight, head.lin1.bias, head.lin2.weight, head.lin2.bias, head.lin3.weight, head.lin3.bias)]
    e64, d64, _ = _tail_ref(r.detach().cpu(), w, None, 1.0, torch.float64, ())
    torch.testing.assert_close(torch.cat([ea, ep, en]).detach().cpu().double(), e64, rtol=1e-5, atol=1e-5)
    torch.testing.assert_close(torch.cat([dp, dn]).detach().cpu().double(), d64, rtol=1e-5, atol=1e-5)
    # ... and a supported head takes the kernel
    head2 = _Head(64, 64, 0.0).cuda().eval()
    names = []
    prev, nat.trace = nat.trace, names
    try:
        ST.tripletnet(head2)._tail(torch.randn(3, 128).cuda())
    finally:
        nat.trace = prev
    assert [t[0] for t in names] == ["mlp3_triplet_fwd_f32"]


# ------------------------------------------------------------------------------------------------ 2 + 3. the whole step vs the oracle
STEP_CASES = [(c, conv, ub, mode) for c in ("n1_noedges", "odd", "spread") for conv in ("gcn", "sage") for ub in (False, True)
              for mode in ("eval", "train")] + [("dd", "gcn", False, "train"), ("dd", "sage", True, "eval")]


@pytest.mark.parametrize("case,conv,use_batch,mode", STEP_CASES)
def test_step_vs_three_single_graph_oracle_calls(case, conv, use_batch, mode):
    from two_stage_gnn_amd import _native as nat, message_passing as mp, sag_triplet as ST
    fin, nhid, C, graphs = _triplet(case)
    p_drop = 0.5 if mode == "train" else 0.0
    net = _net(fin, nhid, C, conv, use_batch, p_drop, seed=NET_SEED)
    net.train(mode == "train")
    p64, p32 = _params(net, torch.float64), _params(net, torch.float32)
    amb = [b for b, (x, ei) in enumerate(graphs) if _ambiguous(p64, x, ei, conv)]
    if amb:
        pytest.skip("the fp64 oracle's own top-k cut is ambiguous for graph(s) %s of this triplet" % amb)
    tnet = ST.tripletnet(net)
    datas = [_D(x, ei) for x, ei in graphs]
    names = []
    prev, nat.trace = nat.trace, names
    try:
        dp, dn, ea, ep, en = tnet(*datas)
        loss = ST.MarginRankingLoss(margin=1.5)(dp, dn, torch.full((1,), -1.0, device="cuda"))
        loss.backward()
    finally:
        nat.trace = prev
    launched = [t[0] for t in names]
    assert "mlp3_triplet_fwd_f32" in launched and "mlp3_triplet_bwd_f32" in launched, launched
    assert any(k.startswith("sag_pool_graph") for k in launched), launched          # the fused node, not the composed operators
    assert net.use_batch == use_batch
    keep, scale = None, 1.0
    if mode == "train":
        pd, seed, used = mp.last_mlp3_dropout
        keep, scale = mp.mlp3_dropout_mask(pd, seed, used, 3, nhid).cpu(), 1.0 / (1.0 - pd)
    dp64, dn64, e64, l64 = _oracle_step(p64, graphs, conv, keep, scale)
    dp32, dn32, e32, l32 = _oracle_step(p32, graphs, conv, keep, scale)
    assert l64 > 0.0                                       # the hinge is active: the gradients below are not all zero
    for name, got, r64, r32 in (("embed_a", ea, e64[0], e32[0]), ("embed_p", ep, e64[1], e32[1]), ("embed_n", en, e64[2], e32[2]),
                                ("dist_p", dp, dp64, dp32), ("dist_n", dn, dn64, dn32)):
        diff = (got.detach().cpu().double() - r64).abs()
        err, e_cpu = float(diff.max()), float((r32.double() - r64).abs().max())
        print("%s %s: |hip - fp64| %.2e, |cpu fp32 - fp64| %.2e" % (case, name, err, e_cpu))
        within = bool((diff <= 1e-5 + 1e-5 * r64.abs()).all())                    # rtol = atol = 1e-5
        if name.startswith("dist"):                           # fp32 distances: 10 x the fp32 oracle's own error arbitrates
            within = within or err <= 10.0 * e_cpu
        assert within, (name, err, e_cpu)
    assert abs(float(loss) - l64) <= max(1e-5 * max(1.0, abs(l64)), 10 * abs(l32 - l64))
    for k, q in net.named_parameters():
        r64, r32 = p64[k].grad, p32[k].grad
        assert q.grad is not None and r64 is not None, k
        err = float((q.grad.cpu().double() - r64).abs().max())
        bound, e_cpu = _bound(r64, r32, 1e-4, 1e-9)
        assert err <= bound, (k, err, e_cpu, float(r64.abs().max()))


def test_case_list_has_no_ambiguous_triplet():
    """the skip above can hide a failure, so: with these seeds the fp64 oracle alone reports NO ambiguous graph (at most one triplet of
    the list may ever be excluded)"""
    skipped = 0
    for case, conv in sorted({(c, v) for c, v, _, _ in STEP_CASES}):
        fin, nhid, C, graphs = _triplet(case)
        p64 = _params(_net(fin, nhid, C, conv, False, 0.0, seed=NET_SEED, dev="cpu"), torch.float64)
        skipped += any(_ambiguous(p64, x, ei, conv) for x, ei in graphs)
    assert skipped == 0, skipped


# ------------------------------------------------------------------------------------------------ 4. equals the hand composition
def _hand(net, datas):
    """what the parent commit offers for this step: three Net forwards at B = 1 + torch distances"""
    e = [net(d) for d in datas]
    return F.pairwise_distance(e[0], e[1], 2), F.pairwise_distance(e[0], e[2], 2), e[0], e[1], e[2]


@pytest.mark.parametrize("case,conv", [("odd", "gcn"), ("odd", "sage"), ("spread", "gcn"), ("spread", "sage")])
def test_fused_triplet_equals_three_fused_single_graph_forwards(case, conv):
    from two_stage_gnn_amd import sag_triplet as ST
    fin, nhid, C, graphs = _triplet(case)
    net = _net(fin, nhid, C, conv, True, 0.0, seed=NET_SEED).eval()
    datas = [_D(x, ei) for x, ei in graphs]
    assert net._fused_ok()
    with torch.no_grad():
        got = ST.tripletnet(net)(*datas)
        want = _hand(net, datas)
    for a, b in zip(got, want):
        assert a.shape == b.shape
        torch.testing.assert_close(a, b, rtol=1e-5, atol=1e-5)


@pytest.mark.parametrize("why", ["fused_off", "sage_directed", "sage_large_graph"])
def test_inputs_the_fused_node_does_not_take_run_composed(why):
    from two_stage_gnn_amd import _native as nat, sag_triplet as ST
    fin, nhid, C, graphs = _triplet("odd")
    if why == "sage_large_graph":
        graphs[0] = _graph(5, int(nat.lib().tsgnn_sag_pool_graph_max_nodes()) + 37, fin, 1.5)
    elif why == "sage_directed":
        graphs[0] = _graph(5, 21, fin, sym=False)
    net = _net(fin, nhid, C, "gcn" if why == "fused_off" else "sage", False, 0.0, seed=NET_SEED).eval()
    datas = [_D(x, ei) for x, ei in graphs]
    with torch.no_grad():
        if why == "fused_off":                             # the same triplet through both routes
            want = ST.tripletnet(net)(*datas)
            net.fused = False
        names = []
        prev, nat.trace = nat.trace, names
        try:
            got = ST.tripletnet(net)(*datas)
        finally:
            nat.trace = prev
        assert not any(t[0].startswith("sag_pool_graph") for t in names)
        if why != "fused_off":
            net.use_batch = True
            want = _hand(net, datas)
    for a, b in zip(got, want):
        torch.testing.assert_close(a, b, rtol=1e-5, atol=1e-5)


# ------------------------------------------------------------------------------------------------ 5. trainer integration
@pytest.mark.parametrize("conv", ["gcn", "sage"])
def test_flat_trainer_steps_equal_torch_adam_on_the_composed_route(conv):
    """three optimiser steps: the fused triplet under FlatTrainer (gradients straight into the flat bucket, clip 2.0 + Adam in the
    library's kernels, one hipGraph) against autograd + clip_grad_norm_ + torch.optim.Adam on the composed operators and the torch tail"""
    from two_stage_gnn_amd import sag_triplet as ST
    from two_stage_gnn_amd.data_parallel import FlatTrainer, GraphedStep
    fin, nhid, C, graphs = _triplet("odd")
    m1 = _net(fin, nhid, C, conv, False, 0.0, seed=NET_SEED).train()
    m2 = copy.deepcopy(m1)
    m2.fused = False
    datas = [_D(x, ei) for x, ei in graphs]
    tgt = torch.full((1,), -1.0, device="cuda")
    net2, crit2 = ST.tripletnet(m2), torch.nn.MarginRankingLoss(margin=1.5)
    b2 = net2.batch(*datas)
    params2 = list(m2.parameters())
    opt = torch.optim.Adam(params2, lr=1e-3)
    for _ in range(3):
        opt.zero_grad(set_to_none=True)
        dp, dn = net2._torch_tail(net2._readout(b2))[:2]
        crit2(dp, dn, tgt).backward()
        torch.nn.utils.clip_grad_norm_([q for q in params2 if q.grad is not None], 2.0)
        opt.step()
    net1, crit1 = ST.tripletnet(m1), ST.MarginRankingLoss(margin=1.5)
    b1 = net1.batch(*datas)
    tr = FlatTrainer(m1, lr=1e-3, clip=2.0)
    gs = GraphedStep(tr, lambda: crit1(*net1.embed(b1)[:2], tgt), warmup=3)          # (warm-up steps are rolled back)
    assert gs.describe().startswith("one graph"), gs.describe()
    for _ in range(3):
        gs.step()
    assert gs.loss_value() > 0.0
    for (k, q1), (_, q2) in zip(m1.named_parameters(), m2.named_parameters()):
        assert q2.grad is not None, k
        torch.testing.assert_close(q1.detach(), q2.detach(), rtol=2e-4, atol=2e-6, msg=lambda s_, k=k: k + ": " + s_)


def test_refilled_features_of_a_resident_triplet_are_followed_by_replays():
    """GraphedStep's contract: refill the resident input between replays.  Losses and parameters after every replay equal those of an
    eager twin fed the same sequence"""
    from two_stage_gnn_amd import sag_triplet as ST
    from two_stage_gnn_amd.data_parallel import FlatTrainer, GraphedStep
    fin, nhid, C, graphs = _triplet("odd")
    datas = [_D(x, ei) for x, ei in graphs]
    tgt = torch.full((1,), -1.0, device="cuda")
    nets = [ST.tripletnet(_net(fin, nhid, C, "sage", False, 0.0, seed=NET_SEED).train()) for _ in range(2)]
    crit = ST.MarginRankingLoss(margin=1.5)
    bs = [t.batch(*datas) for t in nets]
    trainers = [FlatTrainer(t.model, lr=1e-2, clip=2.0) for t in nets]
    fns = [lambda t=t, b=b: crit(*t.embed(b)[:2], tgt) for t, b in zip(nets, bs)]
    gs = GraphedStep(trainers[0], fns[0], warmup=3)
    assert gs.describe().startswith("one graph"), gs.describe()
    n = bs[0].x.size(0)
    for i in range(4):
        xi = tie_free(300 + i, n, fin).cuda() * (1.0 + i)
        for b in bs:
            b.x.copy_(xi)
        gs.step()
        l_graph = gs.loss_value()
        l_eager = float(trainers[1].step(fns[1]))
        assert abs(l_graph - l_eager) <= 1e-5 * max(1.0, abs(l_eager)), (i, l_graph, l_eager)
        for (k, a), b in zip(nets[0].model.named_parameters(), nets[1].model.parameters()):
            scale = float(b.detach().abs().max()) + 1e-30
            assert float((a.detach() - b.detach()).abs().max()) <= 1e-5 * scale, (i, k)


# ------------------------------------------------------------------------------------------------ 6. the resident cache
def test_second_step_on_the_same_objects_uploads_no_graph_structure(monkeypatch):
    from two_stage_gnn_amd import sag_stack as SS, sag_triplet as ST, triplet as T3
    fin, nhid, C, graphs = _triplet("odd")
    net = _net(fin, nhid, C, "gcn", False, 0.0, seed=NET_SEED).eval()
    datas = [_D(x, ei) for x, ei in graphs]
    tnet = ST.tripletnet(net)
    with torch.no_grad():
        first = tnet(*datas)
        c = tnet.cache
        assert (c.hits, c.misses, c.h2d, len(c)) == (0, 3, 6, 3)
        plans = len(SS.SagPlan._cache)
        second = tnet(*datas)
        assert (c.hits, c.misses, c.h2d, len(c)) == (3, 3, 6, 3) and len(SS.SagPlan._cache) == plans
        again = tnet(datas[0], datas[0], datas[2])         # anchor and positive the same object
        assert c.h2d == 6 and abs(float(again[0]) - 1e-6 * np.sqrt(C)) <= 1e-5
        monkeypatch.setattr(T3, "RESIDENT", False)         # TSGNN_TRIPLET_CACHE=0
        off = ST.tripletnet(net)
        third = off(*datas)
        assert len(off.cache) == 0 and off.cache.h2d == 6
        off(*datas)
        assert off.cache.h2d == 12
    for a, b, d in zip(first, second, third):
        torch.testing.assert_close(a, b, rtol=1e-6, atol=1e-7)
        torch.testing.assert_close(a, d, rtol=1e-6, atol=1e-7)
