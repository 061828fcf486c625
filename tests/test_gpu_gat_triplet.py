"""gat_triplet on the GPU: the batch assembler (csrc/gat_assemble.hip) array by array against the dense conversion, the tripletnet
drop-in against three B = 1 calls of the module and against the reference's own fixtures, the resident cache, the fallbacks, a
FlatTrainer step, and stage two through packed chunks."""
import copy

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import load_golden
from util_graphs import dense_batch
import test_gat_triplet_host as H

pytestmark = pytest.mark.gpu

MARGIN = 10.0          # (distances of these models are ~1: the hinge max(0, dist_p - dist_n + margin) is active)


def _dev():
    return torch.device("cuda", torch.cuda.current_device())


# ------------------------------------------------------------------------------------------------ the assembler alone
ASM_NMAX = 12
# (n, kind): a full graph, n = 1, an edge-less graph, directed ones, a second full one; 11 graphs = two launches
ASM_GRAPHS = [(9, "directed"), (12, "sym"), (1, "sym"), (7, "empty"), (10, "sym"), (5, "sym"), (11, "sym"), (12, "directed"), (6, "sym"),
              (3, "directed"), (8, "sym")]


def _sorted_in_rows(values, rowptr):
    """values sorted inside each CSR row"""
    rows = torch.repeat_interleave(torch.arange(rowptr.numel() - 1, device=values.device), (rowptr[1:] - rowptr[:-1]).long())
    key = rows.long() * (1 << 32) + values.long()
    return torch.sort(key).values


@pytest.mark.parametrize("fin", [3, 8])
@pytest.mark.parametrize("K", [1, 3, 5, 8, 11])
def test_assembler_equals_the_dense_conversion(K, fin):
    from two_stage_gnn_amd import attention as att, gat_triplet as GT, message_passing as mp, resident as R
    from two_stage_gnn_amd.graph import GraphBatch
    dev = _dev()
    objs = [H.make_obj(100 + i, n, nmax=ASM_NMAX, fin=fin, kind=kind) for i, (n, kind) in enumerate(ASM_GRAPHS[:K])]
    cache = R.ResidentCache()
    parts = [GT.resident_piece(o, dev, cache) for o in objs]
    assert cache.h2d == K
    if K >= 3:                                             # a piece starts off 16 bytes in rows and in entries: the scalar head / tail run
        e0, r0 = np.cumsum([p.nnz for p in parts])[:-1], np.cumsum([p.nr for p in parts])[:-1]
        assert (e0 % 4 != 0).any() and (r0 % 4 != 0).any() and any(p.nnz % 4 for p in parts)
    heads = (2, 3)
    guard = 8
    x, g = GT.assemble(parts, dev, heads, guard=guard)
    torch.cuda.synchronize()
    # the same graphs through the dense conversion
    adj = torch.as_tensor(np.stack([(np.asarray(o.graph["adj"]) > 0).astype(np.float32) for o in objs])).to(dev)
    feats = torch.as_tensor(np.stack([o.graph["feats"] for o in objs])).to(dev)
    sizes = np.array([o.graph["num_nodes"] for o in objs])
    ref = GraphBatch.from_dense_ghost1(adj, sizes)
    rp_t, col_t, src_e_t = ref.transpose_map()
    nnz, rows = ref.nnz, ref.n_rows
    assert (g.B, g.nmax, g.n_rows, g.n_ghost, g.nnz, g.layout) == (ref.B, ref.nmax, rows, 0, nnz, "packed")
    assert np.array_equal(g.sizes, ref.sizes) and np.array_equal(g.real_sizes, ref.real_sizes)
    assert torch.equal(g.rowptr, ref.rowptr) and torch.equal(g.col[:nnz], ref.col[:nnz])
    assert torch.equal(g.graph_ptr, ref.graph_ptr) and torch.equal(g.row_graph[:rows], ref.row_graph[:rows])
    assert torch.equal(g.row_slot[:rows], ref.row_slot[:rows]) and torch.equal(g.row_mult, ref.row_mult)
    mine_t = g.transpose_map()
    assert torch.equal(mine_t[0], rp_t)
    assert torch.equal(_sorted_in_rows(mine_t[1][:nnz], rp_t), _sorted_in_rows(col_t[:nnz], rp_t))
    assert torch.equal(_sorted_in_rows(mine_t[2][:nnz], rp_t), _sorted_in_rows(src_e_t[:nnz], rp_t))
    if nnz:
        ar = torch.arange(nnz, device=dev, dtype=torch.int32)
        inv = att._inverse_entry_map(g, mine_t[2])
        assert inv is g._inv_e_t and torch.equal(inv[:nnz][mine_t[2][:nnz].long()], ar)                  # the inverse really inverts
        assert torch.equal(g.col[:nnz][mine_t[2][:nnz].long()].long(),                                   # col[src_e_t[p]] = p's transposed row
                           torch.repeat_interleave(torch.arange(rows, device=dev), (rp_t[1:] - rp_t[:-1]).long()))
    for h in heads:
        assert torch.equal(att._isolated_columns(g, mine_t[0], rows, h), att._isolated_columns(ref, rp_t, rows, h))
    lst, lst_ref = att._isolated_list(g, None, force=True), att._isolated_list(ref, att._isolated_columns(ref, rp_t, rows, 2), force=True)
    n_listed = att.isolated_count(ref)
    assert att.isolated_count(g) == n_listed and n_listed > 0
    assert torch.equal(lst[0][:n_listed], lst_ref[0]) and torch.equal(lst[1][:n_listed], lst_ref[1]) and torch.equal(lst[2], lst_ref[2])
    ld = (fin + 3) // 4 * 4
    assert x.shape == (rows, ld) and torch.equal(x, mp.pack_rows(feats, ref, ld))
    # nothing behind the arrays' ends was written
    ibuf, fbuf, ioff, isz, foff, fsz = g._raw
    for buf, offs, lens in ((ibuf.cpu().numpy(), ioff, isz), (fbuf.view(torch.int32).cpu().numpy(), foff, fsz)):
        keep = np.ones(buf.size, dtype=bool)
        for o, n in zip(offs, lens):
            keep[int(o):int(o) + n] = False
        assert keep.sum() >= guard * len(lens) and (buf[keep] == GT.GUARD).all()
        assert not (buf[~keep] == GT.GUARD).any()                                                      # ... and every element before them was


def test_a_fifth_head_count_is_built_at_first_use():
    """the launch writes the indicator of four head counts; a fifth is made by attention._isolated_columns when a layer asks for it"""
    from two_stage_gnn_amd import attention as att, gat_triplet as GT, resident as R
    dev = _dev()
    objs = [H.make_obj(100 + i, n, nmax=ASM_NMAX, fin=3, kind=kind) for i, (n, kind) in enumerate(ASM_GRAPHS[:3])]
    parts = [GT.resident_piece(o, dev, R.ResidentCache()) for o in objs]
    x, g = GT.assemble(parts, dev, (1, 2, 3, 4, 5))
    assert sorted(g._iso_cols) == [1, 2, 3, 4]
    rp_t = g.transpose_map()[0]
    five = att._isolated_columns(g, rp_t, g.n_rows, 5)
    assert five.shape == (g.n_rows, 5) and torch.equal(five[:, :4], g._iso_cols[4]) and torch.equal(five[:, 4], g._iso_cols[1][:, 0])


# ------------------------------------------------------------------------------------------------ the model
def _objs(seed, sizes, nmax, fin, p_edge=0.25):
    x, adj, sz = dense_batch(seed, len(sizes), nmax, fin, sizes=sizes, p_edge=p_edge)
    return [H.GraphObj(adj[b].numpy(), x[b].numpy(), int(sz[b]), label=b % 2) for b in range(len(sizes))], x, adj, sz


def _model(fin, layers, final_dim, **kw):
    from two_stage_gnn_amd import gat_encoders as G
    return G.DGATEncoderGraph(fin, 8, 8, 2, None, num_layers=layers, num_heads=[2] * layers, neg_input_slopes=[0.2] * layers,
                              dropouts=kw.pop("dropouts", [0.0] * layers), final_dim=final_dim, **kw).cuda()


def _three_calls(m, x, adj, sz, sizes_arg=True):
    """the reference's three B = 1 forwards of the module itself + torch's distances"""
    e = [m(x[b:b + 1].cuda(), adj[b:b + 1].cuda(), sz[b:b + 1] if sizes_arg else None)[1] for b in range(3)]
    return F.pairwise_distance(e[0], e[1], 2), F.pairwise_distance(e[0], e[2], 2), e[0], e[1], e[2]


def _flags(m):
    from two_stage_gnn_amd.gat_encoders import DGATHead
    return [hd.per_graph_features for hd in m.modules() if isinstance(hd, DGATHead)]


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


def _check_against(m1, o1, m2, o2):
    for a, b in zip(o1, o2):
        torch.testing.assert_close(a, b, rtol=1e-4, atol=1e-5)
    for (k, q1), q2 in zip(m1.named_parameters(), m2.parameters()):
        assert (q1.grad is None) == (q2.grad is None), k
        if q2.grad is not None:
            bound = 5e-3 * float(q2.grad.abs().max()) + 1e-6
            err = float((q1.grad - q2.grad).abs().max())
            assert err <= bound, (k, err, bound)


@pytest.mark.parametrize("final_dim", ["output_dim", "number_classes"])
@pytest.mark.parametrize("layers", [2, 3])
def test_tripletnet_equals_three_single_graph_calls(layers, final_dim):
    """a default-constructed encoder (per_graph_features=False: input[0] for every graph of a batch, so any batched route through the
    module itself computes positive and negative from the anchor's features) gives the three B = 1 forwards"""
    from two_stage_gnn_amd import gat_triplet as GT
    fin = 8
    objs, x, adj, sz = _objs(71, [20, 9, 14], 20, fin)
    torch.manual_seed(3)
    m1 = _model(fin, layers, final_dim)
    m2 = copy.deepcopy(m1)
    assert _flags(m1) == [False] * (2 * layers)
    net = GT.tripletnet(m1)
    o1 = net(*objs)
    assert len(net.cache) == 3 and "_TripletTailBackward" in _node_names(o1[0]) and "_GatLayerBackward" in _node_names(o1[0])
    assert _flags(m1) == [False] * (2 * layers)                         # the model's flag is what it was
    GT.MarginRankingLoss(margin=MARGIN)(o1[0], o1[1], torch.full_like(o1[0], -1.0)).backward()
    o2 = _three_calls(m2, x, adj, sz)
    loss2 = torch.nn.MarginRankingLoss(margin=MARGIN)(o2[0], o2[1], torch.full_like(o2[0], -1.0))
    assert float(loss2.detach()) > 0
    loss2.backward()
    assert float((o2[3] - o2[2]).abs().max()) > 1e-2                    # (the three graphs do differ: T4 would be visible)
    _check_against(m1, o1, m2, o2)


def test_tripletnet_with_graphs_without_any_edge_equals_three_single_graph_calls():
    """the n = 1 graph (no self loop) and the edge-less graph of ASM_GRAPHS next to a graph with edges: the module's B = 1 calls of the
    graphs with nnz = 0 are made like any other, and the drop-in's batch gives their outputs and gradients"""
    from two_stage_gnn_amd import gat_triplet as GT
    fin = 8
    objs = [H.make_obj(100 + i, ASM_GRAPHS[i][0], nmax=ASM_NMAX, fin=fin, kind=ASM_GRAPHS[i][1]) for i in (2, 3, 0)]
    adj = torch.as_tensor(np.stack([(np.asarray(o.graph["adj"]) > 0).astype(np.float32) for o in objs]))
    x = torch.as_tensor(np.stack([np.asarray(o.graph["feats"], dtype=np.float32) for o in objs]))
    sz = np.array([int(o.graph["num_nodes"]) for o in objs], dtype=np.int64)
    assert adj.sum(dim=(1, 2)).gt(0).tolist() == [False, False, True] and sz.tolist() == [1, 7, 9]
    torch.manual_seed(3)
    m1 = _model(fin, 2, "output_dim")
    m2 = copy.deepcopy(m1)
    o1 = GT.tripletnet(m1)(*objs)
    GT.MarginRankingLoss(margin=MARGIN)(o1[0], o1[1], torch.full_like(o1[0], -1.0)).backward()
    o2 = _three_calls(m2, x, adj, sz)
    loss2 = torch.nn.MarginRankingLoss(margin=MARGIN)(o2[0], o2[1], torch.full_like(o2[0], -1.0))
    assert float(loss2.detach()) > 0
    loss2.backward()
    _check_against(m1, o1, m2, o2)


def test_flag_is_restored_on_an_exception(monkeypatch):
    from two_stage_gnn_amd import gat_triplet as GT
    objs, *_ = _objs(71, [20, 9, 14], 20, 8)
    m = _model(8, 2, "output_dim")

    def boom(*a, **k):
        raise RuntimeError("boom")
    monkeypatch.setattr(m, "gcn_forward", boom)
    with pytest.raises(RuntimeError, match="boom"):
        GT.tripletnet(m)(*objs)
    assert _flags(m) == [False] * 4


def test_other_heads_take_the_modules():
    """a head that is not a single Linear (map2_model replaced) runs through the modules and resident.torch_distances"""
    from two_stage_gnn_amd import gat_triplet as GT
    objs, x, adj, sz = _objs(72, [20, 9, 14], 20, 8)
    torch.manual_seed(4)
    m1 = _model(8, 2, "output_dim")
    m1.map2_model = torch.nn.Sequential(torch.nn.ReLU(), torch.nn.Linear(8, 5)).cuda()
    m2 = copy.deepcopy(m1)
    o1 = GT.tripletnet(m1)(*objs)
    assert "_TripletTailBackward" not in _node_names(o1[0])
    (o1[0] - o1[1]).sum().backward()
    o2 = _three_calls(m2, x, adj, sz)
    (o2[0] - o2[1]).sum().backward()
    _check_against(m1, o1, m2, o2)


# ------------------------------------------------------------------------------------------------ the reference's own fixtures
@pytest.mark.parametrize("name", H.FIXTURES)
def test_drop_in_matches_the_reference_tripletnet(name):
    from two_stage_gnn_amd import gat_encoders as G, gat_triplet as GT
    g = load_golden(name)
    fin, hid, emb, lab = (int(v) for v in g["dims"])
    m = G.DGATEncoderGraph(fin, hid, emb, lab, None, num_layers=int(g["num_layers"]), num_heads=[int(h) for h in g["heads"]],
                           final_dim=str(g["final_dim"]))
    m.load_state_dict({k[2:]: torch.tensor(v) for k, v in g.items() if k.startswith("p.")}, strict=True)
    m = m.cuda()
    net = GT.tripletnet(m)
    crit = GT.MarginRankingLoss(margin=float(g["margin"]))
    for t, trip in enumerate(H.triplets(g)):
        m.zero_grad(set_to_none=True)
        dp, dn, ea, e_p, en = net(*[H.GraphObj(a, f, n) for (a, f, n) in trip])
        loss = crit(dp, dn, torch.full_like(dp, -1.0))
        loss.backward()
        np.testing.assert_allclose(dp.detach().cpu().numpy(), g["t%d.dist_p" % t], rtol=1e-4, atol=1e-5)
        np.testing.assert_allclose(dn.detach().cpu().numpy(), g["t%d.dist_n" % t], rtol=1e-4, atol=1e-5)
        np.testing.assert_allclose(torch.cat([ea, e_p, en]).detach().cpu().numpy(), g["t%d.embed" % t], rtol=1e-4, atol=1e-5)
        np.testing.assert_allclose(float(loss.detach()), float(g["t%d.loss" % t]), rtol=1e-4, atol=1e-5)
        for k, p in m.named_parameters():
            ref = g["t%d.g.%s" % (t, k)]
            got = p.grad.cpu().numpy() if p.grad is not None else np.zeros_like(ref)
            np.testing.assert_allclose(got, ref, rtol=2e-3, atol=1e-4, err_msg="%d %s" % (t, k))


# ------------------------------------------------------------------------------------------------ cache and syncs
def test_second_call_uploads_nothing_and_does_not_wait_for_the_device():
    from two_stage_gnn_amd import gat_triplet as GT
    objs, *_ = _objs(73, [20, 9, 14], 20, 8)
    torch.manual_seed(5)
    m = _model(8, 2, "output_dim")
    net = GT.tripletnet(m)
    crit = GT.MarginRankingLoss(margin=MARGIN)
    first = net(*objs)
    crit(first[0], first[1], torch.full_like(first[0], -1.0)).backward()       # (first use: uploads, library load, allocator warm-up)
    c = net.cache
    assert (c.h2d, c.misses, c.hits, len(c)) == (3, 3, 0, 3)
    m.zero_grad(set_to_none=True)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        second = net(*objs)
        crit(second[0], second[1], torch.full_like(second[0], -1.0)).backward()
        with pytest.raises(RuntimeError):
            second[0].cpu()                                                 # (the mode is live: a copy to the host IS flagged)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert (c.h2d, c.misses, c.hits, len(c)) == (3, 3, 3, 3)
    for a, b in zip(first, second):
        assert torch.equal(a, b)
    assert all(torch.isfinite(q.grad).all() for q in m.parameters() if q.grad is not None)


# ------------------------------------------------------------------------------------------------ fallbacks
def test_dropout_in_training_mode_takes_the_dense_calls():
    from two_stage_gnn_amd import gat_triplet as GT
    objs, x, adj, sz = _objs(74, [20, 9, 14], 20, 8)
    torch.manual_seed(6)
    m1 = _model(8, 2, "output_dim", dropouts=[0.3, 0.3]).train()
    net = GT.tripletnet(m1)
    o = net(*objs)
    (o[0] - o[1]).sum().backward()
    assert len(net.cache) == 0 and net.cache.h2d == 0                       # nothing resident added by that call
    assert all(torch.isfinite(t).all() for t in o)
    grads = [q.grad for q in m1.parameters() if q.grad is not None]
    assert grads and all(torch.isfinite(t).all() for t in grads)
    # eval mode: dropout is off, the packed path, the B = 1 calls' numbers
    m1.eval()
    m2 = copy.deepcopy(m1)
    m1.zero_grad(set_to_none=True)
    o1 = net(*objs)
    assert len(net.cache) == 3 and "_TripletTailBackward" in _node_names(o1[0])
    (o1[0] - o1[1]).sum().backward()
    o2 = _three_calls(m2, x, adj, sz)
    (o2[0] - o2[1]).sum().backward()
    _check_against(m1, o1, m2, o2)


def test_padded_rows_that_differ_take_the_dense_calls():
    from two_stage_gnn_amd import gat_triplet as GT
    objs, x, adj, sz = _objs(75, [20, 9, 14], 20, 8)
    x[1, 12:] = torch.randn(8, 8, generator=torch.Generator().manual_seed(1))      # graph 1's padded rows differ from one another
    objs[1] = H.GraphObj(adj[1].numpy(), x[1].numpy(), 9)
    torch.manual_seed(7)
    m1 = _model(8, 2, "output_dim")
    m2 = copy.deepcopy(m1)
    net = GT.tripletnet(m1)
    o1 = net(*objs)
    assert net.cache.h2d == 2 and "_TripletTailBackward" not in _node_names(o1[0])
    (o1[0] - o1[1]).sum().backward()
    o2 = _three_calls(m2, x, adj, sz, sizes_arg=False)                      # all Nmax rows of every graph: the reference's arithmetic
    (o2[0] - o2[1]).sum().backward()
    _check_against(m1, o1, m2, o2)


def test_cache_off_takes_the_dense_calls(monkeypatch):
    from two_stage_gnn_amd import gat_triplet as GT, triplet as T3
    objs, x, adj, sz = _objs(76, [20, 9, 14], 20, 8)
    torch.manual_seed(8)
    m = _model(8, 2, "output_dim").eval()
    with torch.no_grad():
        on = GT.tripletnet(m)(*objs)
        monkeypatch.setattr(T3, "RESIDENT", False)                          # TSGNN_TRIPLET_CACHE=0
        from two_stage_gnn_amd import resident as R
        shared = R.resident_cache(m)
        before = (len(shared), shared.h2d, shared.hits, shared.misses)
        net = GT.tripletnet(m)
        off = net(*objs)
        assert net.cache is not shared and len(net.cache) == 0 and net.cache.h2d == 0
        assert (len(shared), shared.h2d, shared.hits, shared.misses) == before == (3, 3, 0, 3)    # the model's cache was not touched
    with torch.enable_grad():
        assert "_TripletTailBackward" not in _node_names(net(*objs)[0])                          # the dense calls, not the packed path
    for a, b in zip(on, off):
        torch.testing.assert_close(a, b, rtol=1e-4, atol=1e-5)


# ------------------------------------------------------------------------------------------------ FlatTrainer
def _reg_loss(crit, outs, tgt):
    """the margin loss + norm regularisers on the three embeddings (train_triplet.py:262-263): gradients reach the tail on the distances
    AND on the embeddings, so the head's bias has a gradient that is not pure rounding (the distances alone do not depend on it, and
    Adam normalises whatever noise it is given to a full-size update)"""
    dp, dn, ea, e_p, en = outs
    return crit(dp, dn, tgt) + 1e-2 * (ea.norm(2) + e_p.norm(2) + en.norm(2))


def test_step_under_flat_trainer_equals_torch_adam():
    """three optimiser steps: the resident triplet under FlatTrainer (the tail's dW / db straight into the flat bucket, clip 2.0 + Adam
    in the library's kernels, one hipGraph) against three B = 1 calls stepped by autograd + clip_grad_norm_ + torch.optim.Adam"""
    from two_stage_gnn_amd import gat_triplet as GT
    from two_stage_gnn_amd.data_parallel import FlatTrainer, GraphedStep
    objs, x, adj, sz = _objs(77, [20, 9, 14], 20, 8)
    torch.manual_seed(9)
    m1 = _model(8, 2, "output_dim").train()
    m2 = copy.deepcopy(m1)
    tgt = torch.tensor([-1.0]).cuda()
    crit2 = torch.nn.MarginRankingLoss(margin=MARGIN)
    params2 = list(m2.parameters())
    opt = torch.optim.Adam(params2, lr=1e-3)
    for _ in range(3):
        opt.zero_grad(set_to_none=True)
        _reg_loss(crit2, _three_calls(m2, x, adj, sz), tgt).backward()
        torch.nn.utils.clip_grad_norm_([p for p in params2 if p.grad is not None], 2.0)
        opt.step()
    net1, crit1 = GT.tripletnet(m1), GT.MarginRankingLoss(margin=MARGIN)
    b = net1.batch(*objs)
    tr = FlatTrainer(m1, lr=1e-3, clip=2.0)
    gs = GraphedStep(tr, lambda: _reg_loss(crit1, net1.embed(b), tgt), warmup=3)      # (warm-up steps are rolled back)
    for _ in range(3):
        gs.step()
    assert gs.loss_value() > 0
    for (k, p1), (_, p2) in zip(m1.named_parameters(), m2.named_parameters()):
        if p2.grad is None:
            continue
        torch.testing.assert_close(p1.detach(), p2.detach(), rtol=2e-4, atol=2e-6, msg=lambda s_, k=k: k + ": " + s_)


# ------------------------------------------------------------------------------------------------ stage two
STAGE2_SIZES = [12, 5, 9, 3, 11, 12, 1, 7, 10, 4, 8]


@pytest.fixture(scope="module")
def stage2():
    """11 graphs, a model, and the eval-mode B = 1 forward of every graph (computed once)"""
    objs, x, adj, sz = _objs(5, STAGE2_SIZES, 12, 6)
    torch.manual_seed(3)
    m = _model(6, 2, "output_dim").eval()
    with torch.no_grad():
        want = torch.cat([m(x[b:b + 1].cuda(), adj[b:b + 1].cuda(), sz[b:b + 1])[1] for b in range(len(objs))])
    return objs, m, want


@pytest.mark.parametrize("chunk", [1, 4, 8, 16])
def test_embed_dataset_in_packed_chunks(stage2, chunk):
    from two_stage_gnn_amd import gat_triplet as GT, resident as R, two_stage as TS
    objs, m, want = stage2
    got = TS.embed_dataset(GT.tripletnet(m), objs, chunk=chunk)
    assert got.is_cuda and not got.requires_grad and got.shape == want.shape
    torch.testing.assert_close(got, want, rtol=1e-4, atol=1e-4)
    assert len(R.resident_cache(m)) == len(objs) and R.resident_cache(m).h2d == len(objs)      # one upload per graph, whatever the chunk
    assert not m.training and _flags(m) == [False] * 4
    torch.testing.assert_close(TS.embed_dataset(m, objs, chunk=chunk), got, rtol=0, atol=0)    # a bare model with chunk= : the same path


def test_bare_model_without_chunk_keeps_the_plain_loop():
    from two_stage_gnn_amd import resident as R, two_stage as TS
    objs, x, adj, sz = _objs(5, STAGE2_SIZES[:4], 12, 6)
    torch.manual_seed(3)
    m = _model(6, 2, "output_dim").eval()
    TS.embed_dataset(m, objs)
    assert len(R.resident_cache(m)) == 0


def test_evaluate_equals_the_plain_loop_and_the_same_classifier():
    from two_stage_gnn_amd import gat_triplet as GT, two_stage as TS
    sizes = [12, 5, 9, 3, 11, 12, 2, 7, 10, 4, 8, 6] * 2
    objs, x, adj, sz = _objs(6, sizes, 12, 6)
    torch.manual_seed(4)
    m = _model(6, 2, "output_dim").eval()
    train, val = objs[:16], objs[16:]
    got = TS.evaluate(train, val, GT.tripletnet(m), n_neighbors=3, chunk=5)
    emb = TS.embed_dataset(m, objs)                                             # the plain loop
    conf, _ = TS.knn_confusions(emb[:16], TS._labels(train), emb[16:], TS._labels(val), 3)
    want = TS.metrics_from_confusion(conf[0])
    want["train acc"] = int(np.trace(conf[1])) / int(conf[1].sum())
    assert got == want
    assert set(TS.evaluate_mlp(train, val, GT.tripletnet(m), hidden=(16, 8))) == {"acc"}
