"""The host half of the SAGPool triplet stream (two_stage_gnn_amd/sag_stream.py), no GPU: the arena against a plain-python restatement,
its refusals, the capacity plan against ``SagPlan`` for every triplet of both datasets, the k chain in float32, and the cap on what the
GPU tests may leave out of a comparison (no graph of either dataset has an ambiguous pooling cut in the fp64 oracle; exactly one schedule
entry per dataset names one object three times)."""
import itertools

import numpy as np
import pytest
import torch

import sag_stream_util as U


class _Data:
    def __init__(self, x, ei):
        self.x, self.edge_index = x, ei


def _ss():
    from two_stage_gnn_amd import sag_stream
    return sag_stream


@pytest.mark.parametrize("name", ["small6", "dd3"])
def test_arena_equals_a_plain_python_restatement(name):
    S = _ss()
    fin, _, _, graphs = U.dataset(name)
    ar = S.pack_arena(U.datas(graphs, "cpu"))
    rec, per = U.restate(graphs)
    assert ar.records.dtype == np.int32 and np.array_equal(ar.records, rec)
    assert ar.fin == fin and ar.ld == (fin + 3) // 4 * 4 and ar.n_graphs == len(graphs) and ar.total_nodes == sum(U.SIZES[name])
    assert ar.off["rowptr"] == 0 and ar.off["col"] % 4 == 0 and ar.off["col"] >= ar.total_nodes + len(graphs) and ar.words == ar.buf.size
    assert ar.feats.shape == (ar.total_nodes, ar.ld) and not ar.feats[:, fin:].any()
    for i, (rp, col, x) in enumerate(per):
        n, nnz, row0, ent0 = (int(v) for v in rec[i][:4])
        assert np.array_equal(ar.buf[ar.off["rowptr"] + row0 + i: ar.off["rowptr"] + row0 + i + n + 1], rp), i
        assert np.array_equal(ar.buf[ar.off["col"] + ent0: ar.off["col"] + ent0 + nnz], col), i
        assert np.array_equal(ar.feats[row0: row0 + n, :fin], x), i
    assert ar.caps == (3 * max(U.SIZES[name]), 3 * int(rec[:, 1].max())) and ar.largest == max(U.SIZES[name])
    if name == "small6":
        assert rec[1][1] == 0 and rec[0][0] == 1                     # the graph without edges, the single node


def test_arena_is_pack_hosts_order_with_repeated_edges_kept():
    from two_stage_gnn_amd import sag_triplet as ST
    S = _ss()
    x = torch.arange(12, dtype=torch.float32).view(4, 3)
    ei = torch.tensor([[1, 0, 2, 1, 1, 0, 3, 3], [0, 1, 1, 2, 0, 1, 3, 3]])          # 0 <-> 1 twice, a repeated self loop on 3
    d = _Data(x, ei)
    ar = S.pack_arena([d, d])
    rowptr, col, _, sizes, sym = ST.pack_host([d])
    assert sym == (True,) and col.size == 8
    for i in range(2):
        n, nnz, row0, ent0 = (int(v) for v in ar.records[i][:4])
        assert np.array_equal(ar.buf[row0 + i: row0 + i + n + 1], rowptr) and np.array_equal(ar.buf[ar.off["col"] + ent0:][:nnz], col)


def test_pack_arena_refuses():
    S = _ss()
    from two_stage_gnn_amd import _native as nat
    ok = _Data(torch.zeros(3, 2), torch.tensor([[0, 1], [1, 0]]))
    limit = int(nat.lib().tsgnn_sag_pool_graph_max_nodes())
    bad = {
        "at least one node": _Data(torch.zeros(0, 2), torch.zeros(2, 0, dtype=torch.long)),
        "exceed": _Data(torch.zeros(limit + 1, 2), torch.zeros(2, 0, dtype=torch.long)),
        "outside": _Data(torch.zeros(3, 2), torch.tensor([[0, 3], [3, 0]])),
        "not symmetric": _Data(torch.zeros(3, 2), torch.tensor([[0, 1, 0], [1, 0, 1]])),          # 0 -> 1 twice, 1 -> 0 once
        "feature width": _Data(torch.zeros(3, 4), torch.tensor([[0, 1], [1, 0]])),
    }
    for what, d in bad.items():
        with pytest.raises(ValueError, match="graph 1: .*" + what):
            S.pack_arena([ok, d])
    with pytest.raises(ValueError, match="graph 0: .*outside"):
        S.pack_arena([_Data(torch.zeros(3, 2), torch.tensor([[0, -1], [-1, 0]])), ok])
    with pytest.raises(ValueError, match="offsets reach"):
        S.pack_arena([ok, ok], limit=8)
    with pytest.raises(ValueError, match="no graphs"):
        S.pack_arena([])
    assert S.pack_arena([_Data(torch.zeros(limit, 2), torch.zeros(2, 0, dtype=torch.long))]).largest == limit


@pytest.mark.parametrize("name", ["small6", "dd3"])
def test_capacity_plan_bounds_every_triplets_plan(name):
    """N and max_seg of every level are at least SagPlan's for every triplet of the dataset, one object three times included, and are
    attained by the largest graph three times"""
    from two_stage_gnn_amd.sag_stack import SagPlan
    S = _ss()
    sizes = U.SIZES[name]
    cap = S.CapacityPlan(max(sizes), U.RATIO, 3)
    assert cap.capacity and cap.depth == 3 and len(cap.levels) == 4 and all(L.B == 3 for L in cap.levels)
    seen = 0
    for trip in itertools.product(sizes, repeat=3):
        plan = SagPlan(np.array(trip), U.RATIO, "cpu", 3)
        for L, Lc in zip(plan.levels, cap.levels):
            assert L.N <= Lc.N and L.max_seg <= Lc.max_seg and Lc.N == 3 * Lc.max_seg, (trip, L.N, Lc.N)
        if trip == (max(sizes),) * 3:
            assert [L.N for L in plan.levels] == [L.N for L in cap.levels]
        seen += 1
    assert seen == len(sizes) ** 3


@pytest.mark.parametrize("ratio", [0.5, 0.3])
def test_k_chain_is_sagplans_in_float32(ratio):
    from two_stage_gnn_amd.sag_stack import SagPlan
    S = _ss()
    ns = np.arange(1, 4097)
    plan = SagPlan(ns, ratio, "cpu", 3)
    chain = np.array([S.k_chain(int(n), ratio, 3) for n in ns])
    for l in range(4):
        assert np.array_equal(plan.levels[l].sizes, chain[:, l]), l
    assert (np.diff(chain, axis=0) >= 0).all()                       # k is monotone in n: the largest graph bounds every level
    if ratio == 0.3:
        k64 = np.minimum(np.ceil(ratio * ns.astype(np.float64)).astype(np.int64), ns)
        assert (k64 != chain[:, 1]).any()                            # the two precisions fall on different sides of an integer
        # float32(0.3) lies above 0.3, yet its float32 product with 10 rounds to exactly 3: k = 3, where the same ratio times 10 in
        # double gives 3.0000001 and k = 4
        assert float(np.float32(0.3) * np.float32(10)) == 3.0 and chain[9, 1] == 3 and float(np.float32(0.3)) * 10.0 > 3.0


@pytest.mark.parametrize("name", ["small6", "dd3"])
def test_no_graph_is_ambiguous_and_one_entry_names_one_object_three_times(name):
    """the cap on exclusions: no entry may be left out of a comparison for ambiguity, and the only entry whose gradient comparison may
    be skipped (a = p = n: d_p - d_n is identically zero) occurs exactly once"""
    fin, nhid, C, graphs = U.dataset(name)
    p64 = U._params(U._net(fin, nhid, C, "gcn", False, 0.0, seed=U.NET_SEED, dev="cpu"), torch.float64)
    assert [i for i, (x, ei) in enumerate(graphs) if U._ambiguous(p64, x, ei, "gcn")] == []
    sched = U.SCHEDULES[name]
    assert sched.shape == (5, 3) and int(sched.max()) < len(graphs)
    assert sum(len(set(r.tolist())) == 1 for r in sched) == 1 and sum(len(set(r.tolist())) == 2 for r in sched) >= 1
    sizes = np.array(U.SIZES[name])
    tot = sizes[sched].sum(1)
    assert tot[0] == max(tot[:-1]) and tot[1] == min(tot[:4])        # the largest triplet first, then the smallest of the mixed ones
