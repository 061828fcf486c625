"""Host side of the row panels' gather schedule (two_stage_gnn_amd/graph.py pack_gather_schedule, GraphBatch.gather_schedule;
format: include/tsgnn.h): the packer's invariants, the batches it is stated to fit, and when no schedule is handed out."""
import numpy as np
import pytest
import torch

from two_stage_gnn_amd import graph as G
from two_stage_gnn_amd import synthetic

SHAPES = [(8, 32), (16, 24)]


def _decode(rec, shape):
    """-> {panel row (global): [ids]} and the groups used per panel; asserts the structural rules of a record on the way"""
    ng, S = shape
    P = rec.shape[0]
    assert rec.shape == (P, ng, 4 + S) and rec.dtype == np.int32
    rows, used_groups = {}, []
    for p in range(P):
        nxt = 0                                               # panel rows are handed out in order, group after group
        used = 0
        for q in range(ng):
            first, start, end, short = (int(v) & 0xFFFFFFFF for v in rec[p, q, :4])
            ids = rec[p, q, 4:]
            if start == 0:
                assert end == 0 and short == 0 and (ids == -1).all(), "an unused group carries nothing"
                continue
            used = q + 1
            assert first == nxt, "a group owns consecutive rows, from where the previous group stopped"
            assert start < (1 << S) and end < (1 << S) and (short & ~start) == 0
            assert start & 1, "a group's first slot opens a row"
            cur, open_ = None, False
            for s in range(S):
                if (start >> s) & 1:
                    assert not open_, "a row is closed before the next one opens"
                    cur, open_ = 32 * p + nxt, True
                    assert cur not in rows, "every panel row is opened exactly once"
                    rows[cur] = [[], bool((short >> s) & 1)]
                    nxt += 1
                if open_:
                    rows[cur][0].append(int(ids[s]))
                else:
                    assert ids[s] == -1, "slots behind the group's last row are empty"
                if (end >> s) & 1:
                    assert open_
                    open_ = False
            assert not open_, "a row never spans groups"
        assert nxt == 32, "all 32 panel rows are written"
        used_groups.append(used)
    return rows, used_groups


def _check(rowptr, col, n_rows, shape, row_slot=None, balance=True):
    rec = G.pack_gather_schedule(rowptr, col, n_rows, shape, row_slot, balance=balance)
    assert rec is not None
    rows, used = _decode(rec, shape)
    P = -(-n_rows // 32)
    assert sorted(rows) == list(range(32 * P))
    edges = 0
    for r in range(32 * P):
        ids, short = rows[r]
        nb = [int(c) for c in col[rowptr[r]:rowptr[r + 1]]] if r < n_rows else []
        if row_slot is not None:
            nb = [(int(row_slot[c]) << 20) | c for c in nb]
        assert ids == (nb if nb else [-1]), "every edge once, in the row's neighbour order"
        assert short == (len(nb) < 8)
        edges += len(nb)
    assert edges == int(rowptr[n_rows])
    return used


def _random_csr(rng, n, maxdeg):
    deg = rng.integers(0, maxdeg + 1, n)
    deg[rng.integers(0, n, max(1, n // 5))] = 0
    rowptr = np.concatenate([[0], np.cumsum(deg)]).astype(np.int32)
    col = rng.integers(0, n, int(rowptr[-1])).astype(np.int32)
    return rowptr, col


@pytest.mark.parametrize("shape", SHAPES)
def test_packer_invariants_on_random_small_graphs(shape):
    rng = np.random.default_rng(5)
    for n, maxdeg in ((1, 0), (31, 3), (32, 5), (33, 6), (108, 4), (200, 5)):
        rowptr, col = _random_csr(rng, n, maxdeg)
        _check(rowptr, col, n, shape)
        _check(rowptr, col, n, shape, balance=False)
        _check(rowptr, col, n, shape, row_slot=rng.integers(0, 1000, n))
    # rows of exactly S neighbours, alone in their groups
    S = shape[1]
    deg = np.array([S, 0, S, 1, 8, 7, 9], dtype=np.int64)
    rowptr = np.concatenate([[0], np.cumsum(deg)]).astype(np.int32)
    _check(rowptr, rng.integers(0, 7, int(rowptr[-1])).astype(np.int32), 7, shape)


BATCHES = [("DD", 32, 1000, s) for s in range(8)] + [("PROTEINS", 64, 620, 1), ("MUTAG", 32, 1000, 0)]


@pytest.mark.parametrize("shape_name,B,nmax,seed", BATCHES)
def test_both_shapes_pack_every_panel_of_the_stated_batches(shape_name, B, nmax, seed):
    hb = synthetic.host_batch(seed, B, shape_name, nmax)
    n = int(hb["sizes"].sum())
    used = _check(hb["rowptr"], hb["col"], n, (8, 32), balance=False)
    assert max(used) <= 7                                     # (greedy packing leaves a group to spare)
    _check(hb["rowptr"], hb["col"], n, (16, 24), balance=False)
    # balanced (what the launches get): the same rules, every group of a full panel at work, no lane's list longer than greedy's
    for shape in SHAPES:
        used = _check(hb["rowptr"], hb["col"], n, shape)
        assert min(used[:-1] or [shape[0]]) >= shape[0] - 1
        rec = G.pack_gather_schedule(hb["rowptr"], hb["col"], n, shape)
        fill = (rec[:, :, 4:] >= 0).sum(axis=2).max(axis=1)
        assert fill.mean() < 0.8 * shape[1]


def test_none_for_a_row_above_s_and_for_a_panel_that_does_not_pack():
    for shape in SHAPES:
        S = shape[1]
        deg = np.array([3, S + 1, 2], dtype=np.int64)
        rowptr = np.concatenate([[0], np.cumsum(deg)]).astype(np.int32)
        assert G.pack_gather_schedule(rowptr, np.zeros(int(rowptr[-1]), np.int32), 3, shape) is None
    # 32 rows of 17 neighbours: one row per group of 32 (or 24) slots, 32 groups needed
    rowptr = (17 * np.arange(33)).astype(np.int32)
    for shape in SHAPES:
        assert G.pack_gather_schedule(rowptr, np.zeros(17 * 32, np.int32), 32, shape) is None
    with pytest.raises(ValueError):
        G.pack_gather_schedule(rowptr, np.zeros(17 * 32, np.int32), 32, (16, 16))


def _host_graphbatch(hb, with_slots=False):
    g = G.GraphBatch()
    g.sizes = np.asarray(hb["sizes"], dtype=np.int64)
    g.B, g.nmax = len(g.sizes), int(hb["nmax"])
    g.n_rows, g.n_ghost = int(g.sizes.sum()), int(hb["nmax"])
    g.rowptr, g.col, g.val = torch.from_numpy(hb["rowptr"]), torch.from_numpy(hb["col"]), None
    g.device = torch.device("cpu")
    if with_slots:
        g.row_slot = torch.from_numpy(np.concatenate([np.arange(s) for s in g.sizes]).astype(np.int32))
    return g


def test_unit_cut_rule_mirrors_the_launches():
    assert not G.unit_cut(255 * 32, 256) and not G.unit_cut(256 * 32, 256)
    assert G.unit_cut(256 * 32 + 1, 256) and G.unit_cut(384 * 32, 256)
    assert not G.unit_cut(385 * 32, 256)                       # (far more panels than units: plain panels again)
    assert not G.unit_cut(271 * 32, 256, panel_units=False) and not G.unit_cut(300, 4)


def test_gather_schedule_of_a_batch_and_when_it_is_none():
    hb = synthetic.host_batch(3, 32, "DD", 1000)               # 271 panels
    g = _host_graphbatch(hb, with_slots=True)
    assert -(-g.n_rows // 32) == 271
    assert g.gather_schedule((8, 32), ncu=256) is None          # cut into units on a 256-unit device
    s = g.gather_schedule((8, 32), ncu=304)
    assert s is not None and s.dtype == torch.int32 and tuple(s.shape) == (271, 8, 36)
    assert g.gather_schedule((8, 32), ncu=304) is s             # cached per batch structure
    t = g.gather_schedule((8, 32), slots=True, ncu=304)
    ids, idt = s[:, :, 4:].numpy(), t[:, :, 4:].numpy()
    assert ((idt >= 0) == (ids >= 0)).all() and ((idt[ids >= 0] & 0xFFFFF) == ids[ids >= 0]).all()
    assert ((idt[ids >= 0] >> 20) == g.row_slot.numpy()[ids[ids >= 0]]).all()
    assert tuple(g.gather_schedule((16, 24), ncu=304).shape) == (271, 16, 28)
    g.val = torch.ones(int(hb["rowptr"][-1]))                   # weighted graph
    g.__dict__.pop("_gather_sched")
    assert g.gather_schedule((8, 32), ncu=304) is None
    g.val = None
    g.ghost_slots_fixed = 600                                   # capacity-padded (ingest) batch
    g.__dict__.pop("_gather_sched")
    assert g.gather_schedule((8, 32), ncu=304) is None
