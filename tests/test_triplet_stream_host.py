"""Host side of the triplet stream (two_stage_gnn_amd/triplet_stream.py), no GPU: ``pack_arena`` against a plain-python restatement
array by array, every refusal, the exact capacities, the schedule checks of ``load`` and ``schedule_of`` on a stub sampler."""
import copy

import numpy as np
import pytest

import triplet_stream_util as U


def _ts():
    from two_stage_gnn_amd import triplet_stream as TS
    return TS


def test_pack_arena_equals_the_restatement_array_by_array():
    TS = _ts()
    graphs = U.dataset()
    ar = TS.pack_arena(graphs, U.NMAX, U.ELL_W)
    rec, per = U.restate(graphs)
    assert ar.records.dtype == np.int32 and ar.buf.dtype == np.int32 and ar.feats.dtype == np.float32
    np.testing.assert_array_equal(ar.records, rec)
    assert all(o % 4 == 0 for o in ar.off.values()) and ar.words % 4 == 0            # every section sits on 16 bytes
    assert ar.off["rowptr"] < ar.off["col"] < ar.off["tail_ptr"] < ar.off["tail_col"] < ar.words == ar.buf.size
    assert rec[:, 2].sum() > 0 and rec[0, 2] == rec[:, 2].sum()                     # only graph 0 has a tail
    used = np.zeros(ar.words, dtype=bool)
    for i, (rp, col, tp, tc, f) in enumerate(per):
        n, nnz, nt, row0, ent0, tail0 = rec[i, :6]
        for name, lo, want in (("rowptr", row0 + i, rp), ("col", ent0, col), ("tail_ptr", row0 + i, tp), ("tail_col", tail0, tc)):
            lo += ar.off[name]
            np.testing.assert_array_equal(ar.buf[lo:lo + len(want)], want, err_msg="%s of graph %d" % (name, i))
            used[lo:lo + len(want)] = True
        np.testing.assert_array_equal(ar.feats[row0:row0 + n, :U.FIN], f)
    assert not ar.buf[~used].any()                                                  # padding between the sections: zero
    assert ar.ld == 12 and ar.feats.shape == (sum(U.SIZES), 12) and ar.fin == U.FIN and ar.largest == 48
    # the isolated node: an empty row; the one-node graph: one empty row
    g, v = U.ISOLATED
    rp = per[g][0]
    assert rp[v + 1] == rp[v] and rec[1, 0] == 1 and rec[1, 1] == 0


def test_pad_columns_of_the_feature_table_are_zero():
    TS = _ts()
    graphs = U.dataset()
    for g in graphs:
        g.graph["feats"] = g.graph["feats"][:, :10]
    ar = TS.pack_arena(graphs, U.NMAX)
    assert ar.fin == 10 and ar.ld == 12 and not ar.feats[:, 10:].any() and ar.feats[:, :10].any()


def test_exact_capacities_cover_every_schedule_entry():
    """three times the largest n / nnz / ntail: exact for schedules in which one object may fill several places (U.SCHEDULE has
    [0, 0, 6] and [1, 1, 1]); the sum of the three largest distinct graphs would be overflowed by [0, 0, 6]"""
    TS = _ts()
    ar = TS.pack_arena(U.dataset(), U.NMAX)
    rec = ar.records.astype(np.int64)
    assert ar.caps == tuple(3 * int(rec[:, c].max()) for c in (0, 1, 2)) and ar.caps[0] == 3 * 48
    need = rec[U.SCHEDULE][:, :, :3].sum(axis=1)                     # [T, 3]: rows, entries, tail entries of every schedule entry
    assert (need <= np.array(ar.caps)).all()
    assert need[2, 0] > int(np.sort(rec[:, 0])[-3:].sum())          # ... and the distinct-graph bound is not enough for [0, 0, 6]
    assert TS.pack_arena(U.dataset(), U.NMAX, batch=2).caps[0] == 2 * 48


@pytest.mark.parametrize("what", ["n_zero", "n_over", "weight", "asym", "width", "offsets"])
def test_pack_arena_refuses_and_names_the_graph(what):
    TS = _ts()
    graphs = [copy.deepcopy(g) for g in U.dataset()]
    bad, kw = 4, {}
    d = graphs[bad].graph
    if what == "n_zero":
        d["num_nodes"] = 0
    elif what == "n_over":
        d["num_nodes"] = U.NMAX + 1
    elif what == "weight":
        i, j = np.argwhere(d["adj"] > 0)[0]
        d["adj"][i, j] = d["adj"][j, i] = 0.5
    elif what == "asym":
        i, j = np.argwhere(d["adj"] > 0)[0]
        d["adj"][i, j] = 0.0
    elif what == "width":
        d["feats"] = d["feats"][:, :8]
    else:
        kw, bad = {"limit": 1000}, None
    with pytest.raises(ValueError, match=("graph %d" % bad) if bad is not None else "offsets"):
        TS.pack_arena(graphs, U.NMAX, **kw)


def test_load_refuses_bad_schedules_on_the_host():
    TS = _ts()
    s = TS.TripletStream.__new__(TS.TripletStream)             # (load validates before it touches the device)
    s.arena, s.B = TS.pack_arena(U.dataset(), U.NMAX), 3
    for bad in (np.zeros((4, 2), dtype=np.int64), np.zeros(6, dtype=np.int64), np.zeros((0, 3), dtype=np.int64),
                np.array([[0, 1, -1]]), np.array([[0, 1, 7]]), np.array([[0.0, 1.0, 2.0]])):
        with pytest.raises(ValueError):
            s.load(bad)
    out = TS.check_schedule(U.SCHEDULE, 7)
    assert out.dtype == np.int32 and out.flags["C_CONTIGUOUS"] and np.array_equal(out, U.SCHEDULE)


def test_schedule_of_drains_a_sampler_by_object_identity():
    TS = _ts()
    graphs = U.dataset()

    class Sampler:
        def __init__(self, rows):
            self.rows, self.i, self.shuffled = rows, 99, 0

        def shuffle(self):
            self.i, self.shuffled = 0, self.shuffled + 1

        def end(self):
            return self.i >= len(self.rows)

        def sampler(self):
            a, p, n = self.rows[self.i]
            self.i += 1
            return {"anchor": graphs[a], "pos": graphs[p], "neg": graphs[n], "label": 0}

    sm = Sampler(U.SCHEDULE.tolist())
    got = TS.schedule_of(sm, graphs)
    assert sm.shuffled == 1 and got.shape == (5, 3) and np.array_equal(got, U.SCHEDULE)
    # an equal copy is not the object
    with pytest.raises(ValueError, match="not in"):
        TS.schedule_of(sm, graphs[:3] + [copy.deepcopy(graphs[3])] + graphs[4:])
    from two_stage_gnn_amd import triplet
    assert triplet.TripletStream is TS.TripletStream and triplet.schedule_of is TS.schedule_of and triplet.pack_arena is TS.pack_arena


def test_capacity_batch_takes_a_graph_that_fills_every_slot():
    """``CapacityBatch.collate``'s ghost-slot check: a graph of n nodes needs min(nmax, n + 1) ghost slots (what the fused stack runs
    on, sage_stack._Fwd) — a graph with n == nmax has no ghost slot to need, so a slot whose bound is nmax takes it; a bound below
    what the largest graph needs is still refused"""
    import torch
    from two_stage_gnn_amd import ingest
    from two_stage_gnn_amd.tu_data import TUDataset
    nmax = 8
    sizes = np.array([8, 3])
    gp = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    rows = [[(r + 1) % 8, (r - 1) % 8] for r in range(8)] + [[9], [8, 10], [9]]           # a ring of 8, a path of 3
    rowptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
    col = np.concatenate([np.sort(r) for r in rows]).astype(np.int64)
    ds = TUDataset(gp, rowptr, col, np.zeros(2, dtype=np.int64), np.zeros(11, dtype=np.int64), None, 4)
    cpu = torch.device("cpu")
    slot = ingest.CapacityBatch(2, nmax, 32, 64, 4, cpu, ghost_slots=nmax)
    slot.collate(ds, np.array([0, 1]))                                                     # n == nmax: accepted
    assert (slot.rows, slot.edges, slot.largest) == (11, 20, 8)
    small = ingest.CapacityBatch(1, nmax, 32, 64, 4, cpu, ghost_slots=3)
    with pytest.raises(ValueError, match="ghost-slot bound"):
        small.collate(ds, np.array([1]))                                                   # 3 nodes need 4 ghost slots
    with pytest.raises(ValueError, match="ghost-slot bound"):
        ingest.CapacityBatch(1, nmax, 32, 64, 4, cpu, ghost_slots=7).collate(ds, np.array([0]))
    tight = ingest.CapacityBatch(1, nmax, 32, 64, 4, cpu, ghost_slots=4)
    tight.collate(ds, np.array([1]))
    assert tight.largest == 3
