"""Host side of the mini-batch stream (two_stage_gnn_amd/minibatch_stream.py, csrc/batch_stream.hip), no GPU: the arena of a
CSR-resident dataset against the graph-object route, ``epoch_schedule``, the capacity checks of ``load`` / ``fits``, and the entry
point's validator, which refuses before any launch."""
import numpy as np
import pytest

import minibatch_stream_util as U


def _arenas(onehot=False, nmax=U.NMAX):
    from two_stage_gnn_amd import minibatch_stream as MS
    from two_stage_gnn_amd.triplet_stream import pack_arena
    graphs = U.dataset(nmax=nmax, onehot=onehot)
    ds = U.tu_dataset(graphs)
    return graphs, ds, pack_arena(graphs, nmax, U.ELL_W, batch=5), MS


@pytest.mark.parametrize("nmax", [48, 64])
def test_pack_arena_tu_equals_pack_arena_array_for_array(nmax):
    graphs, ds, ref, MS = _arenas(nmax=nmax)
    ar = MS.pack_arena_tu(ds, nmax, U.ELL_W, batch=5, table=U.feature_table(graphs))
    assert ar.off == ref.off and ar.words == ref.words and ar.caps == ref.caps
    for k in ("fin", "ld", "nmax", "ell_w", "batch", "largest", "n_graphs", "total_nodes"):
        assert getattr(ar, k) == getattr(ref, k), k
    for k in ("records", "buf", "feats"):
        a, b = getattr(ar, k), getattr(ref, k)
        assert a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b), k
    assert ar.labels.dtype == np.int32 and ar.labels.tolist() == [g.graph["label"] for g in graphs]
    assert ar.node_label.dtype == np.int32 and np.array_equal(ar.node_label, ds.node_label)
    assert ar.records[U.TAIL, 2] > 0 and (np.delete(ar.records[:, 2], U.TAIL) == 0).all()


def test_pack_arena_tu_node_label_mode_and_default_table():
    graphs, ds, ref, MS = _arenas(onehot=True)
    ar = MS.pack_arena_tu(ds, U.NMAX, U.ELL_W, batch=5, features="node-label")
    assert ar.feats is None and ar.fin == U.FIN and ar.ld == U.LD
    assert np.array_equal(ar.records, ref.records) and np.array_equal(ar.buf, ref.buf)
    tab = MS.pack_arena_tu(ds, U.NMAX, U.ELL_W, batch=5)                      # no table given: the one-hot node labels
    assert np.array_equal(tab.feats, ref.feats)
    # the graph-object route carries labels and node labels too, and the arena goes back to the dataset it came from
    obj = MS._pack_graph_objects(graphs, U.NMAX, U.ELL_W, 5, "node-label")
    assert obj.feats is None and obj.fin == U.FIN and np.array_equal(obj.node_label, ar.node_label) and np.array_equal(obj.labels, ar.labels)
    back = MS.arena_dataset(ar)
    for k in ("graph_ptr", "rowptr", "col", "graph_label", "node_label"):
        assert np.array_equal(getattr(back, k), getattr(ds, k)), k


def test_pack_arena_tu_refuses_what_the_stack_cannot_take():
    graphs, ds, ref, MS = _arenas()
    from two_stage_gnn_amd.tu_data import TUDataset
    with pytest.raises(ValueError, match="graph 0: num_nodes = 48"):
        MS.pack_arena_tu(ds, 47)
    col = ds.col.copy()
    col[0] = int(ds.graph_ptr[1])                                           # graph 0's first column now points into graph 1
    with pytest.raises(ValueError, match="graph 0: a column lies outside"):
        MS.pack_arena_tu(TUDataset(ds.graph_ptr, ds.rowptr, col, ds.graph_label, ds.node_label, None, U.FIN), U.NMAX)
    col = ds.col.copy()
    r0 = ds.col[ds.rowptr[0]:ds.rowptr[1]]
    col[0] = next(j for j in range(48) if j not in r0 and j != 0)           # (0, j) without (j, 0)
    with pytest.raises(ValueError, match="graph 0: the adjacency is not symmetric"):
        MS.pack_arena_tu(TUDataset(ds.graph_ptr, ds.rowptr, col, ds.graph_label, ds.node_label, None, U.FIN), U.NMAX)
    with pytest.raises(ValueError, match="without node labels"):
        MS.pack_arena_tu(TUDataset(ds.graph_ptr, ds.rowptr, ds.col, ds.graph_label, None, None, 0), U.NMAX, features="node-label")
    with pytest.raises(ValueError, match="node label lies outside"):
        MS.pack_arena_tu(TUDataset(ds.graph_ptr, ds.rowptr, ds.col, ds.graph_label, ds.node_label, None, U.FIN - 1), U.NMAX,
                         features="node-label")


@pytest.mark.parametrize("n,batch", [(24, 8), (24, 5), (7, 7), (5, 8), (1, 1)])
def test_epoch_schedule_is_one_permutation_cut_into_batches(n, batch):
    from two_stage_gnn_amd.minibatch_stream import epoch_schedule
    full, rest = epoch_schedule(n, batch, np.random.default_rng(3))
    assert full.shape == (n // batch, batch) and rest.shape == (n % batch,) and full.dtype == rest.dtype == np.int64
    assert sorted(np.concatenate([full.reshape(-1), rest]).tolist()) == list(range(n))
    again, _ = epoch_schedule(n, batch, np.random.default_rng(3))
    other, _ = epoch_schedule(n, batch, np.random.default_rng(4))
    assert np.array_equal(full, again) and (n < 8 or not np.array_equal(full, other))


def test_default_capacity_is_the_sum_of_the_largest():
    graphs, ds, ref, MS = _arenas()
    s = sorted(U.SIZES, reverse=True)
    for B in (1, 3, 24):
        assert MS.default_capacity(ref.records, B) == (sum(s[:B]), int(ref.records[U.TAIL, 2]))
    assert MS.default_capacity(ref.records, 30)[0] == sum(s) + 6 * 48        # fewer graphs than places: the largest stands in
    assert MS.default_capacity(ref.records, 3)[0] < 3 * 48


def test_load_and_fits_refuse_on_the_host():
    graphs, ds, ref, MS = _arenas()
    rec = ref.records
    B = 3
    sched, row_cap, tail_cap = U.plan(B, graphs)
    U.check_plan(B, sched, row_cap, graphs)
    ntail = int(rec[U.TAIL, 2])
    assert tail_cap >= ntail > tail_cap - 4
    # exactly at capacity (entry 0), duplicate ids (entry 2): accepted
    assert MS.fits_mask(sched, rec, B, row_cap, ntail).all()
    out = MS.check_fit(sched, rec, B, row_cap, ntail)
    assert out.dtype == np.int32 and out.flags["C_CONTIGUOUS"] and np.array_equal(out, sched)
    # one row over row_cap; one tail word over tail_cap
    want = U.SIZES[0] + U.SIZES[9] + U.SIZES[4] - 1
    m = MS.fits_mask(sched, rec, B, want, ntail)
    assert m.tolist() == [False, True, True, True, False]
    with pytest.raises(ValueError, match=r"entry 0 has %d rows.*eager route" % (want + 1)):
        MS.check_fit(sched, rec, B, want, ntail)
    m = MS.fits_mask(sched, rec, B, row_cap, ntail - 1)
    assert m.tolist() == [True, True, True, False, True]
    with pytest.raises(ValueError, match=r"entry 3 has .* %d tail entries.*eager route" % ntail):
        MS.check_fit(sched, rec, B, row_cap, ntail - 1)
    twice = np.array([[U.TAIL, U.TAIL, U.ONE_NODE]])                        # duplicates count as often as they appear
    assert MS.fits_mask(twice, rec, B, row_cap, 2 * ntail).all() and not MS.fits_mask(twice, rec, B, row_cap, 2 * ntail - 1).any()
    for fn in (MS.fits_mask, MS.check_fit):
        with pytest.raises(ValueError, match="shape"):
            fn(sched[:, :2], rec, B, row_cap, tail_cap)
        with pytest.raises(ValueError, match="shape"):
            fn(sched[0], rec, B, row_cap, tail_cap)
        with pytest.raises(ValueError, match="shape"):
            fn(sched[:0], rec, B, row_cap, tail_cap)
        with pytest.raises(ValueError, match="integer"):
            fn(sched.astype(np.float32), rec, B, row_cap, tail_cap)
        bad = sched.copy()
        bad[1, 1] = len(rec)
        with pytest.raises(ValueError, match="must lie in"):
            fn(bad, rec, B, row_cap, tail_cap)
        bad[1, 1] = -1
        with pytest.raises(ValueError, match="must lie in"):
            fn(bad, rec, B, row_cap, tail_cap)


def test_every_plan_fits_its_exact_capacity_and_the_default_holds_distinct_graphs():
    """the schedules of the gather test against the stream's own host checks: every entry fits the plan's exact capacities, the
    first one fills the rows to the last, and one row or one tail word less refuses exactly the entries at the bound"""
    graphs, ds, ref, MS = _arenas()
    rec = ref.records
    sizes, tails = np.asarray(U.SIZES), U.tail_counts(graphs)
    assert np.array_equal(rec[:, 0], sizes) and np.array_equal(rec[:, 2], tails)
    for B in U.BATCHES:
        sched, row_cap, tail_cap = U.plan(B, graphs)
        U.check_plan(B, sched, row_cap, graphs)
        assert tail_cap % 4 == 0 and row_cap <= 1500
        rows, tl = MS.entry_sums(rec, sched)
        assert np.array_equal(rows, sizes[sched].sum(1)) and np.array_equal(tl, tails[sched].sum(1))
        assert MS.fits_mask(sched, rec, B, row_cap, tail_cap).all() and np.array_equal(MS.check_fit(sched, rec, B, row_cap, tail_cap), sched)
        assert MS.fits_mask(sched, rec, B, row_cap - 1, tail_cap).tolist() == (rows < row_cap).tolist() and rows[0] == row_cap
        assert MS.fits_mask(sched, rec, B, row_cap, int(tl.max()) - 1).tolist() == (tl < tl.max()).tolist()
        if B <= len(sizes):                                       # entry 0 is the B largest graphs: the default capacity, to the row
            assert MS.default_capacity(rec, B)[0] == row_cap
        for ids in sched:
            out = U.restate_launch(graphs, ids.tolist(), U.NMAX, row_cap)
            assert out["graph_ptr"][B] == sizes[ids].sum() and out["slot_count"][0] == B and out["tail_col"].size <= tail_cap


def test_graph_object_route_takes_the_width_of_the_one_hot_rows():
    graphs, ds, ref, MS = _arenas(onehot=True)
    some = [g for g in graphs if int(np.max(g.graph["node_label"])) < U.FIN - 1]
    assert 0 < len(some) < len(graphs)
    top = max(int(np.max(g.graph["node_label"])) for g in some) + 1
    assert MS._pack_graph_objects(some, U.NMAX, U.ELL_W, 2, "node-label").fin == top < U.FIN
    ar = MS._pack_graph_objects(some, U.NMAX, U.ELL_W, 2, "node-label", fin=U.FIN)
    assert ar.fin == U.FIN and ar.ld == U.LD and ar.feats is None
    assert MS._pack_graph_objects(some, U.NMAX, U.ELL_W, 2, "node-label", fin=top - 1).fin == top      # a label that does not fit


def test_entry_point_refuses_before_any_launch():
    """every refusal of tsgnn_batch_gather_f32 comes back from the host validator: there is no GPU here, so a call that reached the
    launch would fail with another code"""
    from two_stage_gnn_amd import _native as nat
    L = nat.lib()
    P = 1 << 20                                                              # (pointers are only tested for NULL and alignment)
    names = [p[1] for p in nat.parse_header()["tsgnn_batch_gather_f32"][1]]
    good = dict(records=P, n_graphs=24, arena=P, off_rowptr=0, off_col=512, off_tail_ptr=1024, off_tail_col=1536, arena_words=2048,
                feats=P, ldf=12, node_label=None, fin=9, labels=P, max_n=48, max_tail=200, sched=P, sched_cap=5, state=P, ticket=P, B=32,
                nmax=64, row_cap=600, tail_cap=200, ell_w=16, graph_ptr=P, slot_count=P, row_graph=P, row_slot=P, ell=P, tail_ptr=P,
                tail_col=P, ell_slots=P, tail_slots=P, x=P, ldx=12, ids_out=P, label_out=P, stream=None)
    assert list(good) == names

    def rc(**kw):
        return L.tsgnn_batch_gather_f32(*[{**good, **kw}[k] for k in names])
    EINVAL, EUNSUPPORTED = -1, -3
    for k in ("records", "arena", "labels", "sched", "state", "ticket", "graph_ptr", "slot_count", "row_graph", "row_slot", "ell", "tail_ptr",
              "tail_col", "x", "ids_out", "label_out", "ell_slots", "tail_slots"):
        assert rc(**{k: None}) == EINVAL, k
    assert rc(feats=None) == EINVAL and rc(node_label=P) == EINVAL            # a table or the nodes' labels: exactly one
    assert rc(feats=None, node_label=P, fin=0) == EINVAL and rc(feats=None, node_label=P, fin=9, ldx=16) == EINVAL
    assert rc(feats=None, node_label=P, fin=13, ldx=12) == EINVAL
    for kw in (dict(B=0), dict(B=129), dict(sched_cap=0), dict(n_graphs=0), dict(nmax=0), dict(row_cap=0), dict(tail_cap=0), dict(ell_w=12),
               dict(ldf=0), dict(max_n=0), dict(max_tail=-1), dict(row_cap=47), dict(tail_cap=199), dict(max_n=65), dict(off_col=-4),
               dict(off_rowptr=516), dict(arena_words=1535)):
        assert rc(**kw) == EINVAL, kw
    for kw in (dict(records=P + 4), dict(arena=P + 4), dict(feats=P + 4), dict(ell=P + 4), dict(ell_slots=P + 4), dict(x=P + 4),
               dict(state=P + 8), dict(label_out=P + 4), dict(off_col=513), dict(ldx=16), dict(ldf=10, ldx=10),
               dict(row_cap=(1 << 20) - 32), dict(nmax=2049, max_n=48), dict(sched_cap=1 << 26), dict(row_cap=1 << 27, ell_slots=None, tail_slots=None)):
        assert rc(**kw) == EUNSUPPORTED, kw
    # (`good` itself has row_cap 600 < 32 * 48: a capacity below B times the largest graph is not among the refusals; each case above
    # differs from `good` in the named words only)
