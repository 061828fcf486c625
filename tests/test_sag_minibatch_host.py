"""The host half of the SAGPool mini-batch stream (two_stage_gnn_amd/sag_stream.py: ``MiniBatchStream``'s helpers; the validator of
tsgnn_sag_batch_gather_f32), no GPU: the arena with labels, the capacity helpers against a brute-force loop over the k chain, every
refusal of ``check_fit``, the numpy restatement of the launch against ``sag_triplet.pack_host``'s collation, the entry point's statuses
without a launch, and the cap on what the GPU tests may leave out of a comparison (no graph has an ambiguous pooling cut)."""
import numpy as np
import pytest
import torch

import sag_minibatch_util as M
import sag_stream_util as U0

EINVAL, EUNSUPPORTED = -1, -3
P = 1 << 20                      # (pointers are only tested for NULL and alignment here)


def _ss():
    from two_stage_gnn_amd import sag_stream
    return sag_stream


def _arena(name, B):
    fin, nhid, C, graphs, labels = M.dataset(name)
    return _ss().pack_arena(M.datas(name, "cpu"), batch=B, n_classes=C), graphs, labels


@pytest.mark.parametrize("name,B", [("small12", 5), ("dd3", 2), ("fin1", 128)])
def test_pack_arena_gives_caps_and_labels_for_any_batch(name, B):
    S = _ss()
    ar, graphs, labels = _arena(name, B)
    rec, per = U0.restate(graphs)
    assert np.array_equal(ar.records, rec) and ar.batch == B
    assert ar.caps == (B * max(M.SIZES[name]), B * int(rec[:, 1].max())) and ar.largest == max(M.SIZES[name])
    assert ar.labels.dtype == np.int32 and ar.labels.tolist() == labels.tolist()
    assert ar.ld == (ar.fin + 3) // 4 * 4 and (name != "fin1" or ar.ld == 4)
    # labels given beside the objects win over data.y; without n_classes the arena carries none (the triplet stream's arena)
    other = [0] * len(graphs)
    assert S.pack_arena(M.datas(name, "cpu"), batch=B, n_classes=2, labels=other).labels.tolist() == other
    assert S.pack_arena(M.datas(name, "cpu"), batch=B).labels is None
    with pytest.raises(ValueError, match="graph 0: label .* outside"):
        S.pack_arena(M.datas(name, "cpu"), batch=B, n_classes=1)
    assert np.array_equal(S.size_records(M.datas(name, "cpu")), rec[:, :2])


@pytest.mark.parametrize("ratio", [0.5, 0.8, 1.0, 0.3])
def test_level_sums_and_default_caps_equal_a_brute_force_loop(ratio):
    """ratio 0.8 with n a multiple of 5 and ratio 1.0 are the float32 rounding corners: float32(0.8) n must not round above the
    integer 4 n / 5, and k(n) = n at ratio 1"""
    S = _ss()
    rng = np.random.default_rng(5)
    n = np.concatenate([np.arange(1, 70), 5 * np.arange(1, 200), rng.integers(1, 1025, 100)])
    rec = np.zeros((n.size, 8), dtype=np.int64)
    rec[:, 0], rec[:, 1] = n, rng.integers(0, 5000, n.size)
    chain = np.array([M.k_chain(int(v), ratio) for v in n])
    assert np.array_equal(S.k_levels(n, ratio, 3), chain)
    assert np.array_equal(chain, np.array([S.k_chain(int(v), ratio, 3) for v in n]))
    if ratio == 0.8:
        assert (chain[n % 5 == 0, 1] == 4 * n[n % 5 == 0] // 5).all()
    if ratio == 1.0:
        assert (chain == n[:, None]).all()
    for B in (1, 3, 8, 128):
        sched = rng.integers(0, n.size, (17, B))
        want = np.array([[sum(chain[i][l] for i in row) for l in range(4)] for row in sched])
        assert np.array_equal(S.level_sums(rec, sched, ratio, 3), want)
        assert np.array_equal(S.nnz_sums(rec, sched), np.array([sum(rec[i, 1] for i in row) for row in sched]))
        caps = S.default_level_caps(rec, B, ratio, 3)
        assert caps == [sum(sorted(chain[:, l], reverse=True)[:B]) for l in range(4)]
        assert S.default_nnz_cap(rec, B) == sum(sorted(rec[:, 1], reverse=True)[:B])
        # every entry of DISTINCT graphs fits the default; the schedule's own capacity is attained and never above it
        distinct = np.array([rng.permutation(n.size)[:B] for _ in range(17)])
        assert (S.level_sums(rec, distinct, ratio, 3) <= np.array(caps)).all()
        sc = S.schedule_capacity(rec, distinct, ratio, 3)
        assert sc["level_caps"] == np.maximum(S.level_sums(rec, distinct, ratio, 3).max(0), chain[np.argmax(n)]).tolist()
        assert sc["row_cap"] == sc["level_caps"][0] and sc["nnz_cap"] == max(S.nnz_sums(rec, distinct).max(), rec[:, 1].max())
        assert all(a <= b for a, b in zip(sc["level_caps"], caps))
        assert S.fits_mask(distinct, rec, B, sc["row_cap"], sc["nnz_cap"], sc["level_caps"], ratio).all()
    # a dataset of fewer graphs than B: the largest stands in for the missing ones
    assert S.default_level_caps(rec[:3], 5, ratio, 3) == [int(chain[:3, l].sum() + 2 * chain[:3, l].max()) for l in range(4)]
    assert S.default_nnz_cap(np.zeros((2, 8), dtype=np.int64), 4) == 1


def test_check_fit_refuses_and_names_the_first_entry():
    S = _ss()
    ar, graphs, labels = _arena("small12", 3)
    rec = ar.records
    caps = S.default_level_caps(rec, 3, 0.5, 3)                      # 64 + 33 + 32 rows
    nnz = S.default_nnz_cap(rec, 3)
    assert caps[0] == 129
    ok = np.array([[10, 9, 8], [0, 1, 2]])
    assert S.check_fit(ok, rec, 3, caps[0], nnz, caps, 0.5).dtype == np.int32
    assert S.fits_mask(ok, rec, 3, caps[0], nnz, caps, 0.5).tolist() == [True, True]
    dup = np.array([[0, 1, 2], [10, 10, 9], [10, 10, 10]])           # duplicates count as often as they appear
    with pytest.raises(ValueError, match=r"schedule entry 1 has \[161, .*eager route"):
        S.check_fit(dup, rec, 3, caps[0], nnz, caps, 0.5)
    assert S.fits_mask(dup, rec, 3, caps[0], nnz, caps, 0.5).tolist() == [True, False, False]
    with pytest.raises(ValueError, match="schedule entry 0 .*eager route"):                  # the CSR entries alone
        S.check_fit(ok, rec, 3, caps[0], int(rec[[10, 9, 8], 1].sum()) - 1, caps, 0.5)
    assert nnz >= int(rec[[10, 9, 8], 1].sum())
    for l in range(4):                                                                      # every level alone
        low = list(caps)
        low[l] -= 1
        with pytest.raises(ValueError, match="schedule entry 0 .*eager route"):
            S.check_fit(ok, rec, 3, max(caps[0], 129), nnz, low, 0.5)
        assert S.fits_mask(ok, rec, 3, 129, nnz, low, 0.5).tolist() == [False, True]
    with pytest.raises(ValueError, match="schedule entry 0 .*eager route"):                  # row_cap below level_caps[0]
        S.check_fit(ok, rec, 3, 128, nnz, caps, 0.5)
    for bad, what in ((np.array([[0, 1]]), "shape"), (np.array([[0, 1, 12]]), "indices"), (np.array([[0.0, 1.0, 2.0]]), "integer"),
                      (np.zeros((0, 3), dtype=np.int64), "shape")):
        with pytest.raises(ValueError, match=what):
            S.check_fit(bad, rec, 3, caps[0], nnz, caps, 0.5)
        with pytest.raises(ValueError, match=what):
            S.fits_mask(bad, rec, 3, caps[0], nnz, caps, 0.5)


def test_capacity_plan_takes_level_caps_and_keeps_the_triplet_layout():
    S = _ss()
    for batch in (3, 1):
        cap = S.CapacityPlan(31, 0.5, 3, batch=batch)
        assert cap.ldg == 4 and [L.N for L in cap.levels] == [batch * k for k in (31, 16, 8, 4)]
    cap = S.CapacityPlan(31, 0.5, 3, batch=7, level_caps=[100, 52, 27, 15])
    assert cap.ldg == 8 and cap.capacity and [L.N for L in cap.levels] == [100, 52, 27, 15]
    assert [L.max_seg for L in cap.levels] == [31, 16, 8, 4] and all(L.B == 7 for L in cap.levels)
    assert S.CapacityPlan(5, 0.5, 3, batch=128).ldg == 132 and S.CapacityPlan(5, 0.5, 3, batch=4).ldg == 8
    with pytest.raises(ValueError, match="level_caps"):
        S.CapacityPlan(31, 0.5, 3, batch=7, level_caps=[100, 52, 27])
    with pytest.raises(ValueError, match="level_caps"):
        S.CapacityPlan(31, 0.5, 3, batch=7, level_caps=[100, 15, 27, 15])


@pytest.mark.parametrize("name,B", [("small12", 3), ("small12", 4), ("small12", 33), ("dd3", 2), ("fin1", 5)])
def test_numpy_restatement_of_the_launch_equals_pack_hosts_collation(name, B):
    """the restatement reads the ARENA's restated rows; ``pack_host`` reads the edge lists: rows, columns, features, sizes, and the
    graph pointers against ``SagPlan``'s host values"""
    from two_stage_gnn_amd.sag_stack import SagPlan
    S = _ss()
    ar, graphs, labels = _arena(name, B)
    rec, per = U0.restate(graphs)
    sched = M.schedule(name, B)
    assert sched.shape[1] == B and int(sched.max()) < len(graphs)
    for ratio in (0.5, 0.8):
        caps = S.schedule_capacity(rec, sched, ratio, 3)
        ldg = (B + 1 + 3) // 4 * 4
        for ids in sched:
            got = M.launch_np(rec, per, labels, ids, ratio, 3, caps["row_cap"], caps["nnz_cap"], caps["level_caps"], ldg, ar.ld)
            rowptr, col, batch, sizes, x = M.collate_np(graphs, ids)
            n, nnz = int(sizes.sum()), int(col.size)
            assert np.array_equal(got["rowptr"][:n + 1], rowptr) and (got["rowptr"][n:] == nnz).all()
            assert np.array_equal(got["col"][:nnz], col) and (got["col"][nnz:] == -1).all()
            assert np.array_equal(got["x"][:n, :ar.fin], x) and not got["x"][n:].any() and not got["x"][:, ar.fin:].any()
            assert (got["dinv"][:n] > 0).all() and not got["dinv"][n:].any() and not got["self_w"][n:].any()
            plan = SagPlan(sizes, ratio, "cpu", 3)
            for l in range(4):
                pre = np.concatenate([[0], np.cumsum(plan.levels[l].sizes)])
                assert got["gp"][l, :B + 1].tolist() == pre.tolist() and (got["gp"][l, B:] == pre[-1]).all()
            assert got["label"].tolist() == [labels[i] for i in ids] and got["ids"].tolist() == ids.tolist()
    # the schedule covers what it promises
    tot = np.array(M.SIZES[name])[sched].sum(1)
    assert tot[0] == tot.max() and tot[1] <= tot[0]
    if name == "small12":
        assert any(set(r.tolist()) == {0} for r in sched) and any(rec[r, 1].sum() == 0 and len(set(r.tolist())) > 1 for r in sched)


def test_batch_gather_refuses_on_the_host():
    """every status tsgnn_sag_batch_gather_f32 returns without a launch"""
    from two_stage_gnn_amd import _native as nat
    fn = nat.lib().tsgnn_sag_batch_gather_f32

    def call(records=P, n_graphs=12, arena=P, off_rowptr=0, off_col=256, words=1024, feats=P, ldf=8, labels=P, max_n=64, max_nnz=320,
             sched=P, sched_cap=5, state=P, ticket=P, B=5, row_cap=173, nnz_cap=900, caps=(173, 87, 44, 22), ratio=0.5, depth=3, rowptr=P,
             col=P, x=P, ldx=8, dinv=P, self_w=P, gp=P, ldg=8, ids=P, label_out=P):
        lc = np.asarray(caps, dtype=np.int64) if caps is not None else None
        return fn(records, n_graphs, arena, off_rowptr, off_col, words, feats, ldf, labels, max_n, max_nnz, sched, sched_cap, state, ticket,
                  B, row_cap, nnz_cap, lc.ctypes.data if lc is not None else None, ratio, depth, rowptr, col, x, ldx, dinv, self_w, gp, ldg,
                  ids, label_out, None)
    ptrs = ("records", "arena", "feats", "labels", "sched", "state", "ticket", "caps", "rowptr", "col", "x", "dinv", "self_w", "gp", "ids",
            "label_out")
    for k in ptrs:
        assert call(**{k: None}) == EINVAL, k
    for kw in (dict(B=0), dict(B=129, ldg=132), dict(depth=0), dict(depth=8), dict(ratio=0.0), dict(ratio=1.5), dict(ratio=float("nan")),
               dict(sched_cap=0), dict(n_graphs=0), dict(max_n=0), dict(ldf=0, ldx=0),
               dict(row_cap=63, caps=(63, 87, 44, 22)),                           # a capacity below the largest graph: rows,
               dict(nnz_cap=319), dict(nnz_cap=0, max_nnz=0),                      # CSR entries (at least 1),
               dict(caps=(173, 31, 44, 22)), dict(caps=(173, 87, 15, 22)), dict(caps=(173, 87, 44, 7)),      # every level: 64, 32, 16, 8
               dict(caps=(172, 87, 44, 22)),                                       # level_caps[0] is row_cap
               dict(ldg=4), dict(ldg=7), dict(ldg=6),                              # ldg < B + 1, ldg % 4
               dict(off_col=-4), dict(off_rowptr=-4), dict(words=128)):
        assert call(**kw) == EINVAL, kw
    for kw in (dict(ldf=6, ldx=6), dict(ldx=12), dict(off_col=258), dict(off_rowptr=2),
               dict(records=P + 4), dict(arena=P + 8), dict(feats=P + 4), dict(rowptr=P + 4), dict(x=P + 4), dict(dinv=P + 8),
               dict(self_w=P + 4), dict(gp=P + 4), dict(state=P + 8), dict(label_out=P + 4),
               dict(row_cap=1 << 31, caps=(1 << 31, 87, 44, 22)), dict(nnz_cap=1 << 31), dict(sched_cap=(1 << 31) // 5 + 1),
               dict(max_n=(1 << 31) // 5 + 1, row_cap=1 << 30, caps=(1 << 30, 1 << 30, 1 << 30, 1 << 30)),
               dict(max_nnz=(1 << 31) // 5 + 1, nnz_cap=(1 << 31) - 1)):
        assert call(**kw) == EUNSUPPORTED, kw


@pytest.mark.parametrize("name", ["small12", "dd3", "many40"])
def test_no_graph_is_ambiguous(name):
    """the cap on exclusions: no graph of a dataset the step tests run has an ambiguous pooling cut in the fp64 oracle, so no schedule
    entry may be left out of a comparison"""
    fin, nhid, C, graphs, labels = M.dataset(name)
    p64 = M._params(M.net(name, dev="cpu"), torch.float64)
    assert [i for i, (x, ei) in enumerate(graphs) if M._ambiguous(p64, x, ei, "gcn")] == []
    assert int(labels.max()) < C and len(set(labels.tolist())) >= 2
