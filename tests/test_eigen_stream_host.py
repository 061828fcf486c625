"""eigen_stream without a GPU: ``pack_arena`` against the concatenated piece buffers and ``pack_host``'s numbers, the capacities against
every schedule entry, every refusal of ``pack_arena`` and ``check_schedule``, the entry points' declarations and the gather's
host-side validator, and a numpy restatement of the gather launch whose real prefix is ``eigen_two_stage_util.assemble_numpy`` of the
three pieces."""

import numpy as np
import pytest

import eigen_stream_util as U
import eigen_two_stage_util as EU


def _arena(data, name):
    from two_stage_gnn_amd import eigen_stream as S
    ps, J, Jf = U.shape(data, name)
    return S.pack_arena(U.dataset(data, name), len(ps), J, Jf), len(ps), J, Jf


@pytest.mark.parametrize("data,name", U.GATHER_CASES)
def test_arena_is_the_concatenated_piece_buffers(data, name):
    from two_stage_gnn_amd import eigen_stream as S, eigen_triplet as ET
    ar, L, J, Jf = _arena(data, name)
    objs = U.dataset(data, name)
    pcs = U.pieces_of(objs, L, J, Jf)
    assert ar.records.dtype == np.int32 and ar.records.shape == (len(objs), S.REC_WORDS) and S.REC_WORDS * 4 % 16 == 0
    assert ar.buf.dtype == np.int32 and ar.words == ar.buf.size == sum(p[0].size for p in pcs)
    assert np.array_equal(ar.buf, np.concatenate([p[0] for p in pcs]))
    assert (ar.records[:, 0] % 4 == 0).all()                                  # every piece starts on 16 bytes
    words = 0
    for i, (buf, n, z) in enumerate(pcs):
        pad = [0] * (S.LMAX - len(n))
        assert ar.records[i].tolist() == [words, i] + n + pad + z + pad + [0, 0]
        off = ET.piece_layout(n, z, J, Jf, ar.ldf)                             # sections at the layout's offsets, each on 16 bytes
        assert int(off[-1]) == buf.size and (off % 4 == 0).all()
        p = ET.pack_host(objs[i].graph, L, J, Jf)
        u = ET.unpack_piece(ar.buf[words:words + buf.size], n, z, J, Jf, ar.ldf)
        for (rp, col, val), c in zip(u["graphs"], p["graphs"]):                # piece-local indices
            assert np.array_equal(rp, c[0]) and np.array_equal(col, c[1]) and np.array_equal(val, c[2]) and rp[0] == 0
        words += buf.size
    assert (ar.n_graphs, ar.fin, ar.ldf, ar.L, ar.J, ar.Jf) == (len(objs), U.FIN[data], 8, L, J, Jf)
    nlev = L + 1
    assert ar.top == (tuple(ar.records[:, 2:2 + nlev].max(0).tolist()), tuple(ar.records[:, 6:6 + nlev].max(0).tolist()))
    assert ar.caps == tuple(tuple(3 * t for t in part) for part in ar.top)
    if data == "big":
        assert ar.nmax == 320 and ar.top[0][0] * ar.ldf > 2048                 # the feature section spans several copy chunks
    else:
        assert ar.nmax == EU.NMAX == ar.top[0][0]                              # a full graph: no ghost slot of its own
        assert all(ar.records[g, 3] == 1 and ar.records[g, 7] == 0 for g in U.ONE_CLUSTER)      # one pooled node, no entry


@pytest.mark.parametrize("data,name", U.GATHER_CASES)
def test_capacities_bound_every_schedule_entry(data, name):
    """three times the largest n_i / nnz_i, not the three largest distinct graphs: the entry that names one object three times fits"""
    from two_stage_gnn_amd import eigen_stream as S
    ar, L, J, Jf = _arena(data, name)
    nlev = L + 1
    sched = U.schedule(data)
    assert S.check_schedule(sched, ar.n_graphs).dtype == np.int32
    assert set(sched.reshape(-1).tolist()) == set(range(ar.n_graphs))
    need_n = ar.records[:, 2:2 + nlev][sched].sum(1)
    need_z = ar.records[:, 6:6 + nlev][sched].sum(1)
    assert (need_n <= np.array(ar.caps[0])).all() and (need_z <= np.array(ar.caps[1])).all()
    assert need_n[0].tolist() == list(ar.caps[0]) and len(set(sched[0].tolist())) == 1     # the first entry fills every row capacity
    assert need_n[1, 0] < need_n[0, 0]                                         # the second is smaller: stale rows would show
    assert any(e[0] == e[1] != e[2] for e in sched)                            # anchor = positive
    if data == "small":
        assert (need_z[:, 1] == 0).any() and any(U.UNASSIGNED in e for e in sched.tolist())     # a level with E = 0


def test_pack_arena_refusals():
    from two_stage_gnn_amd import eigen_stream as S, eigen_triplet as ET
    ps, J, Jf = EU.CONFIGS["l2_j1"]
    L = len(ps)
    good = U.dataset("small", "l2_j1")[:3]
    assert S.pack_arena(good, L, J, Jf).n_graphs == 3
    with pytest.raises(ValueError, match="no graphs"):
        S.pack_arena([], L, J, Jf)

    def changed(i, **kw):
        objs = list(good)
        d = dict(good[i].graph)
        for k, v in kw.items():
            if v is None:
                del d[k]
            else:
                d[k] = v
        objs[i] = EU.GraphObj(d)
        return objs
    with pytest.raises(ValueError, match="graph 1: the graph dict has no 'pool_adj_1_0'"):          # check_dict
        S.pack_arena(changed(1, pool_adj_1_0=None), L, J, Jf)
    with pytest.raises(ValueError, match="graph 2: the graph dict has 'pool_adj_0_1'"):
        S.pack_arena(changed(2, pool_adj_0_1=good[2].graph["pool_adj_0_0"]), L, J, Jf)
    with pytest.raises(ValueError, match="graph 0: the graph dict has 'adj_pool_3'"):            # prepared for another L
        S.pack_arena(changed(0, adj_pool_3=good[0].graph["adj_pool_2"], num_nodes_3=1), L, J, Jf)
    P = np.array(good[1].graph["pool_adj_0_0"], copy=True)
    P[0, int(good[1].graph["num_nodes_1"])] = 0.5                                                   # pack_host
    with pytest.raises(ValueError, match="graph 1: pool_adj_0_.*column >= the pooled node count"):
        S.pack_arena(changed(1, pool_adj_0_0=P), L, J, Jf)
    with pytest.raises(ValueError, match="graph 2: feats must be"):
        S.pack_arena(changed(2, feats=np.zeros((3, 6), dtype=np.float32)), L, J, Jf)
    other = U.dataset("big", "big")[0]
    with pytest.raises(ValueError, match="graph 1: the graph dict has no"):                       # another (L, J, Jf)
        S.pack_arena([good[0], U.dataset("small", "l1_j1")[1]], L, J, Jf)
    wide = EU.GraphObj(EU.make_dict(EU.make_result(np.random.default_rng(1), 9, ps), np.random.default_rng(2), 23, J, Jf, 6))
    with pytest.raises(ValueError, match="graph 2: Nmax = 23 differs from the other graphs' 19"):
        S.pack_arena(good[:2] + [wide], L, J, Jf)
    f5 = EU.GraphObj(EU.make_dict(EU.make_result(np.random.default_rng(1), 9, ps), np.random.default_rng(2), EU.NMAX, J, Jf, 5))
    with pytest.raises(ValueError, match="graph 1: feature width 5 differs from the other graphs' 6"):
        S.pack_arena([good[0], f5], L, J, Jf)
    assert other.graph["adj"].shape[0] == 320
    # a level adjacency that is not symmetric: level 0 (a directed edge) and a pooled level
    directed = EU.GraphObj(EU.make_dict(EU.make_result(np.random.default_rng(3), 12, ps, odd=True), np.random.default_rng(4), EU.NMAX, J, Jf, 6))
    with pytest.raises(ValueError, match="graph 1, level 0: the adjacency is not symmetric.*no transposed CSR.*host sizes"):
        S.pack_arena([good[0], directed], L, J, Jf)
    A1 = np.array(good[0].graph["adj_pool_1"], copy=True)
    r, c = np.argwhere(np.triu(A1, 1) > 0)[0]
    A1[r, c] += 1.0
    with pytest.raises(ValueError, match="graph 0, level 1: the adjacency is not symmetric"):
        S.pack_arena(changed(0, adj_pool_1=A1), L, J, Jf)
    # more levels than the assembler takes
    dps, dJ, dJf = EU.DEEP["l4_j1_f1"]
    assert len(dps) > ET.max_levels()
    with pytest.raises(ValueError, match="4 pooling levels, the assembler takes up to 3"):
        S.pack_arena(good, len(dps), dJ, dJf)
    # offsets that reach the limit: the arena's words, then the batch's feature rows
    words = S.pack_arena(good, L, J, Jf).words
    with pytest.raises(ValueError, match="graph 2: .*offsets reach"):
        S.pack_arena(good, L, J, Jf, limit=words)
    assert S.pack_arena(good, L, J, Jf, limit=words + 1).words == words
    lone = good[2:3]
    a = S.pack_arena(lone, L, J, Jf)
    rows = (a.caps[0][0] + a.nmax) * a.ldf
    assert rows > a.words
    with pytest.raises(ValueError, match="offsets reach %d .*%d \\+ 19 rows x 8" % (rows, a.caps[0][0])):
        S.pack_arena(lone, L, J, Jf, limit=rows)
    assert S.pack_arena(lone, L, J, Jf, limit=rows + 1).words == a.words


def test_check_schedule_refusals():
    from two_stage_gnn_amd import eigen_stream as S, triplet_stream as TS
    assert S.check_schedule is TS.check_schedule and S.schedule_of is TS.schedule_of and S.HEAD == TS.HEAD
    assert issubclass(S.TripletStream, TS.ArenaStream)
    for name in ("load", "position", "_warm_up_schedule", "_checked", "__len__"):      # reused, not copied
        assert name not in S.TripletStream.__dict__
    for bad, what in ((np.zeros((4, 2), dtype=np.int64), "shape"), (np.zeros((0, 3), dtype=np.int64), "shape"),
                      (np.zeros(3, dtype=np.int64), "shape"), (np.zeros((2, 3)), "integer"),
                      (np.array([[0, 1, -1]]), "indices"), (np.array([[0, 1, 4]]), "indices")):
        with pytest.raises(ValueError, match=what):
            S.check_schedule(bad, 4)


def _desc(Rc, Ec, nmax=19, J=2, Jf=1, ldf=8, B=3, K=3, P=1 << 20):
    """a header of tsgnn_eigen_assemble_f32's description with every output present (pointers are only tested, never followed)"""
    from two_stage_gnn_amd import _native as nat
    nlev = len(Rc)
    d = np.zeros(int(nat.lib().tsgnn_eigen_assemble_header_words()), dtype=np.int64)
    d[0:8] = (K, B, nlev, J, Jf, ldf, nmax, 1)
    d[9], d[10] = P, P if Jf else 0
    for i in range(nlev):
        d[12 + 2 * i], d[13 + 2 * i] = Rc[i], Ec[i]
        d[20 + 7 * i:27 + 7 * i] = P
    for i in range(nlev - 1):
        d[48 + 4 * i:52 + 4 * i] = P
    return d


def test_entry_points_are_declared_and_the_gather_validates_on_the_host():
    from two_stage_gnn_amd import _native as nat
    decl = nat.parse_header()
    assert [n for _, n in decl["tsgnn_eigen_triplet_gather_f32"][1]] == ["records", "n_graphs", "arena", "arena_words", "top_n", "top_nnz",
                                                                        "sched", "sched_cap", "state", "ticket", "desc", "ids_out", "stream"]
    assert [n for _, n in decl["tsgnn_eigen_pool_fwd_cap_f32"][1]] == [n for _, n in decl["tsgnn_eigen_pool_fwd_f32"][1]]
    L = nat.lib()
    P = 1 << 20
    good = _desc((57, 12), (228, 36))
    tn, tz = np.array([19, 4], dtype=np.int64), np.array([76, 12], dtype=np.int64)

    def call(d_=good, rec=P, n=4, ar=P, words=100, tn_=tn, tz_=tz, sched=P, cap=5, state=P, tk=P, ids=P):
        p = lambda a: a.ctypes.data if a is not None else None
        return L.tsgnn_eigen_triplet_gather_f32(rec, n, ar, words, p(tn_), p(tz_), sched, cap, state, tk, p(d_), ids, None)
    EINVAL, EUNSUPPORTED = -1, -3
    for kw in (dict(rec=None), dict(ar=None), dict(sched=None), dict(state=None), dict(tk=None), dict(ids=None), dict(d_=None),
               dict(tn_=None), dict(tz_=None), dict(n=0), dict(cap=0), dict(words=0)):
        assert call(**kw) == EINVAL, kw
    # a capacity below three times the caller's top, per level, rows and entries
    for tn2, tz2 in (([20, 4], [76, 12]), ([19, 5], [76, 12]), ([19, 4], [77, 12]), ([19, 4], [76, 13]), ([0, 4], [76, 12]),
                     ([19, 4], [-1, 12])):
        assert call(tn_=np.array(tn2, dtype=np.int64), tz_=np.array(tz2, dtype=np.int64)) == EINVAL, (tn2, tz2)
    # a description ea_unpack's rules reject
    assert call(d_=_desc((57, 12), (228, 36), B=2, K=2)) == EINVAL             # not a triplet
    assert call(d_=_desc((57, 12), (228, 36), ldf=6)) == EINVAL                # rows off 16 bytes
    assert call(d_=_desc((57, 12), (228, 36), J=6)) == EINVAL and call(d_=_desc((57, 12), (228, 36), Jf=5)) == EINVAL
    assert call(d_=_desc((57, 12, 3, 3, 3), (228, 36, 0, 0, 0))) == EINVAL     # more level graphs than the assembler takes
    for word in (9, 10, 20, 26, 27, 33, 48, 51):                               # a missing output, a misaligned one
        miss = good.copy()
        miss[word] = 0
        assert call(d_=miss) == EINVAL, word
        miss[word] = P + 4
        assert call(d_=miss) == EINVAL, word
    neg = good.copy()
    neg[12] = -1
    assert call(d_=neg) == EINVAL
    # unaligned records / arena / state, offsets >= 2^31, a grid of 65,536 chunks or more
    assert call(rec=P + 4) == EUNSUPPORTED and call(ar=P + 8) == EUNSUPPORTED and call(state=P + 8) == EUNSUPPORTED
    assert call(words=1 << 31) == EUNSUPPORTED and call(cap=(1 << 31) // 3) == EUNSUPPORTED
    big = _desc((3 * 1000, 300), (3 * 9000, 900), nmax=1000, ldf=1 << 20)
    assert call(d_=big, tn_=np.array([1000, 100], dtype=np.int64), tz_=np.array([9000, 300], dtype=np.int64)) == EUNSUPPORTED
    wide = _desc((3 * 100000, 300), (3 * 100000000, 900), nmax=100000, ldf=8)                # 2 x 48,829 chunks of col and val alone
    assert call(d_=wide, tn_=np.array([100000, 100], dtype=np.int64), tz_=np.array([100000000, 300], dtype=np.int64)) == EUNSUPPORTED


@pytest.mark.parametrize("data,name", U.GATHER_CASES)
def test_numpy_gather_has_the_assembled_triplet_as_its_prefix(data, name):
    """the restatement of the launch (eigen_stream_util.gather_numpy, which the GPU test holds the kernel to): for every schedule
    entry the [:R_i] / [:E_i] prefixes are ``assemble_numpy`` of the three pieces word for word, the closing entries agree, and what
    lies behind is the padding of csrc/eigen_stream.hip's header comment"""
    ar, L, J, Jf = _arena(data, name)
    pcs = U.pieces_of(U.dataset(data, name), L, J, Jf)
    Rc, Ec = ar.caps
    bits = lambda a: np.ascontiguousarray(a).view(np.int32)
    for ids in U.schedule(data):
        got, R, E = U.gather_numpy(ar, ids)
        want = EU.assemble_numpy([pcs[i] for i in ids], ar.nmax, J, Jf, ar.ldf)
        for i in range(L + 1):
            assert np.array_equal(got["rowptr_%d" % i][:R[i] + 1], want["rowptr_%d" % i][:R[i] + 1])
            assert (got["rowptr_%d" % i][R[i]:] == E[i]).all() and got["rowptr_%d" % i].size == Rc[i] + ar.nmax + 1
            for k in ("col_%d", "val_%d"):
                assert np.array_equal(bits(got[k % i][:E[i]]), bits(want[k % i][:E[i]]))
            assert (got["col_%d" % i][E[i]:] == U.IPAT).all() and np.isnan(got["val_%d" % i][E[i]:]).all()       # unwritten
            assert np.array_equal(got["graph_ptr_%d" % i], want["graph_ptr_%d" % i]) and got["graph_ptr_%d" % i][3] == R[i]
            assert np.array_equal(got["slot_count_%d" % i], want["slot_count_%d" % i])
            for k, pad in (("row_graph_%d", 2), ("row_slot_%d", 0)):
                assert np.array_equal(got[k % i][:R[i]], want[k % i]) and (got[k % i][R[i]:] == pad).all()
        for i in range(L):
            assert np.array_equal(got["cluster_of_%d" % i][:R[i]], want["cluster_of_%d" % i]) and (got["cluster_of_%d" % i][R[i]:] == -1).all()
            assert np.array_equal(bits(got["coef_%d" % i][:R[i]]), bits(want["coef_%d" % i])) and not bits(got["coef_%d" % i][R[i]:]).any()
            nb = R[i + 1] + 4
            assert np.array_equal(got["bptr_%d" % i][:nb], want["bptr_%d" % i]) and (got["bptr_%d" % i][nb - 1:] == R[i]).all()
            assert np.array_equal(got["members_%d" % i][:R[i]], want["members_%d" % i]) and (got["members_%d" % i][R[i]:] == U.IPAT).all()
        if Jf:
            assert np.array_equal(bits(got["final"][:R[L]]), bits(want["final"])) and not bits(got["final"][R[L]:]).any()
        assert np.array_equal(bits(got["x"][:R[0]]), bits(want["x"][:R[0]])) and not bits(got["x"][R[0]:]).any()
