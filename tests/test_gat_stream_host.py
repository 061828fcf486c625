"""gat_stream without a GPU: ``pack_arena`` against the concatenated piece buffers and ``pack_host``'s numbers, the capacities against
every schedule entry, every refusal of ``pack_arena`` and ``check_schedule``, the entry point's declaration and its host-side
validator."""
import numpy as np
import pytest

import gat_stream_util as U
import test_gat_triplet_host as H


@pytest.mark.parametrize("name", ["small3", "small8", "big"])
def test_arena_is_the_concatenated_piece_buffers(name):
    from two_stage_gnn_amd import gat_stream as S, gat_triplet as GT
    objs = U.dataset(name)
    ar = S.pack_arena(objs)
    rec, bufs = U.restate(objs)
    assert ar.records.dtype == np.int32 and ar.records.shape == (len(objs), S.REC_WORDS) and np.array_equal(ar.records, rec)
    assert ar.buf.dtype == np.int32 and ar.words == ar.buf.size == sum(b.size for b in bufs)
    assert np.array_equal(ar.buf, np.concatenate(bufs))
    assert np.array_equal(ar.buf, np.concatenate([GT.piece_buffer(GT.pack_host(o)) for o in objs]))
    assert (ar.records[:, 0] % 4 == 0).all()                                  # every piece starts on 16 bytes
    assert ar.n_graphs == len(objs) and ar.fin == U.FIN[name] and ar.ldf == (U.FIN[name] + 3) // 4 * 4
    for i, o in enumerate(objs):
        p = GT.pack_host(o)
        assert ar.records[i].tolist() == [ar.records[i, 0], p["n"], p["nr"], p["nnz"], p["k"], p["mult"], i, 0]
    if name == "big":                                                          # a piece spans several copy chunks, off 16 bytes
        assert ar.top[1] > 2 * 2048 and ar.top[0] * ar.ldf > 2048 and ar.nmax == 320
        assert any(int(r[3]) % 4 for r in ar.records) and any(int(r[2]) % 4 for r in ar.records)
    else:
        assert ar.nmax == 12 and sorted(set(ar.records[:, 1].tolist())) == sorted(set(n for n, _ in U.ASM_GRAPHS))
        assert 0 in ar.records[:, 3].tolist()                                  # the edge-less graph


@pytest.mark.parametrize("name", ["small3", "big"])
def test_capacities_bound_every_schedule_entry(name):
    """three times the largest nr / nnz / k, not the three largest distinct graphs: the entry that names one object three times fits"""
    from two_stage_gnn_amd import gat_stream as S
    ar = S.pack_arena(U.dataset(name))
    sched = U.schedule(name)
    assert S.check_schedule(sched, ar.n_graphs).dtype == np.int32
    assert 8 <= len(sched) <= 12 and set(sched.reshape(-1).tolist()) == set(range(ar.n_graphs))
    assert any(len(set(e.tolist())) == 1 for e in sched)
    top = int(np.argmax(ar.records[:, 2] * (1 << 20) + ar.records[:, 3]))      # the largest graph: most rows, then most entries
    assert all((sched[:, j] == top).any() for j in range(3))
    need = ar.records[:, 2:5][sched].sum(1)                                    # [T, 3]: rows, entries, listed columns per entry
    assert (need <= np.array(ar.caps)).all() and ar.caps == tuple(3 * t for t in ar.top)
    assert (np.diff(need[:2, 0]) < 0).all()                                    # the second entry is smaller: stale rows would show
    distinct = np.sort(ar.records[:, 2])[-3:].sum()
    if name == "big":
        assert need[:, 0].max() == ar.caps[0] > distinct                       # [3, 3, 3] fills the capacity the distinct sum misses
    else:
        assert (need[:, 1] == 0).any()                                         # a triplet without any edge


def test_pack_arena_refusals():
    from two_stage_gnn_amd import gat_stream as S
    good = [H.make_obj(i, n) for i, n in enumerate((5, 8, 3))]
    assert S.pack_arena(good).n_graphs == 3
    with pytest.raises(ValueError, match="no graphs"):
        S.pack_arena([])
    rows = H.make_obj(4, 5)
    rows.graph["feats"][7, 1] = 0.5                                            # padded feature rows that differ
    with pytest.raises(ValueError, match="graph 1: one representative"):
        S.pack_arena([good[0], rows])
    edge = H.make_obj(4, 5)
    edge.graph["adj"][6, 2] = 1.0                                              # adj positive outside [:n, :n]
    with pytest.raises(ValueError, match="graph 2: one representative"):
        S.pack_arena(good[:2] + [edge])
    with pytest.raises(ValueError, match="graph 1: Nmax = 9 differs"):
        S.pack_arena([good[0], H.make_obj(7, 5, nmax=9)])
    with pytest.raises(ValueError, match="graph 2: feature width 5 differs"):
        S.pack_arena(good[:2] + [H.make_obj(7, 5, fin=5)])
    with pytest.raises(ValueError, match="graph 0: adj must be"):
        S.pack_arena([H.GraphObj(np.zeros((8, 9)), np.zeros((8, 3), dtype=np.float32), 3)])
    words = S.pack_arena(good).words
    with pytest.raises(ValueError, match="graph 2: .*offsets reach"):
        S.pack_arena(good, limit=words)
    assert S.pack_arena(good, limit=words + 1).words == words
    lone = [H.make_obj(9, 5, fin=8, kind="empty")]                             # 80 words; a batch of 3 x 6 rows x 8 floats
    assert S.pack_arena(lone).words == 80 and S.pack_arena(lone).caps == (18, 0, 18)
    with pytest.raises(ValueError, match="offsets reach 144 .*18 rows x 8"):
        S.pack_arena(lone, limit=144)                                          # the batch's feature rows reach it, the arena does not
    assert S.pack_arena(lone, limit=145).words == 80


def test_check_schedule_refusals():
    from two_stage_gnn_amd import gat_stream as S, triplet_stream as TS
    assert S.check_schedule is TS.check_schedule and S.schedule_of is TS.schedule_of and S.HEAD == TS.HEAD
    assert issubclass(S.TripletStream, TS.ArenaStream)
    for name in ("load", "position", "_warm_up_schedule", "_checked", "__len__"):      # reused, not copied
        assert name not in S.TripletStream.__dict__
    for bad, what in ((np.zeros((4, 2), dtype=np.int64), "shape"), (np.zeros((0, 3), dtype=np.int64), "shape"),
                      (np.zeros(3, dtype=np.int64), "shape"), (np.zeros((2, 3)), "integer"),
                      (np.array([[0, 1, -1]]), "indices"), (np.array([[0, 1, 4]]), "indices")):
        with pytest.raises(ValueError, match=what):
            S.check_schedule(bad, 4)


def test_schedule_of_reads_a_sampler():
    from two_stage_gnn_amd import gat_stream as S
    objs = U.dataset("small3")

    class Sampler:
        def __init__(self, rows):
            self.rows, self.i = rows, 0

        def shuffle(self):
            self.i = 0

        def end(self):
            return self.i >= len(self.rows)

        def sampler(self):
            a, p, n = (objs[j] for j in self.rows[self.i])
            self.i += 1
            return {"anchor": a, "pos": p, "neg": n}
    assert S.schedule_of(Sampler(U.schedule("small3").tolist()), objs).tolist() == U.schedule("small3").tolist()


def test_entry_point_is_declared_and_validates_on_the_host():
    from two_stage_gnn_amd import _native as nat
    decl = nat.parse_header()
    assert "tsgnn_gat_triplet_gather_f32" in decl
    assert [n for _, n in decl["tsgnn_gat_triplet_gather_f32"][1]] == ["records", "n_graphs", "arena", "arena_words", "max_nr", "max_nnz", "max_k",
                                                                      "sched", "sched_cap", "state", "ticket", "desc", "ids_out", "stream"]
    L = nat.lib()
    P = 1 << 20                                                                # (pointers are only tested here, never followed)
    d = H._desc(K=0, R=36, E=90, I=12, B=3)
    call = lambda d_=d, rec=P, n=4, ar=P, words=100, nr=12, nnz=30, k=4, sched=P, cap=5, state=P, tk=P, ids=P: \
        L.tsgnn_gat_triplet_gather_f32(rec, n, ar, words, nr, nnz, k, sched, cap, state, tk, d_.ctypes.data if d_ is not None else None, ids, None)
    assert call(rec=None) == -1 and call(ar=None) == -1 and call(sched=None) == -1 and call(state=None) == -1 and call(tk=None) == -1
    assert call(ids=None) == -1 and call(d_=None) == -1
    assert call(n=0) == -1 and call(cap=0) == -1 and call(nr=0) == -1 and call(nnz=-1) == -1 and call(k=13) == -1
    assert call(nr=13) == -1 and call(nnz=31) == -1 and call(k=5) == -1        # a capacity below three times the largest piece
    assert call(d_=H._desc(K=0, R=36, E=90, I=12, B=2)) == -1                  # not a triplet
    assert call(d_=H._desc(K=0, R=36, E=90, I=12, B=3, ldf=6)) == -1           # rows off 16 bytes
    miss = H._desc(K=0, R=36, E=90, I=12, B=3)
    miss[19] = 0
    assert call(d_=miss) == -1                                                 # a missing output
    assert call(rec=P + 4) == -3 and call(ar=P + 8) == -3 and call(state=P + 8) == -3      # off 16 bytes
    assert call(words=1 << 31) == -3 and call(cap=(1 << 31) // 3) == -3
