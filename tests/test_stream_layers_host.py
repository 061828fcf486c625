"""The layers the streams are built from (two_stage_gnn_amd/triplet_stream.py: ``ArenaStream``, ``SageArenaStream``, ``TripletSteps``;
post_train.py: ``AnchorSteps``; minibatch_stream.py: ``MiniBatchSteps``), no GPU: the shared mini-batch code on ``__new__`` stubs of the
three ``MiniBatchStream`` classes (stub records and capacities, ``load`` replaced by a recorder), and where every concrete stream
class gets its protocol from."""
import inspect
import re
import types

import numpy as np
import pytest

B = 3
# four graphs; graph 1 is the smallest in the column the family sorts by, and its B copies exceed ONE capacity (the last
# column below); graph 0 is the second smallest and its copies fit; the copies of graphs 2 and 3 have too many rows
ROWS, OTHER = [5, 4, 9, 7], [4, 20, 8, 6]
ROW_CAP, OTHER_CAP = 16, 15


def _mods():
    from two_stage_gnn_amd import gat_stream, minibatch_stream, sag_stream
    return {"sage": minibatch_stream, "sag": sag_stream, "gat": gat_stream}


def _stub(family, row_cap=ROW_CAP, other_cap=OTHER_CAP, max_steps=2):
    """-> (stream built with ``__new__``, the entries its ``load`` was given, the words that name its capacities)"""
    from two_stage_gnn_amd import triplet_stream as TS
    cls = _mods()[family].MiniBatchStream
    st = cls.__new__(cls)
    rec = np.zeros((4, 8), dtype=np.int32)
    if family == "sage":                                          # n, nnz, ntail, ...: rows and tail entries
        rec[:, 0], rec[:, 2] = ROWS, OTHER
        st.row_cap, st.tail_cap = row_cap, other_cap
        words = "row_cap %d / tail_cap %d" % (row_cap, other_cap)
    elif family == "sag":                                         # n, nnz, ...: the rows of every level (ratio 0.5: 5, 3, 2, 1) and CSR entries
        rec[:, 0], rec[:, 1] = ROWS, OTHER
        st.level_caps = np.array([row_cap, 9, 6, 3], dtype=np.int64)
        st.row_cap, st.nnz_cap, st.plan = row_cap, other_cap, types.SimpleNamespace(ratio=0.5)
        words = "the capacities (level_caps %s, nnz_cap %d)" % ([row_cap, 9, 6, 3], other_cap)
    else:                                                         # offset, n, nr, nnz, k, ...: rows, entries, listed columns
        rec[:, 2], rec[:, 3] = ROWS, OTHER
        st.row_cap, st.nnz_cap, st.iso_cap = row_cap, other_cap, 0
        words = "the capacities (row_cap %d, nnz_cap %d, iso_cap 0)" % (row_cap, other_cap)
    st.arena, st.B, st.max_steps = TS.Arena(records=rec, n_graphs=4), B, max_steps
    loaded = []
    st.load = lambda schedule: loaded.append(np.asarray(schedule))
    return st, loaded, words


FAMILIES = ["sage", "sag", "gat"]


@pytest.mark.parametrize("family", FAMILIES)
def test_the_warm_up_entry_is_the_smallest_graph_whose_copies_fit(family):
    st, loaded, _ = _stub(family)
    assert st.fits(np.arange(4).reshape(-1, 1).repeat(B, axis=1)).tolist() == [True, False, False, False]
    st._warm_up_schedule()
    assert len(loaded) == 1 and loaded[0].shape == (1, B) and loaded[0].tolist() == [[0] * B]
    # without max_steps there is no warm-up entry: the caller builds the step after the first load
    st, loaded, _ = _stub(family, max_steps=None)
    st._warm_up_schedule()
    assert loaded == []


@pytest.mark.parametrize("family", FAMILIES)
def test_the_warm_up_refusals_keep_their_text(family):
    st, loaded, words = _stub(family, row_cap=11, other_cap=11)       # below 3 x 4 rows, and below every graph's other column x 3
    name = "MiniBatchStream" if family == "sage" else "%s_stream.MiniBatchStream" % family
    text = ("%s: max_steps asks for a warm-up entry, and 3 copies of no graph fit %s; leave max_steps out and build the step after the "
            "first load(schedule)" % (name, words))
    with pytest.raises(ValueError, match="^" + re.escape(text) + "$"):
        st._warm_up_schedule()
    st, loaded2, _ = _stub(family, max_steps=0)
    with pytest.raises(ValueError, match="^max_steps must be at least 1$"):
        st._warm_up_schedule()
    assert loaded == [] and loaded2 == []


@pytest.mark.parametrize("family", FAMILIES)
def test_eager_step_refuses_bad_ids_before_it_touches_a_device(family):
    st, _, _ = _stub(family)                                          # (no device, no model, no dataset: a refusal needs none)
    i64 = lambda *v: np.array(v, dtype=np.int64)
    for ids, shape, dtype in ((i64(0, 1).reshape(2, 1), "(2, 1)", "int64"), (i64(), "(0,)", "int64"), (i64(0, 1, 2, 3), "(4,)", "int64"),
                              (np.array([0.0, 1.0]), "(2,)", "float64")):
        text = "eager_loss takes 1 to 3 integer indices; got shape %s of %s" % (shape, dtype)
        for call in (st.eager_step, st.eager_loss):
            with pytest.raises(ValueError, match="^" + re.escape(text) + "$"):
                call(ids)
    for ids in (i64(0, 4), i64(-1), i64(2, -1, 0)):
        with pytest.raises(ValueError, match="^" + re.escape("indices must lie in [0, 4)") + "$"):
            st.eager_step(ids)


@pytest.mark.parametrize("family", FAMILIES)
def test_mine_refuses(family):
    st, _, _ = _stub(family)
    name = "MiniBatchStream" if family == "sage" else "%s_stream.MiniBatchStream" % family
    text = "%s: a schedule entry names a mini-batch, not a triplet: there is no negative to mine" % name
    with pytest.raises(RuntimeError, match="^" + re.escape(text) + "$"):
        st.mine(None, None, 1.0)
    with pytest.raises(RuntimeError, match="^" + re.escape(text) + "$"):
        st.mine()


def _streams():
    from two_stage_gnn_amd import diffpool_stream as D, eigen_stream as E, gat_stream as G, minibatch_stream as M, post_train as P
    from two_stage_gnn_amd import sag_stream as S, triplet_stream as T
    return [T.TripletStream, P.PostTrainStream, M.MiniBatchStream, D.TripletStream, D.PostTrainStream, S.TripletStream,
            S.PostTrainStream, S.MiniBatchStream, G.TripletStream, G.PostTrainStream, G.MiniBatchStream, E.TripletStream, E.PostTrainStream]


def test_every_stream_takes_its_protocol_from_arena_stream():
    from two_stage_gnn_amd import minibatch_stream as M, post_train as P, triplet_stream as T
    A = T.ArenaStream
    streams = _streams()
    assert len(set(streams)) == 13
    for cls in streams:
        what = "%s.%s" % (cls.__module__, cls.__name__)
        assert A in cls.__mro__, what
        assert cls.load is A.load and cls.position is A.position and cls.__len__ is A.__len__ and cls._loaded is A._loaded, what
        assert cls._refuse is A._refuse and cls._init_protocol is A._init_protocol, what
        mini, anchor, triplet = (issubclass(cls, k) for k in (M.MiniBatchSteps, P.AnchorSteps, T.TripletSteps))
        assert mini + anchor + triplet == 1 and mini == (cls.__name__ == "MiniBatchStream") and anchor == (cls.__name__ == "PostTrainStream"), what
        # the documented overrides: a mini-batch stream's mine() refusal and warm-up entry, and the _checked hooks
        assert cls.mine is (M.MiniBatchSteps.mine if mini else A.mine), what
        assert cls._warm_up_schedule is (M.MiniBatchSteps._warm_up_schedule if mini else A._warm_up_schedule), what
        if anchor:
            assert cls._checked is P.AnchorSteps._checked and cls.step_loss is P.AnchorSteps.step_loss, what
        elif mini:
            assert "_checked" in cls.__dict__ and "fits" in cls.__dict__ and cls.loss is M.MiniBatchSteps.loss, what
            assert cls.eager_loss is M.MiniBatchSteps.eager_loss and cls._checked_ids is M.MiniBatchSteps._checked_ids, what
        else:
            assert cls._checked is A._checked and cls.loss is T.TripletSteps.loss, what
        assert "__init__" in cls.__dict__ and not re.search(r"\b_sched\b", inspect.getsource(cls.__init__)), what


def test_only_the_protocol_assigns_the_protocol_state():
    """no family module assigns the schedule state; each shared name is defined in one place"""
    from two_stage_gnn_amd import diffpool_stream as D, eigen_stream as E, gat_stream as G, minibatch_stream as M, post_train as P
    from two_stage_gnn_amd import sag_stream as S, triplet_stream as T
    state = re.compile(r"^\s*(?:self\.\w+\s*[,=]\s*)*self\.(?:_sched|_host|_parts|T|ids_out|_tickets)\s*(?:,\s*self\.\w+\s*)*=[^=]", re.M)
    assert state.search("    self.B, self.T = 1, 2\n") and state.search("  self.a = self._sched = None\n") and not state.search("  x = self.T == 3\n")
    for mod in (D, E, G, M, P, S):
        src = inspect.getsource(mod)
        assert not state.search(src), (mod.__name__, state.search(src).group(0))
    assert state.search(inspect.getsource(T.ArenaStream)) and not state.search(inspect.getsource(T.SageArenaStream))
    for mod in (D, E, G, S):
        src = inspect.getsource(mod)
        for name in ("_refuse", "mine", "_warm_up_schedule", "loss", "step_loss", "eager_loss"):
            assert not re.search(r"^\s*def %s\(" % name, src, re.M), (mod.__name__, name)
        assert not re.search(r"^class Arena\b", src, re.M), mod.__name__
    assert S.Arena is T.Arena and G.Arena is T.Arena and E.Arena is T.Arena and M.Arena is T.Arena
    assert S.MAX_BATCH == G.MAX_BATCH == M.MAX_BATCH == 128
