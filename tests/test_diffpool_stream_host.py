"""Host side of the DiffPool triplet stream (two_stage_gnn_amd/diffpool_stream.py), no GPU: the ``assign_feats`` refusal names the
graph, a schedule is validated before anything touches the device, the model refusals that need no device, and the streams that
share ``ArenaStream`` word their refusals as before."""
import copy

import numpy as np
import pytest

import triplet_stream_util as U


class _A:
    bias = True


def _ds():
    from two_stage_gnn_amd import diffpool_stream as DS
    return DS


def _model(**kw):
    from two_stage_gnn_amd import dense_encoders as E
    args = dict(assign_ratio=0.25, num_pooling=1, bn=True, linkpred=False, args=_A(), assign_input_dim=U.FIN, final_dim="output_dim")
    args.update(kw)
    return E.SoftPoolingGcnEncoder(U.NMAX, U.FIN, 32, 32, 2, 3, 32, **args).cpu()


def _net(m):
    from two_stage_gnn_amd import triplet
    return triplet.tripletnet(m)


def test_assign_feats_that_differ_are_refused_by_graph_index():
    DS = _ds()
    graphs = [copy.deepcopy(g) for g in U.dataset()]
    DS.check_assign_feats(graphs)                                  # the same array, or an equal one: accepted
    graphs[2].graph["assign_feats"] = graphs[2].graph["feats"].copy()
    DS.check_assign_feats(graphs)
    pad = graphs[3].graph["feats"].copy()
    pad[U.SIZES[3]:] = 7.0                                         # rows beyond num_nodes are nobody's features
    graphs[3].graph["assign_feats"] = pad
    DS.check_assign_feats(graphs)
    bad = graphs[4].graph["feats"].copy()
    bad[U.SIZES[4] - 1, 0] += 1.0
    graphs[4].graph["assign_feats"] = bad
    with pytest.raises(ValueError, match="graph 4"):
        DS.check_assign_feats(graphs)
    with pytest.raises(ValueError, match="graph 4"):               # ... by the constructor, before it asks for a device
        DS.TripletStream(_net(_model()), graphs)
    graphs[4].graph["assign_feats"] = graphs[4].graph["feats"][:, :8]
    with pytest.raises(ValueError, match="graph 4"):
        DS.check_assign_feats(graphs)


def test_schedules_are_validated_on_the_host():
    DS = _ds()
    from two_stage_gnn_amd import triplet_stream as TS
    assert DS.check_schedule is TS.check_schedule and issubclass(DS.TripletStream, TS.ArenaStream)
    s = DS.TripletStream.__new__(DS.TripletStream)                 # (load validates before it touches the device)
    s.arena, s.B = TS.pack_arena(U.dataset(), U.NMAX), 3
    for bad in (np.zeros((4, 2), dtype=np.int64), np.zeros(6, dtype=np.int64), np.zeros((0, 3), dtype=np.int64),
                np.array([[0, 1, -1]]), np.array([[0, 1, 7]]), np.array([[0.0, 1.0, 2.0]])):
        with pytest.raises(ValueError):
            s.load(bad)
    out = DS.check_schedule(U.SCHEDULE, 7)
    assert out.dtype == np.int32 and np.array_equal(out, U.SCHEDULE)


@pytest.mark.parametrize("what", ["bn", "concat", "num_pooling", "final_dim", "family", "no model"])
def test_model_refusals_that_need_no_device(what):
    DS = _ds()
    graphs = U.dataset()
    if what == "bn":
        m = _model()
        m.bn = False                                               # (the constructor does not forward bn: encoders.py:249-250)
    elif what == "concat":
        m = _model(concat=False)
    elif what == "num_pooling":
        m = _model(num_pooling=0)
    elif what == "final_dim":
        m = _model(final_dim="pretrain")
    elif what == "family":
        from two_stage_gnn_amd import dense_encoders as E
        m = E.GcnEncoderGraph(U.FIN, 32, 32, 2, 3, bn=True, args=_A(), final_dim="output_dim").cpu()
    else:
        m = None
    net = _net(m) if m is not None else object()
    with pytest.raises(TypeError, match="SoftPoolingGcnEncoder.*eager drop-in, tripletnet.forward"):
        DS.TripletStream(net, graphs)


def test_an_accepted_model_on_the_cpu_is_sent_to_the_eager_drop_in():
    with pytest.raises(TypeError, match="runs on the GPU only; use the eager drop-in"):
        _ds().TripletStream(_net(_model()), U.dataset())


def test_the_other_streams_word_their_refusals_as_before():
    """``ArenaStream``'s model check became overridable; ``triplet.TripletStream`` and ``PostTrainStream`` keep theirs"""
    from two_stage_gnn_amd import dense_encoders as E, post_train, triplet
    graphs = U.dataset()
    sp = _model()
    with pytest.raises(TypeError, match=r"^TripletStream takes a tripletnet over a GcnEncoderGraph with concat and bn; use the eager drop-in, "
                                        r"tripletnet.forward\(a, p, n\)$"):
        triplet.TripletStream(_net(sp), graphs)
    nobn = E.GcnEncoderGraph(U.FIN, 32, 32, 2, 3, bn=False, args=_A(), final_dim="output_dim").cpu()
    with pytest.raises(TypeError, match="^TripletStream takes a tripletnet over a GcnEncoderGraph with concat and bn; use the eager"):
        triplet.TripletStream(_net(nobn), graphs)
    with pytest.raises(TypeError, match="^PostTrainStream "):
        post_train.PostTrainStream(sp, graphs)
