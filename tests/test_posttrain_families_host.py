"""Post-training phase for the GAT and DiffPool families, host side (no GPU): ``gat_stream.pack_arena(batch=1)``, every refusal of the
two ``PostTrainStream`` constructors that is decided on a CPU model, ``check_anchors`` behind ``load``, the anchor gather's declaration
and host-side validator, the row-loss entry points' validators, and both fixtures of scripts/gen_golden_posttrain_families.py
against a float64 torch restatement of the reference's loop (tests/posttrain_families_ref.py).

Fixture tolerances are tests/test_posttrain_ref_host.py's for the --method=base fixture: outputs rtol 1e-4 / atol 1e-5, gradients
rtol 1e-3 / atol 1e-4 (the fixture is the reference's own fp32 CPU run).  Final parameters: each of the T Adam steps moves an element
by at most about lr in either run, and an element whose gradient is rounding noise may move the other way, so 2 T lr bounds the
difference (the trajectory rule of tests/test_gpu_posttrain.py)."""
import numpy as np
import pytest
import torch

import gat_stream_util as U
import posttrain_families_ref as FR
import posttrain_ref as PR
import test_gat_triplet_host as H
from conftest import load_golden

OUT_TOL = dict(rtol=1e-4, atol=1e-5)
GRAD_TOL = dict(rtol=1e-3, atol=1e-4)


class A:
    bias = True


# ------------------------------------------------------------------------------------------------ the arena at one piece per entry
@pytest.mark.parametrize("name", ["small3", "big"])
def test_pack_arena_batch_1_capacities(name):
    from two_stage_gnn_amd import gat_stream as S
    objs = U.dataset(name)
    one, three = S.pack_arena(objs, batch=1), S.pack_arena(objs)
    assert one.batch == 1 and three.batch == 3
    assert one.caps == one.top == three.top and three.caps == tuple(3 * t for t in one.top)
    assert np.array_equal(one.records, three.records) and np.array_equal(one.buf, three.buf)
    assert (one.records[:, 2:5] <= np.array(one.caps)).all() and (one.records[:, 2:5].max(0) == np.array(one.caps)).all()
    lone = [H.make_obj(9, 5, fin=8, kind="empty")]                             # 6 rows x 8 floats = 48 words: the limit sees one piece
    assert S.pack_arena(lone, batch=1).caps == (6, 0, 6)
    assert S.pack_arena(lone, limit=81, batch=1).words == 80
    with pytest.raises(ValueError, match="offsets reach 144 .*18 rows x 8"):
        S.pack_arena(lone, limit=144)


# ------------------------------------------------------------------------------------------------ refusals on CPU models
def _labelled(objs, labels):
    out = []
    for o, y in zip(objs, labels):
        out.append(H.GraphObj(o.graph["adj"], o.graph["feats"], o.graph["num_nodes"], label=y))
    return out


def test_gat_constructor_refusals_on_cpu_models():
    from two_stage_gnn_amd import dense_encoders as E, gat_stream, gat_triplet
    objs = _labelled(U.dataset("small8"), [i % 8 for i in range(11)])
    eager = "post_train.post_train_step\\(model, graph\\)$"
    m = U.model("small8", "l2", dev="cpu")
    with pytest.raises(TypeError, match="DGATEncoderGraph.*" + eager):
        gat_stream.PostTrainStream(gat_triplet.tripletnet(m), objs)            # a tripletnet is not the model
    with pytest.raises(TypeError, match="DGATEncoderGraph.*" + eager):
        gat_stream.PostTrainStream(E.GcnEncoderGraph(8, 8, 8, 2, 3, bn=True, args=A(), final_dim="pretrain").cpu(), objs)
    other = U.model("small8", "l2", dev="cpu")
    other.final_dim = "number_classes"
    with pytest.raises(TypeError, match="final_dim = 'output_dim'.*" + eager):
        gat_stream.PostTrainStream(other, objs)
    with pytest.raises(TypeError, match="dropout.*" + eager):
        gat_stream.PostTrainStream(U.model("small8", "l2", dev="cpu", dropouts=[0.0, 0.3]), objs)
    with pytest.raises(ValueError, match="graph 4: label 8 lies outside \\[0, 8\\)"):
        gat_stream.PostTrainStream(m, _labelled(objs, [0, 1, 2, 3, 8, 5, 6, 7, 0, 1, 2]))    # embedding_dim 8: pred has eight columns
    with pytest.raises(ValueError, match="graph 2"):
        gat_stream.PostTrainStream(m, _labelled(objs, [0, 1, -1, 3, 4, 5, 6, 7, 0, 1, 2]))
    with pytest.raises(TypeError, match="GPU only.*" + eager):
        gat_stream.PostTrainStream(m, objs)                                    # everything else passed: the device is what is left
    # the triplet stream's refusals keep their own drop-in
    with pytest.raises(TypeError, match="gat_triplet.tripletnet.*tripletnet.forward\\(a, p, n\\)$"):
        gat_stream.TripletStream(m, objs)
    assert issubclass(gat_stream.PostTrainStream, gat_stream.GatArenaStream) and issubclass(gat_stream.TripletStream, gat_stream.GatArenaStream)
    for name in ("gather", "_allocate", "_views", "load", "position", "mine"):            # shared, not copied
        assert name not in gat_stream.PostTrainStream.__dict__ and name not in gat_stream.TripletStream.__dict__


def test_diffpool_constructor_refusals_on_cpu_models():
    import triplet_stream_util as TU
    from two_stage_gnn_amd import dense_encoders as E, diffpool_stream as D, post_train as PT
    graphs = []
    for gobj, y in zip(TU.dataset(), [0, 1, 1, 0, 1, 0, 0]):
        graphs.append(TU.G(gobj.graph["adj"], gobj.graph["feats"], gobj.graph["num_nodes"]))
        graphs[-1].graph["label"] = y
    eager = "post_train.post_train_step\\(model, graph\\)$"

    def sp(final_dim="pretrain", **kw):
        m = E.SoftPoolingGcnEncoder(TU.NMAX, TU.FIN, 32, 32, 2, 3, 32, assign_ratio=0.25, num_pooling=1, bn=True, args=A(),
                                    assign_input_dim=TU.FIN, final_dim=final_dim).cpu()
        m.map2_model = PT.make_head(32, device=torch.device("cpu"))
        m.bn = kw.get("bn", True)
        return m
    with pytest.raises(TypeError, match="SoftPoolingGcnEncoder.*" + eager):
        D.PostTrainStream(E.GcnEncoderGraph(TU.FIN, 32, 32, 2, 3, bn=True, args=A(), final_dim="pretrain").cpu(), graphs)
    with pytest.raises(TypeError, match="final_dim == \"pretrain\".*" + eager):
        D.PostTrainStream(sp("output_dim"), graphs)
    with pytest.raises(TypeError, match="concat and bn.*" + eager):
        D.PostTrainStream(sp(bn=False), graphs)
    bad = list(graphs)
    bad[3] = TU.G(graphs[3].graph["adj"], graphs[3].graph["feats"], graphs[3].graph["num_nodes"])
    bad[3].graph["label"] = 2
    with pytest.raises(ValueError, match="graph 3: label 2 lies outside \\[0, 2\\)"):
        D.PostTrainStream(sp(), bad)
    with pytest.raises(TypeError, match="GPU only.*" + eager):
        D.PostTrainStream(sp(), graphs)
    assert issubclass(D.PostTrainStream, PT.PostTrainSteps) and issubclass(PT.PostTrainStream, PT.PostTrainSteps)
    assert issubclass(D.PostTrainStream, D.DiffPoolChecks) and issubclass(D.TripletStream, D.DiffPoolChecks)
    for name in ("step", "step_loss", "_checked", "_stacks_ok", "gather", "load"):          # shared, not copied
        assert name not in D.PostTrainStream.__dict__ and name not in PT.PostTrainStream.__dict__


def test_load_goes_through_check_anchors():
    from two_stage_gnn_amd import diffpool_stream as D, gat_stream as S, post_train as PT
    assert S.PostTrainStream._checked is not S.TripletStream._checked and D.PostTrainStream._checked is PT.PostTrainStream._checked
    st = S.PostTrainStream.__new__(S.PostTrainStream)                          # (load validates before it touches the device)
    st.arena, st.B = S.pack_arena(U.dataset("small3"), batch=1), 1
    for good in (np.array([0, 10, 4]), np.array([[3], [2]]), [1, 1]):
        assert st._checked(good).shape == (len(good), 1) and st._checked(good).dtype == np.int32
    for bad in (U.schedule("small3"), np.zeros((4, 2), dtype=np.int64), np.zeros(0, dtype=np.int64), np.array([0, -1]), np.array([11]),
                np.array([0.0, 1.0])):
        with pytest.raises(ValueError):
            st.load(bad)
    st._sched, st.T = None, 0
    with pytest.raises(RuntimeError, match="load"):
        st.mine(None, None, 1.0)
    st._sched, st.T = object(), 1
    with pytest.raises(RuntimeError, match="names 1 graph.*no negative to mine"):      # an entry is one anchor
        st.mine(None, None, 1.0)


# ------------------------------------------------------------------------------------------------ the entry points, on the host
def test_anchor_gather_is_declared_and_validates_on_the_host():
    from two_stage_gnn_amd import _native as nat
    decl = nat.parse_header()
    assert [n for _, n in decl["tsgnn_gat_anchor_gather_f32"][1]] == [n for _, n in decl["tsgnn_gat_triplet_gather_f32"][1]]
    assert [t for t, _ in decl["tsgnn_gat_anchor_gather_f32"][1]] == [t for t, _ in decl["tsgnn_gat_triplet_gather_f32"][1]]
    L = nat.lib()
    P = 1 << 20                                                                # (pointers are only tested here, never followed)
    d = H._desc(K=0, R=12, E=30, I=4, B=1)
    call = lambda d_=d, rec=P, n=4, ar=P, words=100, nr=12, nnz=30, k=4, sched=P, cap=5, state=P, tk=P, ids=P: \
        L.tsgnn_gat_anchor_gather_f32(rec, n, ar, words, nr, nnz, k, sched, cap, state, tk, d_.ctypes.data if d_ is not None else None, ids, None)
    assert call(rec=None) == -1 and call(ar=None) == -1 and call(sched=None) == -1 and call(state=None) == -1 and call(tk=None) == -1
    assert call(ids=None) == -1 and call(d_=None) == -1
    assert call(n=0) == -1 and call(cap=0) == -1 and call(nr=0) == -1 and call(nnz=-1) == -1 and call(k=13) == -1
    assert call(nr=13) == -1 and call(nnz=31) == -1 and call(k=5) == -1        # a capacity below ONE times the largest piece
    assert call(d_=H._desc(K=0, R=12, E=30, I=4, B=3)) == -1                   # a triplet's header
    assert call(d_=H._desc(K=0, R=36, E=90, I=12, B=2)) == -1
    assert call(d_=H._desc(K=0, R=12, E=30, I=4, B=1, ldf=6)) == -1            # rows off 16 bytes
    miss = H._desc(K=0, R=12, E=30, I=4, B=1)
    miss[19] = 0
    assert call(d_=miss) == -1                                                 # a missing output
    assert call(rec=P + 4) == -3 and call(ar=P + 8) == -3 and call(state=P + 8) == -3      # misaligned records / arena / state
    assert call(words=1 << 31) == -3 and call(cap=1 << 31) == -3
    # the triplet entry point still refuses what the anchor one takes, and the reverse
    trip = lambda d_: L.tsgnn_gat_triplet_gather_f32(P, 4, P, 100, 12, 30, 4, P, 5, P, P, d_.ctypes.data, P, None)
    assert trip(d) == -1 and trip(H._desc(K=0, R=35, E=90, I=12, B=3)) == -1


def test_row_loss_entry_points_validate_on_the_host():
    from two_stage_gnn_amd import _native as nat
    L = nat.lib()
    ok = L.tsgnn_posttrain_rowloss_supported
    assert ok(8, 1) == 1 and ok(2, 8) == 1 and ok(1024, 1) == 1
    assert ok(1, 1) == 0 and ok(1025, 1) == 0 and ok(8, 0) == 0 and ok(8, 9) == 0
    P = 1 << 20
    fwd = lambda z=P, ld=8, R=1, C=8, ids=P, lab=P, n=7, p=P, loss=P: L.tsgnn_posttrain_rowloss_fwd_f32(z, ld, R, C, ids, lab, n, p, loss, None)
    bwd = lambda p=P, R=1, C=8, ids=P, lab=P, n=7, dz=P, ld=8: L.tsgnn_posttrain_rowloss_bwd_f32(p, R, C, ids, lab, n, None, dz, ld, None)
    assert fwd(z=None) == -1 and fwd(ids=None) == -1 and fwd(lab=None) == -1 and fwd(p=None) == -1 and fwd(loss=None) == -1
    assert fwd(n=0) == -1 and fwd(R=0) == -1 and fwd(C=1) == -1 and fwd(ld=7) == -1
    assert fwd(C=1025, ld=1025) == -3 and fwd(R=9) == -3
    assert bwd(p=None) == -1 and bwd(dz=None) == -1 and bwd(ids=None) == -1 and bwd(n=0) == -1 and bwd(ld=7) == -1 and bwd(C=1) == -1
    assert bwd(C=1025, ld=1025) == -3 and bwd(R=9) == -3


# ------------------------------------------------------------------------------------------------ the fixtures
@pytest.mark.parametrize("name", ["posttrain_gat", "posttrain_diffpool"])
def test_fixture_against_a_float64_restatement_of_the_loop(name):
    g = load_golden(name)
    dicts = PR.golden_graphs(g)
    T, lr = len(dicts), float(g["lr"])
    sizes = [d["num_nodes"] for d in dicts]
    assert sizes[:6] == [16, 1, 9, 12, 5, 14] and [d["label"] for d in dicts][:6] == [0, 1, 1, 0, 1, 0] and int(g["nmax"]) == 16
    gat = name == "posttrain_gat"
    if gat:
        assert T == 7 and not dicts[6]["adj"].any() and g["heads"].tolist() == [2, 2] and g["dims"].tolist() == [8, 8, 8, 2]
    else:
        assert T == 6 and int(g["num_pooling"]) == 1 and int(g["num_layers"]) == 3
    ref64, _ = FR.reference_runs(name, g)
    for s in range(T):
        np.testing.assert_allclose(ref64["s%d.loss" % s].numpy(), g["s%d.loss" % s].reshape(1), err_msg="loss %d" % s, **OUT_TOL)
    # (outputs and gradients from EQUAL parameters: step 0)
    np.testing.assert_allclose(ref64["s0.pred"].numpy(), g["s0.pred"], err_msg="pred", **OUT_TOL)
    np.testing.assert_allclose(ref64["s0.out"].numpy(), g["s0.out"], err_msg="out", **OUT_TOL)
    assert g["s0.pred"].shape == ((1, 8) if gat else (1, 2)) and g["s0.out"].shape == ((1, 2) if gat else (1, 8))
    stored = {k[5:] for k in g if k.startswith("s0.g.")}
    assert stored == {k[5:] for k in ref64 if k.startswith("s0.g.")}                          # None is absent in both
    names = set(FR.initial(g))
    frozen = {k for k in names if k.startswith(("map_model", "map2_model", "pred_model", "pre_pred_model"))} if gat else \
        {k for k in names if k.startswith(("pred_model", "pre_pred_model"))}
    assert names - stored == frozen and (len(stored) == 8 if gat else len(stored) == 28)
    seen = 0
    for k in sorted(stored):
        np.testing.assert_allclose(ref64["s0.g." + k].numpy(), g["s0.g." + k], err_msg=k, **GRAD_TOL)
        seen += bool(np.abs(g["s0.g." + k]).max() > 1e-3)
    assert seen >= (8 if gat else 20)                                                          # neither soft-max saturates
    worst = 0.0
    for k in names:
        diff = float(np.abs(ref64["final." + k].numpy() - g["final." + k]).max())
        worst = max(worst, diff)
        if k in frozen:
            assert np.array_equal(g["final." + k], g["p." + k]), k                             # no gradient: Adam skipped it
    print("%s: max parameter difference after %d steps %.3e (bound %.3e)" % (name, T, worst, 2 * T * lr))
    assert worst <= 2 * T * lr
    assert max(float(np.abs(g["final." + k] - g["p." + k]).max()) for k in stored) > 3e-3      # (the steps moved them)
    # evaluate(): the stored metrics are those of the stored predictions
    from two_stage_gnn_amd import two_stage as TS
    y, pred = np.array([d["label"] for d in dicts]), g["eval.pred"]
    got = TS.metrics_from_confusion(TS.confusion_matrix(y, pred, np.unique(np.concatenate([y, pred]))))
    for k in ("prec", "recall", "acc", "F1"):
        assert got[k] == pytest.approx(float(g["eval." + k]), abs=1e-12), k
    final64 = {k: torch.as_tensor(g["final." + k]).double() for k in names}                   # the reference's own final parameters
    step = FR.gat_step if gat else FR.diffpool_step
    with torch.no_grad():
        z = torch.cat([step(final64, d)[1] for d in dicts])
    top2 = z.topk(2, dim=1).values
    gap = float((top2[:, 0] - top2[:, 1]).min())
    print("%s: smallest gap between the two largest columns of pred %.3e" % (name, gap))
    assert gap > 1e-4 and z.argmax(dim=1).tolist() == pred.tolist()                            # (no near tie: the argmax is not rounding)
