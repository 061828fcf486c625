"""The post-training phase of 2stg+ on the GPU (two_stage_gnn_amd/post_train.py, csrc/posttrain_head.hip): the eager step against the
reference's own steps (tests/golden/posttrain_gcn.npz), the streamed step against the eager one and the CPU oracle, an epoch from
one hipGraph, no host in the loop, ``two_stage.evaluate_pred`` and the constructor's refusals.

Dataset: the seven graphs of tests/triplet_stream_util.py with labels attached to copies; the anchor schedule runs largest then
smallest, repeats an entry and includes the graph with the isolated node."""
import copy

import numpy as np
import pytest
import torch

import posttrain_ref as PR
import triplet_stream_util as U
from conftest import load_golden, params_of

pytestmark = pytest.mark.gpu

HID = 128
LABELS = [0, 1, 1, 0, 1, 0, 0]
ANCHORS = np.array([0, 1, 4, 1, 1, 6, 3], dtype=np.int64)


class A:
    bias = True


def _dataset(nmax=U.NMAX, labels=LABELS):
    out = []
    for g, y in zip(U.dataset(nmax=nmax), labels):
        c = copy.copy(g)
        c.graph = dict(g.graph, label=y)
        out.append(c)
    return out


def _model(seed=6):
    from two_stage_gnn_amd import dense_encoders as E
    from two_stage_gnn_amd import post_train as PT
    torch.manual_seed(seed)
    m = E.GcnEncoderGraph(U.FIN, HID, HID, 2, 3, bn=True, args=A(), final_dim="pretrain")
    with torch.no_grad():
        for k, p in m.named_parameters():
            if "conv" in k and k.endswith("bias"):
                p.copy_(torch.randn_like(p) * 0.3)           # padded and ghost rows then carry values that can win the max readout
    m = m.cuda()
    PT.install_head(m)
    return m


def _grads_of(m):
    return {k: p.grad.detach().clone() for k, p in m.named_parameters() if p.grad is not None}


def _golden_model(g, prefix="p."):
    from two_stage_gnn_amd import dense_encoders as E
    from two_stage_gnn_amd import post_train as PT
    fin, hid, emb, lab = (int(v) for v in g["dims"])
    m = E.GcnEncoderGraph(fin, hid, emb, lab, int(g["num_layers"]), bn=True, args=A(), final_dim="pretrain").cuda()
    PT.install_head(m)
    m.load_state_dict({k: v.cuda() for k, v in params_of(g, prefix).items()})
    return m


def _golden_objects(g):
    objs = []
    for d in PR.golden_graphs(g):
        objs.append(U.G(d["adj"], d["feats"], d["num_nodes"]))
        objs[-1].graph["label"] = d["label"]
    return objs


def test_eager_step_reproduces_the_reference():
    """step 0 of the fixture from its initial parameters: pred, out, loss and every parameter gradient at the tolerances
    tests/test_gpu_gat_triplet.py holds its golden to (outputs rtol 1e-4 / atol 1e-5, gradients rtol 2e-3 / atol 1e-4); then the
    six steps under FlatTrainer(clip=0): every loss at the same tolerance, the parameters within 2 T lr of the reference's"""
    from two_stage_gnn_amd import _native as nat
    from two_stage_gnn_amd import post_train as PT
    from two_stage_gnn_amd.data_parallel import FlatTrainer
    g = load_golden("posttrain_gcn")
    m, objs = _golden_model(g), _golden_objects(g)
    m.train()
    nat.trace = []
    try:
        loss, pred, out = PT.post_train_step(m, objs[0])
        loss.backward()
        names = [t[0] for t in nat.trace]
    finally:
        nat.trace = None
    assert "posttrain_head_fwd_f32" in names and "posttrain_head_bwd_f32" in names, names
    assert not pred.requires_grad and not out.requires_grad and getattr(m, "_defer_map", False) is False
    np.testing.assert_allclose(pred.cpu().numpy(), g["s0.pred"], rtol=1e-4, atol=1e-5)
    np.testing.assert_allclose(out.cpu().numpy(), g["s0.out"], rtol=1e-4, atol=1e-5)
    np.testing.assert_allclose(float(loss.detach()), float(g["s0.loss"]), rtol=1e-4, atol=1e-5)
    seen = 0
    for k, p in m.named_parameters():
        ref = g["s0.g." + k]
        got = p.grad.cpu().numpy() if p.grad is not None else np.zeros_like(ref)
        print("%s: max|grad| %.3e, max|hip - reference| %.3e" % (k, np.abs(ref).max(), np.abs(got - ref).max()))
        np.testing.assert_allclose(got, ref, rtol=2e-3, atol=1e-4, err_msg=k)
        seen += bool(np.abs(ref).max() > 1e-3)
    assert seen >= 14
    m = _golden_model(g)
    tr = FlatTrainer(m, lr=float(g["lr"]), clip=0)
    for s, obj in enumerate(objs):
        tr.zero_grad()
        loss = PT.post_train_step(m, obj)[0]
        tr.backward(loss)
        tr.gather_grads()
        tr.apply()
        print("step %d: loss %.7f, reference %.7f" % (s, float(loss.detach()), float(g["s%d.loss" % s])))
        np.testing.assert_allclose(float(loss.detach()), float(g["s%d.loss" % s]), rtol=1e-4, atol=1e-5, err_msg="step %d" % s)
    final = params_of(g, "final.")
    diff = max(float((p.detach().cpu() - final[k]).abs().max()) for k, p in m.named_parameters())
    print("max parameter difference after 6 steps: %.3e (bound %.3e)" % (diff, 2 * 6 * float(g["lr"])))
    assert diff <= 2 * 6 * float(g["lr"])


def _oracle_step(p_ref, obj):
    for v in p_ref.values():
        v.grad = None
    loss, pred, out = PR.step(p_ref, obj.graph)
    loss.backward()
    return loss.detach(), pred.detach(), out.detach(), {k: v.grad for k, v in p_ref.items() if v.grad is not None}


@pytest.mark.parametrize("nmax", [48, 64])
def test_streamed_step_equals_the_eager_one_and_the_oracle(nmax):
    """every schedule entry, from the same parameters: loss, logits and ``out`` of the streamed step against ``post_train_step`` on
    the same object at rtol = atol = 1e-5, every parameter gradient at 2e-5 * max|grad| (the bounds tests/test_gpu_triplet_stream.py
    holds the same comparison to), and against the CPU oracle's B = 1 step at that test's oracle bounds (outputs rtol = atol = 1e-4,
    gradients 2e-3 * max|ref| + 1e-6).  Gradients are compared from equal parameters, never after Adam."""
    from two_stage_gnn_amd import _native as nat
    from two_stage_gnn_amd import post_train as PT
    graphs = _dataset(nmax)
    m = _model()
    st = PT.PostTrainStream(m, graphs)
    assert st.B == 1 and st.row_cap == 64 and st.arena.caps[0] == 48 and st.g.ghost_slots_fixed == min(nmax, 49) and st.labels.tolist() == LABELS
    st.load(ANCHORS)
    p_ref = {k: v.detach().cpu().clone().requires_grad_(True) for k, v in m.state_dict().items()}
    for k, i in enumerate(ANCHORS):
        m.zero_grad(set_to_none=True)
        nat.trace = []
        try:
            loss, pred, out = st.step()
            loss.backward()
            names = [t[0] for t in nat.trace]
        finally:
            nat.trace = None
        gs = _grads_of(m)
        assert st.ids_out.tolist() == [int(i)]
        assert all(w in names for w in ("triplet_gather_f32", "posttrain_head_fwd_f32", "posttrain_head_bwd_f32")) and "row_maps" not in names, names
        m.zero_grad(set_to_none=True)
        lossd, predd, outd = PT.post_train_step(m, graphs[i])
        lossd.backward()
        gd = _grads_of(m)
        for a, b in ((loss, lossd), (pred, predd), (out, outd)):
            torch.testing.assert_close(a.detach(), b.detach(), rtol=1e-5, atol=1e-5)
        assert gs.keys() == gd.keys() and len(gs) == 14 and all(("map2_model.%d.%s" % (j, w)) in gs for j in (0, 2, 4) for w in ("weight", "bias"))
        scale = max(float(v.abs().max()) for v in gd.values())
        worst = max(float((gs[n_] - gd[n_]).abs().max()) for n_ in gd)
        print("entry %d (graph %d): loss %.6f, max|grad| %.3e, max|stream - eager| %.3e (bound %.3e)" % (k, i, float(loss.detach()), scale, worst,
                                                                                                       2e-5 * scale))
        for n_ in gd:
            err = float((gs[n_] - gd[n_]).abs().max())
            assert err <= 2e-5 * scale, (k, n_, err, scale)
        lo, po, oo, go = _oracle_step(p_ref, graphs[i])
        torch.testing.assert_close(loss.detach().cpu(), lo, rtol=1e-4, atol=1e-4)
        torch.testing.assert_close(pred.detach().cpu(), po, rtol=1e-4, atol=1e-4)
        torch.testing.assert_close(out.detach().cpu(), oo, rtol=1e-4, atol=1e-4)
        assert set(go) == set(gs)                                  # every gradient of the step is compared, the head's eight included
        for n_, ref in go.items():
            err = float((gs[n_].cpu() - ref).abs().max())
            assert err <= 2e-3 * float(ref.abs().max()) + 1e-6, (k, n_, err, float(ref.abs().max()))
    assert st.position() == len(ANCHORS)


def test_an_epoch_from_one_hipgraph_equals_eager_steps():
    from two_stage_gnn_amd import post_train as PT
    from two_stage_gnn_amd.data_parallel import FlatTrainer, GraphedStep
    graphs = _dataset()
    m1 = _model()
    m2 = copy.deepcopy(m1)
    T, lr = len(ANCHORS), 1e-3
    tr2 = FlatTrainer(m2, lr=lr, clip=0)
    eager = []
    for i in ANCHORS:
        tr2.zero_grad()
        loss = PT.post_train_step(m2, graphs[i])[0]
        tr2.backward(loss)
        tr2.gather_grads()
        tr2.apply()
        eager.append(float(loss.detach()))
    st = PT.PostTrainStream(m1, graphs, max_steps=T)
    assert len(st) == 1 and st.position() == 0                    # the one-entry warm-up schedule
    gs = GraphedStep(FlatTrainer(m1, lr=lr, clip=0), st.step_loss())
    st.load(ANCHORS)                                              # after the warm-up steps: cursor := 0
    streamed = []
    for _ in range(T):
        gs.step()
        streamed.append(gs.loss_value())
    assert st.position() == T
    print("losses streamed %s eager %s" % (streamed, eager))
    np.testing.assert_allclose(streamed, eager, rtol=1e-4)
    diff = max(float((p1.detach() - p2.detach()).abs().max()) for p1, p2 in zip(m1.parameters(), m2.parameters()))
    print("max parameter difference after %d steps: %.3e (bound %.3e)" % (T, diff, 2 * T * lr))
    assert diff <= 2 * T * lr
    moved = max(float((p1.detach() - p0.detach()).abs().max()) for p1, p0 in zip(m1.parameters(), _model().parameters()))
    assert moved > lr                                             # (the replays trained)


def test_no_host_in_the_loop():
    from two_stage_gnn_amd import post_train as PT
    from two_stage_gnn_amd.data_parallel import FlatTrainer, GraphedStep
    graphs = _dataset()
    m = _model()
    st = PT.PostTrainStream(m, graphs)
    st.load(ANCHORS)
    gs = GraphedStep(FlatTrainer(m, lr=1e-3, clip=0), st.step_loss())
    st.load(ANCHORS)
    T = len(st)
    gs.step()
    gs.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        for _ in range(T):
            gs.step()
        with pytest.raises(RuntimeError):
            gs.loss.cpu()                                         # (the mode is live: a copy to the host IS flagged)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    gs.synchronize()
    assert st.position() == T + 1 and np.isfinite(gs.loss_value())


@pytest.mark.parametrize("chunk", [1, 3, 7])
def test_evaluate_pred(chunk):
    from two_stage_gnn_amd import _native as nat
    from two_stage_gnn_amd import post_train as PT
    from two_stage_gnn_amd import two_stage as TS
    graphs = _dataset()
    m = _model()
    nat.trace = []
    try:
        pred = TS.predict_dataset(graphs, m, chunk=chunk)
        names = [t[0] for t in nat.trace]
    finally:
        nat.trace = None
    assert names.count("mlp_probe_predict_f32") == 1 and m.training
    m.eval()
    want = []
    with torch.no_grad():
        for gobj in graphs:
            z = PT.post_train_step(m, gobj)[1]
            assert float((z[0, 0] - z[0, 1]).abs()) > 1e-4         # (no near tie: the argmax is not a matter of rounding)
            want.append(int(z.argmax(dim=1)))
    m.train()
    assert pred.dtype == torch.int32 and pred.tolist() == want
    y = np.array(LABELS)
    ref = TS.metrics_from_confusion(TS.confusion_matrix(y, np.array(want), np.unique(np.concatenate([y, want]))))
    by_class = {c: [gobj for gobj, l in zip(graphs, LABELS) if l == c] for c in (0, 1)}       # the reference's container
    flat = [gobj for c in (0, 1) for gobj in by_class[c]]
    assert TS.evaluate_pred(graphs, m, chunk=chunk) == ref
    assert TS.evaluate_pred(by_class, m, chunk=chunk) == TS.evaluate_pred(flat, m, chunk=chunk)
    # the fixture: the reference's evaluate() on its final model and six graphs
    g = load_golden("posttrain_gcn")
    mg, objs = _golden_model(g, "final."), _golden_objects(g)
    assert TS.predict_dataset(objs, mg, chunk=chunk).tolist() == g["eval.pred"].tolist()
    got = TS.evaluate_pred(objs, mg, chunk=chunk)
    assert set(got) == {"prec", "recall", "acc", "F1"}
    for k in got:
        assert got[k] == pytest.approx(float(g["eval." + k]), abs=1e-12), k


def test_constructor_refuses_other_models_and_labels():
    from two_stage_gnn_amd import dense_encoders as E
    from two_stage_gnn_amd import post_train as PT
    graphs = _dataset()
    sp = E.SoftPoolingGcnEncoder(U.NMAX, U.FIN, 32, 32, 2, 3, 32, assign_ratio=0.25, num_pooling=1, bn=True, args=A(),
                                 assign_input_dim=U.FIN, final_dim="pretrain").cuda()
    PT.install_head(sp)
    with pytest.raises(TypeError, match="post_train_step"):
        PT.PostTrainStream(sp, graphs)
    m = E.GcnEncoderGraph(U.FIN, HID, HID, 2, 3, bn=True, args=A(), final_dim="output_dim").cuda()
    PT.install_head(m)
    with pytest.raises(TypeError, match="post_train_step"):
        PT.PostTrainStream(m, graphs)
    cpu = E.GcnEncoderGraph(U.FIN, HID, HID, 2, 3, bn=True, args=A(), final_dim="pretrain").cpu()
    cpu.map2_model = PT.make_head(HID, device=torch.device("cpu"))
    with pytest.raises(TypeError, match="post_train_step"):
        PT.PostTrainStream(cpu, graphs)
    m = E.GcnEncoderGraph(U.FIN, HID, HID, 2, 3, bn=True, args=A(), final_dim="pretrain").cuda()
    with pytest.raises(TypeError, match="post_train_step"):
        PT.PostTrainStream(m, graphs)                              # map2_model is still the constructor's single Linear
    m.map2_model = torch.nn.Sequential(torch.nn.Linear(HID, 64), torch.nn.ReLU(), torch.nn.Linear(64, 32), torch.nn.LeakyReLU(),
                                       torch.nn.Linear(32, 2)).cuda()
    with pytest.raises(TypeError, match="post_train_step"):
        PT.PostTrainStream(m, graphs)
    m = _model()
    with pytest.raises(ValueError, match="graph 4"):
        PT.PostTrainStream(m, _dataset(labels=[0, 1, 1, 0, 2, 0, 0]))
    with pytest.raises(ValueError, match="graph 2"):
        PT.PostTrainStream(m, _dataset(labels=[0, 1, -1, 0, 1, 0, 0]))
    assert len(PT.PostTrainStream(m, graphs, max_steps=3)) == 1
