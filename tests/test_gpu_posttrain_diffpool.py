"""The post-training phase of 2stg+ for the DiffPool encoder on the GPU (two_stage_gnn_amd/diffpool_stream.py ``PostTrainStream``, the
``SoftPoolingGcnEncoder`` branch of ``post_train.post_train_step``): the eager steps against the reference's own
(tests/golden/posttrain_diffpool.npz), the streamed step against the eager one, an epoch from one hipGraph, poisoned feature rows
and allocator memory, the launch trace with the fused head, ``two_stage.evaluate_pred`` and which models are accepted.

``SoftPoolingGcnEncoder(final_dim='pretrain')`` returns ``(map2_model(map_model(r)), map_model(r))`` on the concatenated readout rows of
every level: the expression csrc/posttrain_head.hip computes, at P = pred_input_dim * (num_pooling + 1).

Datasets: the fixture's six graphs (Nmax 16: a full graph, a one-node graph) and the seven of tests/triplet_stream_util.py with labels
(rows with a CSR tail, an isolated node, Nmax 48 with one pooling level and Nmax 64 with two)."""
import copy

import numpy as np
import pytest
import torch

import fp32_yardstick as FY
import posttrain_families_ref as FR
import triplet_stream_util as U
from conftest import load_golden, params_of

pytestmark = pytest.mark.gpu

NAME = "posttrain_diffpool"
HID = 32
LABELS = [0, 1, 1, 0, 1, 0, 0]
ANCHORS = np.array([0, 1, 4, 1, 1, 6, 3, 2, 5], dtype=np.int64)      # largest then smallest, a repeat, the isolated node, every graph


class A:
    bias = True


def _dataset(nmax=U.NMAX, labels=LABELS):
    out = []
    for g, y in zip(U.dataset(nmax=nmax), labels):
        c = copy.copy(g)
        c.graph = dict(g.graph, label=y)
        out.append(c)
    return out


def _model(nmax=U.NMAX, num_pooling=1, seed=6, hid=HID, final_dim="pretrain"):
    from two_stage_gnn_amd import dense_encoders as E
    from two_stage_gnn_amd import post_train as PT
    torch.manual_seed(seed)
    m = E.SoftPoolingGcnEncoder(nmax, U.FIN, hid, hid, 2, 3, hid, assign_ratio=0.25, num_pooling=num_pooling, bn=True, linkpred=False,
                                args=A(), assign_input_dim=U.FIN, final_dim=final_dim)
    with torch.no_grad():
        for k, p in m.named_parameters():
            if "conv" in k and k.endswith("bias"):
                p.copy_(torch.randn_like(p) * 0.3)           # padded and ghost rows then carry values that can win the max readout
    m = m.cuda()
    PT.install_head(m)
    return m


def _golden_model(g, prefix="p."):
    from two_stage_gnn_amd import dense_encoders as E
    from two_stage_gnn_amd import post_train as PT
    fin, hid, emb, lab = (int(v) for v in g["dims"])
    m = E.SoftPoolingGcnEncoder(int(g["nmax"]), fin, hid, emb, lab, int(g["num_layers"]), hid, assign_ratio=float(g["ratio"]),
                                num_pooling=int(g["num_pooling"]), bn=True, linkpred=False, args=A(), assign_input_dim=fin,
                                final_dim="pretrain").cuda()
    PT.install_head(m)
    m.load_state_dict({k: v.cuda() for k, v in params_of(g, prefix).items()}, strict=True)
    return m.train()


def _case(name):
    if name == "fixture":
        g = load_golden(NAME)
        return _golden_model(g), FR.golden_objects(g), np.array([0, 1, 3, 3, 5, 2, 4], dtype=np.int64)
    nmax, npool = (48, 1) if name == "nmax48" else (64, 2)
    return _model(nmax, npool), _dataset(nmax), ANCHORS


def _grads_of(m):
    return {k: p.grad.detach().clone() for k, p in m.named_parameters() if p.grad is not None}


def _traced(fn):
    from two_stage_gnn_amd import _native as nat
    nat.trace = []
    try:
        fn()
        return [(t[0], t[2]) for t in nat.trace]
    finally:
        nat.trace = None


# ------------------------------------------------------------------------------------------------ 1. the eager step and the fixture
def test_eager_steps_reproduce_the_fixture():
    """step 0 from the fixture's parameters, then all six steps under ``FlatTrainer(clip=0)``: ``pred``, ``out`` and the loss of every
    step and every gradient of step 0 within 8 x the distance of the reference's own fp32 CPU run (the fixture) from the float64
    restatement of its loop (tests/fp32_yardstick.py); the parameters end within 2 T lr of the float64 loop's (the trajectory rule
    of tests/test_gpu_posttrain.py); the fused head's launches are in the trace by name (the module call on dense arrays has none)"""
    from two_stage_gnn_amd import post_train as PT
    from two_stage_gnn_amd.data_parallel import FlatTrainer
    g = load_golden(NAME)
    ref64, _ = FR.reference_runs(NAME, g)
    m, objs = _golden_model(g), FR.golden_objects(g)
    T, lr = len(objs), float(g["lr"])
    box = {}

    def step0():
        box["o"] = PT.post_train_step(m, objs[0])
        box["o"][0].backward()
    trace = _traced(step0)
    names = [t[0] for t in trace]
    loss, pred, out = box["o"]
    assert names.count("posttrain_head_fwd_f32") == 1 and names.count("posttrain_head_bwd_f32") == 1, names
    assert ("posttrain_head_fwd_f32", "posttrain_head_fwd_kernel<1>") in trace and ("posttrain_head_bwd_f32", "posttrain_head_bwd_kernel<1>") in trace
    assert not pred.requires_grad and not out.requires_grad and getattr(m, "_defer_map", False) is False
    assert pred.shape == (1, 2) and out.shape == (1, 8)
    for what, got in (("pred", pred), ("out", out), ("loss", loss.detach().reshape(1))):
        FY._check("s0." + what, got, ref64["s0." + what], torch.tensor(g["s0." + what]).reshape(ref64["s0." + what].shape))
    stored = {k[5:] for k in g if k.startswith("s0.g.")}
    assert len(stored) == 28
    for k, p in m.named_parameters():
        if k in stored:
            FY._check("s0.g." + k, p.grad, ref64["s0.g." + k], torch.tensor(g["s0.g." + k]))
        else:
            assert k.startswith(("pred_model", "pre_pred_model")) and (p.grad is None or not bool(p.grad.any())), k
    m = _golden_model(g)
    tr = FlatTrainer(m, lr=lr, clip=0)
    for s, obj in enumerate(objs):
        tr.zero_grad()
        loss, pred, out = PT.post_train_step(m, obj)
        tr.backward(loss)
        tr.gather_grads()
        tr.apply()
        print("step %d: loss %.7f, reference %.7f" % (s, float(loss.detach()), float(g["s%d.loss" % s])))
        for what, got in (("pred", pred), ("out", out), ("loss", loss.detach().reshape(1))):
            key = "s%d.%s" % (s, what)
            FY._check(key, got, ref64[key], torch.tensor(g[key]).reshape(ref64[key].shape))
    worst = max(float((p.detach().cpu().double() - ref64["final." + k]).abs().max()) for k, p in m.named_parameters())
    print("max parameter difference after %d steps: %.3e (bound %.3e)" % (T, worst, 2 * T * lr))
    assert worst <= 2 * T * lr


# ------------------------------------------------------------------------------------------------ 2. the streamed step
def _streamed(m, st):
    m.zero_grad(set_to_none=True)
    loss, pred, out = st.step()
    loss.backward()
    return loss.detach(), pred.detach(), out.detach(), _grads_of(m)


@pytest.mark.parametrize("name", ["fixture", "nmax48", "nmax64"])
def test_streamed_step_equals_the_eager_step(name):
    """every anchor from equal parameters: loss, logits and ``out`` of the streamed step against ``post_train_step`` on the same
    object at rtol = atol = 1e-5 and every parameter gradient at 2e-5 max|grad| — the bounds tests/test_gpu_posttrain.py holds the
    same comparison to for the plain encoder.  Not bit for bit: on the gathered batch the first contraction runs as
    ``diffpool._ContractCap``, whose sums differ from the eager route's in order (tests/test_gpu_diffpool_stream.py); whether an entry
    is bit-identical is printed.  nmax48: one pooling level, K = 12; nmax64: two levels, K = 16 and 4."""
    from two_stage_gnn_amd import diffpool_stream
    from two_stage_gnn_amd import post_train as PT
    m, objs, anchors = _case(name)
    st = diffpool_stream.PostTrainStream(m, objs)
    assert st.B == 1 and st.labels.tolist() == [int(o.graph["label"]) for o in objs] and st.ids_out.numel() == 1
    st.load(anchors)
    _streamed(m, st)                                              # (warm, as tests/test_gpu_diffpool_stream.py's trace: what the persistent
    st.load(anchors)                                              # batch builds once, at its first use, is not part of a step)
    for k, i in enumerate(anchors):
        box = {}
        names = [t[0] for t in _traced(lambda: box.update(o=_streamed(m, st)))]
        loss, pred, out, gs = box["o"]
        assert st.ids_out.tolist() == [int(i)]
        assert names[0] == "triplet_gather_f32" and names.count("triplet_gather_f32") == 1 and "row_maps" not in names, names
        assert names.count("posttrain_head_fwd_f32") == 1 and names.count("posttrain_head_bwd_f32") == 1 and names.count("contract_cap_bwd_f32") == 1
        m.zero_grad(set_to_none=True)
        lossd, predd, outd = PT.post_train_step(m, objs[i])
        lossd.backward()
        gd = _grads_of(m)
        for a, b in ((loss, lossd), (pred, predd), (out, outd)):
            torch.testing.assert_close(a.detach(), b.detach(), rtol=1e-5, atol=1e-5)
        assert gs.keys() == gd.keys() and all(("map2_model.%d.%s" % (j, w)) in gs for j in (0, 2, 4) for w in ("weight", "bias"))
        scale = max(float(v.abs().max()) for v in gd.values())
        worst = max(float((gs[n_] - gd[n_]).abs().max()) for n_ in gd)
        same = all(torch.equal(gs[n_], gd[n_]) for n_ in gd) and torch.equal(pred, predd.detach())
        print("%s entry %d (graph %d): loss %.6f, max|grad| %.3e, max|stream - eager| %.3e (bound %.3e), bit-identical %s"
              % (name, k, i, float(loss), scale, worst, 2e-5 * scale, same))
        assert scale > 0 and worst <= 2e-5 * scale, (k, worst, scale)
    assert st.position() == len(anchors)


def test_an_epoch_from_one_hipgraph_equals_eager_steps():
    from two_stage_gnn_amd import diffpool_stream, message_passing as mp
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
    st = diffpool_stream.PostTrainStream(m1, graphs, max_steps=T)
    assert len(st) == 1 and st.position() == 0                    # the one-entry warm-up schedule
    gs = GraphedStep(FlatTrainer(m1, lr=lr, clip=0), st.step_loss())
    st.load(ANCHORS)                                              # after the warm-up steps: cursor := 0
    streamed = []
    for i in ANCHORS:
        gs.step()
        gs.synchronize()
        assert st.ids_out.tolist() == [int(i)]
        streamed.append(gs.loss_value())
    assert st.position() == T
    mp.check_device_errors()
    print("losses streamed %s eager %s" % (streamed, eager))
    np.testing.assert_allclose(streamed, eager, rtol=1e-4)
    diff = max(float((p1.detach() - p2.detach()).abs().max()) for p1, p2 in zip(m1.parameters(), m2.parameters()))
    print("max parameter difference after %d steps: %.3e (bound %.3e)" % (T, diff, 2 * T * lr))
    assert diff <= 2 * T * lr
    moved = max(float((p1.detach() - p0.detach()).abs().max()) for p1, p0 in zip(m1.parameters(), _model().parameters()))
    assert moved > lr                                             # (the replays trained)


def test_no_host_in_the_loop():
    from two_stage_gnn_amd import diffpool_stream
    m, objs, anchors = _case("nmax48")
    st = diffpool_stream.PostTrainStream(m, objs)
    st.load(anchors)
    step = st.step_loss()
    step().backward()
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        for _ in range(2):
            loss = step()
            loss.backward()
        with pytest.raises(RuntimeError):
            loss.cpu()                                            # (the mode is live: a copy to the host IS flagged)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert st.position() == 3 and np.isfinite(float(loss.detach()))


# ------------------------------------------------------------------------------------------------ 3. poisoned capacity buffers
@pytest.mark.parametrize("name", ["fixture", "nmax64"])
def test_poisoned_feature_rows_change_nothing(name):
    """before every gather the capacity batch's feature rows hold NaN in every word and torch.empty hands the nodes memory that holds
    NaN: loss, logits and every gradient are finite and bit for bit the unpoisoned step's.  (Only the float array is poisoned: the
    gather rewrites every word of it, tests/test_gpu_triplet_stream.py; an index array left with a poison word would be followed.)"""
    from two_stage_gnn_amd import _native as nat, diffpool_stream
    m, objs, anchors = _case(name)
    st = diffpool_stream.PostTrainStream(m, objs)
    st.load(anchors)
    nat.trace = []
    try:
        clean = [_streamed(m, st) for _ in anchors]
        sizes = sorted({a.untyped_storage().nbytes() for t in nat.trace for a in t[1] if isinstance(a, torch.Tensor)})
    finally:
        nat.trace = None
    assert len(sizes) > 8
    st.load(anchors)
    for k, i in enumerate(anchors):
        st.x.fill_(float("nan"))
        ts = [torch.empty(max(n // 4, 1), dtype=torch.float32, device="cuda") for n in sizes for _ in range(3)]
        for t in ts:
            t.fill_(float("nan"))
        torch.cuda.synchronize()
        del ts
        loss, pred, out, gs = _streamed(m, st)
        assert np.isfinite(float(loss)) and bool(torch.isfinite(pred).all()) and all(bool(torch.isfinite(v).all()) for v in gs.values()), (k, i)
        for a, b in zip((loss, pred, out), clean[k][:3]):
            assert torch.equal(a, b), (k, i)
        assert set(gs) == set(clean[k][3])
        for key, v in gs.items():
            assert torch.equal(v, clean[k][3][key]), (key, k, float((v - clean[k][3][key]).abs().max()))


# ------------------------------------------------------------------------------------------------ 4. evaluate()
@pytest.mark.parametrize("chunk", [1, 3, 7])
def test_evaluate_pred_against_the_fixture(chunk):
    """``two_stage.evaluate_pred`` already applies to this encoder: the reference's ``evaluate()`` on its final model and six graphs"""
    from two_stage_gnn_amd import two_stage as TS
    g = load_golden(NAME)
    m, objs = _golden_model(g, "final."), FR.golden_objects(g)
    assert TS.predict_dataset(objs, m, chunk=chunk).tolist() == g["eval.pred"].tolist()
    got = TS.evaluate_pred(objs, m, chunk=chunk)
    assert set(got) == {"prec", "recall", "acc", "F1"}
    for k in got:
        assert got[k] == pytest.approx(float(g["eval." + k]), abs=1e-12), k


# ------------------------------------------------------------------------------------------------ 5. which models are taken
def test_accepted_and_refused_models():
    """one- and two-level models are accepted; a model whose stacks do not run as the fused nodes, the triplet setting's final_dim,
    a model without the installed head and a label the head has no class for are refused; ``mine()`` refuses"""
    from two_stage_gnn_amd import dense_encoders as E
    from two_stage_gnn_amd import diffpool_stream as D
    from two_stage_gnn_amd import post_train as PT
    graphs, graphs64 = _dataset(), _dataset(64)
    eager = "post_train.post_train_step\\(model, graph\\)$"
    one = D.PostTrainStream(_model(U.NMAX, 1), graphs, max_steps=3)
    two = D.PostTrainStream(_model(64, 2), graphs64, max_steps=3)
    assert len(one) == len(two) == 1 and one.B == two.B == 1 and one.n_classes == 2
    assert one._readout_width(one.model) == 2 * 3 * HID and two._readout_width(two.model) == 3 * 3 * HID
    assert np.isfinite(float(one.step()[0].detach())) and np.isfinite(float(two.step()[0].detach())) and one.ids_out.tolist() == [0]
    with pytest.raises(TypeError, match="fused per-graph node.*" + eager):       # stacks wider than the fused per-graph node takes
        D.PostTrainStream(_model(U.NMAX, hid=136), graphs)
    with pytest.raises(TypeError, match=eager):
        D.PostTrainStream(_model(U.NMAX, final_dim="output_dim"), graphs)
    m = E.SoftPoolingGcnEncoder(U.NMAX, U.FIN, HID, HID, 2, 3, HID, assign_ratio=0.25, num_pooling=1, bn=True, linkpred=False, args=A(),
                                assign_input_dim=U.FIN, final_dim="pretrain").cuda()
    with pytest.raises(TypeError, match="install_head.*" + eager):
        D.PostTrainStream(m, graphs)                               # map2_model is still the constructor's single Linear
    with pytest.raises(ValueError, match="graph 4"):
        D.PostTrainStream(_model(), _dataset(labels=[0, 1, 1, 0, 2, 0, 0]))
    with pytest.raises(TypeError, match=eager):                    # the plain encoder's stream keeps refusing this one
        PT.PostTrainStream(_model(), graphs)
    with pytest.raises(ValueError, match="exceeds"):
        one.load(ANCHORS)
    assert one.load(ANCHORS[:3]) == 3
    with pytest.raises(RuntimeError, match="no negative to mine"):
        one.mine(torch.zeros(7, HID, device="cuda"), None, 1.0)
