"""The post-training phase of 2stg+ for the GAT encoder on the GPU (two_stage_gnn_amd/gat_stream.py ``PostTrainStream``, the GAT branch
of ``post_train.post_train_step``, csrc/gat_stream.hip's one-piece gather, csrc/posttrain_head.hip's row loss): the anchor gather
alone against ``gat_triplet.assemble``, the triplet gather on the same arena against the same witness, the eager steps against the
reference's own (tests/golden/posttrain_gat.npz), the streamed step against the eager one, an epoch from one hipGraph, poisoned
capacity buffers, the launch trace, ``evaluate_readout`` and the refusals that need a GPU.

``DGATEncoderGraph(final_dim='output_dim')`` returns its readout row first, so the reference's ``pred`` is that row [1, embedding_dim]:
the loss runs over its columns, ``map_model`` / ``map2_model`` get no gradient and do not move.

Datasets: the fixture's seven graphs (Nmax 16: a full graph, a one-node graph, a graph without any edge) and those of
tests/gat_stream_util.py (directed graphs, ldf 4 and 8, two head counts, pieces that span several copy chunks)."""
import copy

import numpy as np
import pytest
import torch

import fp32_yardstick as FY
import gat_stream_util as U
import posttrain_families_ref as FR
import test_gpu_gat_stream as GS
from conftest import load_golden, params_of
from guard_buf import PAT

pytestmark = pytest.mark.gpu

NAME = "posttrain_gat"
IPAT = GS.IPAT
ANCHORS = np.array([0, 1, 6, 3, 3, 5, 2, 4], dtype=np.int64)          # largest then smallest, the edge-less graph, a repeat, every graph


def _golden_model(g, prefix="p."):
    from two_stage_gnn_amd import gat_encoders as G
    from two_stage_gnn_amd import post_train as PT
    fin, hid, emb, lab = (int(v) for v in g["dims"])
    m = G.DGATEncoderGraph(fin, hid, emb, lab, None, num_layers=int(g["num_layers"]), num_heads=[int(h) for h in g["heads"]],
                           final_dim="output_dim").cuda()
    PT.install_head(m)
    m.load_state_dict({k: v.cuda() for k, v in params_of(g, prefix).items()}, strict=True)
    return m.train()


def _case(name):
    """-> (model in training mode, labelled graph objects)"""
    if name == "fixture":
        g = load_golden(NAME)
        return _golden_model(g), FR.golden_objects(g)
    data, cfg = name.split(":")
    return U.model(data, cfg, "train"), U.dataset(data)


def _grads_of(m):
    return {k: p.grad.detach().clone() for k, p in m.named_parameters() if p.grad is not None}


# ------------------------------------------------------------------------------------------------ 1. the gather launches alone
def _check_gather(st, sched, objs):
    """every array the launch writes for every entry of ``sched`` [T, B], into guarded buffers prefilled with NaN / -1: the [:R] /
    [:E] / [:I] prefixes bit for bit ``gat_triplet.assemble`` of the entry's objects, the padding as include/tsgnn.h states it (row
    pointers = E, feature rows +0, row_mult 0, indicator rows 0, row_graph B - 1, row_slot 0, graph_ptr[B] = R, iso_ptr[B] = I; columns,
    entry maps and the list past E / I untouched), the guards intact, ``ids_out`` the entry"""
    from two_stage_gnn_amd import gat_triplet as GT, resident as R
    ar, heads, B = st.arena, st.heads, st.B
    assert (st.row_cap, st.nnz_cap, st.iso_cap) == ar.caps == tuple(B * t for t in ar.top)
    raw = GS._guarded(st)
    dev, cache = st.device, R.ResidentCache()
    st.load(sched)
    for k, ids in enumerate(np.asarray(sched).reshape(len(sched), B)):
        GS._refill(raw)
        st.gather()
        got = GS._read(raw, heads)
        assert st.position() == k + 1 and st.ids_out.tolist() == ids.tolist()
        x, g = GT.assemble([GT.resident_piece(objs[i], dev, cache) for i in ids], dev, heads)
        n, E, I = int(g.n_rows), int(g.nnz), int(g._iso_list[3])
        for what, t in {"rowptr": g.rowptr, "rowptr_t": g._t[0], "graph_ptr": g.graph_ptr, "iso_ptr": g._iso_list[2]}.items():
            assert torch.equal(got[what][:t.numel()], t.cpu()), (k, what)
        for what, t in (("col", g.col), ("col_t", g._t[1]), ("src_e_t", g.src_e_t), ("inv", g._inv_e_t)):
            assert torch.equal(got[what][:E], t.cpu()[:E]) and bool((got[what][E:] == IPAT).all()), (k, what)
        for what, t in (("row_graph", g.row_graph), ("row_slot", g.row_slot)):
            assert torch.equal(got[what][:n], t.cpu()[:n]), (k, what)
        assert torch.equal(got["iso_idx"][:I], g._iso_list[0].cpu()[:I]) and bool((got["iso_idx"][I:] == IPAT).all()), (k, "iso_idx")
        assert torch.equal(got["iso_w"][:I], GS._bits(g._iso_list[1])[:I]) and bool((got["iso_w"][I:] == PAT).all()), (k, "iso_w")
        assert torch.equal(got["row_mult"][:n], GS._bits(g.row_mult)[:n]) and torch.equal(got["x"][:n * ar.ldf], GS._bits(x).view(-1)), (k, "x")
        for h in heads:
            assert torch.equal(got["iso_cols%d" % h][:n * h], GS._bits(g._iso_cols[h]).view(-1)[:n * h]), (k, h)
        assert bool((got["rowptr"][n:] == E).all()) and bool((got["rowptr_t"][n:] == E).all()), (k, "padding rows are empty")
        assert not bool(got["x"][n * ar.ldf:].any()) and not bool(got["row_mult"][n:].any()), (k, "+0")
        assert all(not bool(got["iso_cols%d" % h][n * h:].any()) for h in heads), (k, "indicator")
        assert bool((got["row_graph"][n:] == B - 1).all()) and not bool(got["row_slot"][n:].any()), (k, "row maps")
        assert got["graph_ptr"].tolist()[B] == n and got["iso_ptr"].tolist()[B] == I and got["graph_ptr"].numel() == B + 1


@pytest.mark.parametrize("name", ["fixture", "small3:l2", "small8:l3", "big:l2"])
def test_anchor_gather_equals_assemble_for_every_anchor(name):
    """the one-piece launch for EVERY graph of the dataset as anchor, the largest first and the smallest behind it (what the previous
    gather left must be inert); the fixture holds the full graph (no ghost row), the one-node graph and the edge-less graph (E = 0)"""
    from two_stage_gnn_amd import _native as nat, gat_stream
    m, objs = _case(name)
    st = gat_stream.PostTrainStream(m, objs)
    G_ = len(objs)
    top = int(np.argmax(st.arena.records[:, 2] * (1 << 20) + st.arena.records[:, 3]))
    low = int(np.argmin(st.arena.records[:, 2]))
    order = [top, low] + [i for i in range(G_) if i not in (top, low)] + [top]
    if name == "fixture":
        rec = st.arena.records
        assert rec[0, 1] == rec[0, 2] == 16 and rec[1, 1] == 1 and rec[6, 3] == 0 and st.B == 1 and st.labels.tolist() == [0, 1, 1, 0, 1, 0, 1]
    nat.trace = []
    try:
        _check_gather(st, np.array(order).reshape(-1, 1), objs)
        kernels = {t[2] for t in nat.trace if t[0] == "gat_anchor_gather_f32"}
        entries = [t[0] for t in nat.trace if "gather" in t[0]]
    finally:
        nat.trace = None
    assert kernels == {"gat_anchor_gather_kernel"} and entries == ["gat_anchor_gather_f32"] * len(order)
    need = st.arena.records[:, 2]
    assert need.min() < st.row_cap == need.max()                              # padding rows exist, and one anchor fills the capacity


def test_triplet_gather_on_the_same_arena_is_unchanged():
    """the three-piece instantiation behind ``tsgnn_gat_triplet_gather_f32`` on the fixture's graphs: the same bits as
    ``gat_triplet.assemble`` (the witness of the launch's output before it became a template), padding rows with row_graph 2, and the
    kernel's name"""
    from two_stage_gnn_amd import _native as nat, gat_stream, gat_triplet
    m, objs = _case("fixture")
    st = gat_stream.TripletStream(gat_triplet.tripletnet(m), objs)
    one = gat_stream.pack_arena(objs, batch=1)
    assert np.array_equal(st.arena.buf, one.buf) and np.array_equal(st.arena.records, one.records) and st.arena.caps == tuple(3 * c for c in one.caps)
    sched = np.array([[0, 3, 5], [1, 6, 1], [0, 0, 0], [6, 6, 6], [2, 4, 0], [5, 1, 3]], dtype=np.int64)
    nat.trace = []
    try:
        _check_gather(st, sched, objs)
        kernels = {t[2] for t in nat.trace if t[0] == "gat_triplet_gather_f32"}
    finally:
        nat.trace = None
    assert kernels == {"gat_triplet_gather_kernel"}


# ------------------------------------------------------------------------------------------------ 2. the eager step and the fixture
def test_eager_steps_reproduce_the_fixture():
    """step 0 from the fixture's parameters, then all seven steps under ``FlatTrainer(clip=0)``: ``pred`` and the loss of every step
    and every gradient of step 0 within 8 x the distance of the reference's own fp32 CPU run (the fixture) from the float64
    restatement of its loop (tests/fp32_yardstick.py); ``map_model`` and the head get no gradient (None or exactly zero) and their
    parameters do not move; the other parameters end within 2 T lr of the float64 loop's (the trajectory rule of
    tests/test_gpu_posttrain.py); the step takes the resident piece (``gat_assemble_f32``) and the row-loss launches"""
    from two_stage_gnn_amd import _native as nat
    from two_stage_gnn_amd import post_train as PT
    from two_stage_gnn_amd.data_parallel import FlatTrainer
    g = load_golden(NAME)
    ref64, _ = FR.reference_runs(NAME, g)
    m, objs = _golden_model(g), FR.golden_objects(g)
    T, lr = len(objs), float(g["lr"])
    nat.trace = []
    try:
        loss, pred, out = PT.post_train_step(m, objs[0])
        loss.backward()
        names = [t[0] for t in nat.trace]
    finally:
        nat.trace = None
    assert names.count("gat_assemble_f32") == 1 and names.count("posttrain_rowloss_fwd_f32") == 1 and names.count("posttrain_rowloss_bwd_f32") == 1, names
    assert pred.requires_grad and not out.requires_grad and pred.shape == (1, 8) and out.shape == (1, 2)
    FY._check("s0.pred", pred, ref64["s0.pred"], torch.tensor(g["s0.pred"]))
    FY._check("s0.loss", loss.detach().reshape(1), ref64["s0.loss"], torch.tensor(g["s0.loss"]).reshape(1))
    np.testing.assert_allclose(out.cpu().numpy(), g["s0.out"], rtol=1e-4, atol=1e-5)
    stored = {k[5:] for k in g if k.startswith("s0.g.")}
    frozen = [k for k, _ in m.named_parameters() if k not in stored]
    assert len(stored) == 8 and sorted(frozen) == sorted(k for k, _ in m.named_parameters() if k.startswith(("map_model", "map2_model", "pred_model")))
    for k, p in m.named_parameters():
        if k in stored:
            FY._check("s0.g." + k, p.grad, ref64["s0.g." + k], torch.tensor(g["s0.g." + k]))
        else:
            assert p.grad is None or not bool(p.grad.any()), k
    m = _golden_model(g)
    tr = FlatTrainer(m, lr=lr, clip=0)
    for s, obj in enumerate(objs):
        tr.zero_grad()
        loss, pred, _ = PT.post_train_step(m, obj)
        tr.backward(loss)
        tr.gather_grads()
        tr.apply()
        print("step %d: loss %.7f, reference %.7f" % (s, float(loss.detach()), float(g["s%d.loss" % s])))
        FY._check("s%d.pred" % s, pred, ref64["s%d.pred" % s], torch.tensor(g["s%d.pred" % s]))
        FY._check("s%d.loss" % s, loss.detach().reshape(1), ref64["s%d.loss" % s], torch.tensor(g["s%d.loss" % s]).reshape(1))
    start = params_of(g, "p.")
    worst = 0.0
    for k, p in m.named_parameters():
        if k in frozen:
            assert torch.equal(p.detach().cpu(), start[k]), k                                  # unmoved: zero moments = Adam skipping it
        else:
            worst = max(worst, float((p.detach().cpu().double() - ref64["final." + k]).abs().max()))
            assert float((p.detach().cpu() - start[k]).abs().max()) > lr, k                  # (the steps trained it)
    print("max parameter difference after %d steps: %.3e (bound %.3e)" % (T, worst, 2 * T * lr))
    assert worst <= 2 * T * lr
    with pytest.raises(ValueError, match="label 8 lies outside"):
        bad = FR.GraphObj(dict(objs[0].graph, label=8))
        PT.post_train_step(m, bad)


# ------------------------------------------------------------------------------------------------ 3. the streamed step
def _streamed(m, st):
    m.zero_grad(set_to_none=True)
    loss, pred, out = st.step()
    loss.backward()
    return loss.detach(), pred.detach(), out, _grads_of(m)


@pytest.mark.parametrize("name", ["fixture", "small3:l2", "small8:l3", "big:l2"])
def test_streamed_step_equals_the_eager_step(name):
    """every anchor from equal parameters: loss, ``pred`` and ``out`` of the streamed step are bit for bit those of
    ``post_train_step`` on the same object (the rows are computed by the same row-local kernels whatever the row count, the loss by
    the same launch).  The parameter gradients are compared at 2e-5 max|grad| (tests/test_gpu_posttrain.py's bound for the same
    comparison) and the largest difference is printed: the slab plan of the weight-gradient sums depends on the row count, here the
    capacity, so those sums are not bit for bit (tests/test_gpu_gat_stream.py states the same of the triplet stream)."""
    from two_stage_gnn_amd import gat_stream
    from two_stage_gnn_amd import post_train as PT
    m, objs = _case(name)
    st = gat_stream.PostTrainStream(m, objs)
    anchors = ANCHORS[ANCHORS < len(objs)] if name == "fixture" else np.array([len(objs) - 1, 2, 0, 1, 2] + list(range(3, len(objs) - 1)))
    st.load(anchors)
    for k, i in enumerate(anchors):
        loss, pred, out, gs = _streamed(m, st)
        assert st.ids_out.tolist() == [int(i)] and not out.requires_grad
        m.zero_grad(set_to_none=True)
        lossd, predd, outd = PT.post_train_step(m, objs[i])
        lossd.backward()
        gd = _grads_of(m)
        for what, a, b in (("loss", loss, lossd), ("pred", pred, predd), ("out", out, outd)):
            assert GS._same_bits(a, b), (k, what, float((a - b.detach()).abs().max()))
        assert gs.keys() == gd.keys() and not any(n_.startswith(("map_model", "map2_model", "pred_model")) for n_ in gs)
        scale = max(float(v.abs().max()) for v in gd.values())
        worst = max(float((gs[n_] - gd[n_]).abs().max()) for n_ in gd)
        print("%s entry %d (graph %d): loss %.6f, max|grad| %.3e, max|stream - eager| %.3e (bound %.3e), bit-identical gradients %s"
              % (name, k, i, float(loss), scale, worst, 2e-5 * scale, all(GS._same_bits(gs[n_], gd[n_]) for n_ in gd)))
        assert scale > 0 and worst <= 2e-5 * scale, (k, worst, scale)
    assert st.position() == len(anchors)
    loss, pred, out = st.step(with_out=False)
    assert out is None and st.position() == len(anchors) + 1


def test_an_epoch_from_one_hipgraph_equals_eager_steps():
    """T replays of one ``GraphedStep`` against T eager ``post_train_step`` + ``FlatTrainer(clip=0)`` steps of a deep copy: losses at
    rtol 1e-4, parameters within 2 T lr, and the replays trained (tests/test_gpu_posttrain.py's trajectory rule); the head stays put"""
    from two_stage_gnn_amd import gat_stream, message_passing as mp
    from two_stage_gnn_amd import post_train as PT
    from two_stage_gnn_amd.data_parallel import FlatTrainer, GraphedStep
    m1, objs = _case("fixture")
    m2 = copy.deepcopy(m1)
    start = {k: v.detach().clone() for k, v in m1.state_dict().items()}
    T, lr = len(ANCHORS), 1e-3
    tr2 = FlatTrainer(m2, lr=lr, clip=0)
    eager = []
    for i in ANCHORS:
        tr2.zero_grad()
        loss = PT.post_train_step(m2, objs[i])[0]
        tr2.backward(loss)
        tr2.gather_grads()
        tr2.apply()
        eager.append(float(loss.detach()))
    st = gat_stream.PostTrainStream(m1, objs, max_steps=T)
    assert len(st) == 1 and st.position() == 0                    # the one-entry warm-up schedule
    gs = GraphedStep(FlatTrainer(m1, lr=lr, clip=0), st.step_loss())
    assert gs.describe().startswith("one graph"), gs.describe()
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
    moved = {k: float((p.detach() - start[k]).abs().max()) for k, p in m1.named_parameters()}
    assert max(moved.values()) > lr
    assert all(v == 0.0 for k, v in moved.items() if k.startswith(("map_model", "map2_model", "pred_model")))


# ------------------------------------------------------------------------------------------------ 4. poisoned capacity buffers
@pytest.mark.parametrize("name", ["fixture", "big:l2"])
def test_poisoned_capacity_buffers_change_nothing(name):
    """before every gather both capacity buffers hold NaN / -1 in every word and torch.empty hands the node memory that holds NaN:
    loss, ``pred`` and every gradient are finite and bit for bit the unpoisoned step's"""
    from two_stage_gnn_amd import _native as nat, gat_stream
    m, objs = _case(name)
    st = gat_stream.PostTrainStream(m, objs)
    anchors = ANCHORS[ANCHORS < len(objs)]
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
        st._ibuf.fill_(IPAT)
        st._fbuf.view(torch.int32).fill_(PAT)
        GS._poison(sizes)
        loss, pred, out, gs = _streamed(m, st)
        assert np.isfinite(float(loss)) and bool(torch.isfinite(pred).all()) and all(bool(torch.isfinite(v).all()) for v in gs.values()), (k, i)
        assert GS._same_bits(loss, clean[k][0]) and GS._same_bits(pred, clean[k][1]) and GS._same_bits(out, clean[k][2]), (k, i)
        assert set(gs) == set(clean[k][3])
        for key, v in gs.items():
            assert GS._same_bits(v, clean[k][3][key]), (key, k, float((v - clean[k][3][key]).abs().max()))


# ------------------------------------------------------------------------------------------------ 5. the launch trace, no host copy
def test_launch_trace_and_no_host_in_the_loop():
    """a streamed step's library launches are those of the resident eager step with ``gat_assemble_f32`` replaced by ONE
    ``gat_anchor_gather_f32`` (and without the launches of ``out``, which ``step_loss`` does not compute); torch's own operators are
    kinds the resident step uses too and hold no concatenation, index, gather, scatter, copy or clear; the eager ``post_train_step``
    takes the resident piece and the same loss launches; under sync debug mode "error" two steps run without touching the host"""
    from two_stage_gnn_amd import gat_stream, gat_triplet as GT, resident as R
    from two_stage_gnn_amd import post_train as PT
    m, objs = _case("fixture")
    st = gat_stream.PostTrainStream(m, objs)
    st.load(ANCHORS)
    step = st.step_loss()
    for _ in range(2):                                            # (warm: allocator, library load, the resident piece)
        m.zero_grad(set_to_none=True)
        PT.post_train_step(m, objs[0])[0].backward()
    step().backward()
    st.load(ANCHORS)
    m.zero_grad(set_to_none=True)
    box = {}

    def resident():
        piece = GT.resident_piece(objs[0], st.device, R.resident_cache(m))
        box["b"] = GT.assemble([piece], st.device, GT.head_counts(m))
    asm, _ = GS._traced(resident)
    res, res_ops = GS._traced(lambda: PT.row_loss(GT.readout_rows(m, *box["b"]), PT._const_i32(st.device, 0), PT._const_i32(st.device, 0)).backward())
    m.zero_grad(set_to_none=True)
    got, got_ops = GS._traced(lambda: step().backward())
    print("library launches of a streamed GAT post-training step: %d\n%s\ntorch operators: %s" % (len(got), " ".join(got), " ".join(got_ops)))
    assert asm == ["gat_assemble_f32"]
    assert got == ["gat_anchor_gather_f32"] + res and got.count("gat_anchor_gather_f32") == 1 and "gat_assemble_f32" not in got
    assert got.count("gat_attn_fwd_f32") == 2 and got.count("posttrain_rowloss_fwd_f32") == 1 and got.count("posttrain_rowloss_bwd_f32") == 1
    assert not [o for o in got_ops if any(w in o for w in ("cat", "index", "stack", "gather", "scatter"))]
    assert not [o for o in got_ops if "copy" in o or "_local_scalar" in o or "zero" in o], got_ops     # nothing moves, nothing is cleared
    assert set(got_ops) <= set(res_ops), set(got_ops) - set(res_ops)
    m.zero_grad(set_to_none=True)
    eager, _ = GS._traced(lambda: PT.post_train_step(m, objs[0])[0].backward())
    assert eager.count("gat_assemble_f32") == 1 and "gat_anchor_gather_f32" not in eager and eager.count("posttrain_rowloss_fwd_f32") == 1
    torch.cuda.synchronize()
    pos = st.position()
    torch.cuda.set_sync_debug_mode("error")
    try:
        for _ in range(2):
            loss = step()
            loss.backward()
        with pytest.raises(RuntimeError):
            loss.cpu()                                            # (the mode is live: a copy to the host IS flagged)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert st.position() == pos + 2 and np.isfinite(float(loss.detach()))


# ------------------------------------------------------------------------------------------------ 6. evaluate()
@pytest.mark.parametrize("chunk", [1, 3, 7])
def test_evaluate_readout(chunk):
    """the reference's ``evaluate()`` on its final model and seven graphs: the argmax of the readout row per graph and the metrics"""
    from two_stage_gnn_amd import _native as nat
    from two_stage_gnn_amd import post_train as PT
    g = load_golden(NAME)
    m, objs = _golden_model(g, "final."), FR.golden_objects(g)
    nat.trace = []
    try:
        pred = PT.predict_readout(objs, m, chunk=chunk)
        names = [t[0] for t in nat.trace]
    finally:
        nat.trace = None
    assert names.count("gat_assemble_f32") == -(-len(objs) // chunk) and m.training
    assert pred.dtype == torch.int32 and pred.tolist() == g["eval.pred"].tolist()
    got = PT.evaluate_readout(objs, m, chunk=chunk)
    assert set(got) == {"prec", "recall", "acc", "F1"}
    for k in got:
        assert got[k] == pytest.approx(float(g["eval." + k]), abs=1e-12), k
    by_class = {c: [o for o in objs if o.graph["label"] == c] for c in (0, 1)}               # the reference's container
    assert PT.evaluate_readout(by_class, m, chunk=chunk) == PT.evaluate_readout([o for c in (0, 1) for o in by_class[c]], m, chunk=chunk)
    # ties go to the lowest index: a model whose readout rows are constant
    with torch.no_grad():
        z = torch.zeros(3, 8, device="cuda")
        z[1, 5] = z[1, 2] = 1.0
        assert (z == z.max(dim=1, keepdim=True).values).int().argmax(dim=1).tolist() == [0, 2, 0]


# ------------------------------------------------------------------------------------------------ 7. refusals that need the GPU
def test_constructor_load_and_mine_refuse(monkeypatch):
    from two_stage_gnn_amd import gat_fused, gat_stream, resident
    m, objs = _case("fixture")
    eager = "post_train.post_train_step\\(model, graph\\)$"
    with monkeypatch.context() as mk:
        mk.setattr(resident, "RESIDENT", False)
        with pytest.raises(TypeError, match="RESIDENT.*" + eager):
            gat_stream.PostTrainStream(m, objs)
    with monkeypatch.context() as mk:
        mk.setattr(gat_fused, "FUSED", False)
        with pytest.raises(TypeError, match="heads_ok.*" + eager):
            gat_stream.PostTrainStream(m, objs)
    with pytest.raises(ValueError, match="8 features per node, the model takes 3"):
        gat_stream.PostTrainStream(U.model("small3", "l2"), objs)
    st = gat_stream.PostTrainStream(m, objs, max_steps=4)
    assert len(st) == 1 and st.position() == 0 and st.B == 1
    with pytest.raises(ValueError, match="exceeds"):
        st.load(ANCHORS)
    with pytest.raises(ValueError):
        st.load(np.array([[0, 1, 2]]))                             # a triplet schedule
    assert st.load(ANCHORS[:4]) == 4
    with pytest.raises(RuntimeError, match="no negative to mine"):
        st.mine(torch.zeros(7, 8, device="cuda"), None, 1.0)
    assert np.isfinite(float(st.step()[0].detach())) and st.ids_out.tolist() == [0]


# ------------------------------------------------------------------------------------------------ 8. the row-loss launches alone
@pytest.mark.parametrize("R,C,ld", [(1, 8, 8), (1, 2, 5), (3, 64, 64), (2, 65, 72), (8, 1000, 1003), (1, 1024, 1024)])
def test_row_loss_launches_against_float64(R, C, ld):
    """tsgnn_posttrain_rowloss_fwd_f32 / _bwd_f32 through the C ABI: loss, p = softmax(z) and dz for an upstream gradient of 0.5
    against ``F.cross_entropy(F.softmax(z), label)`` in float64 at 8 x the fp32 CPU expression's own distance from it
    (tests/fp32_yardstick.py).  One column per lane (C <= 64), several per lane, a width that is no multiple of the wave (65, 1000),
    the widest (1024); rows with ld > C whose padding holds NaN; logits of +-30 in row 0 (without the max subtraction the first
    soft-max overflows in fp32 at 89); a permuted ``ids``; guard words behind p and dz; two runs give the same bits."""
    import torch.nn.functional as F
    from guard_buf import Out, _owned
    from two_stage_gnn_amd import _native as nat
    gen = torch.Generator().manual_seed(100 * R + C)
    z = torch.randn(R, C, generator=gen) * 1.5
    z[0, 0], z[0, C - 1] = 30.0, -30.0
    n_labels = R + 3
    ids = torch.randperm(n_labels, generator=gen)[:R].int()
    labels = torch.randint(0, C, (n_labels,), generator=gen).int()
    labels[int(ids[0])] = C - 1                                        # (row 0's true class is its smallest logit: the largest loss)
    y = labels[ids.long()].long()

    def ref(dt):
        zz = z.to(dt).clone().requires_grad_(True)
        p = F.softmax(zz, dim=1)
        loss = F.cross_entropy(p, y)
        loss.backward(gradient=torch.tensor(0.5, dtype=dt))
        return loss.detach().reshape(1), p.detach(), zz.grad
    (l64, p64, d64), (l32, p32, d32) = ref(torch.float64), ref(torch.float32)
    zin = torch.full((R, ld), float("nan"))
    zin[:, :C] = z
    zin, ids_d, lab_d = zin.cuda(), ids.cuda(), labels.cuda()
    g = torch.tensor([0.5], device="cuda")
    assert nat.lib().tsgnn_posttrain_rowloss_supported(C, R) == 1
    runs = []
    for _ in range(2):
        P_, L_, D_ = Out(R, C), Out(1, 1), Out(R, ld)
        nat.trace = []
        try:
            nat.call("posttrain_rowloss_fwd_f32", zin, ld, R, C, ids_d, lab_d, n_labels, P_.mat, L_.mat)
            nat.call("posttrain_rowloss_bwd_f32", P_.mat, R, C, ids_d, lab_d, n_labels, g, D_.mat, ld)
            assert [t[2] for t in nat.trace] == ["posttrain_rowloss_fwd_kernel", "posttrain_rowloss_bwd_kernel"]
        finally:
            nat.trace = None
        P_.rest_untouched("p", _owned(R, C, 0, R, 0, C))
        L_.rest_untouched("loss", _owned(1, 1, 0, 1, 0, 1))
        D_.rest_untouched("dz", _owned(R, ld, 0, R, 0, C))
        runs.append((L_.mat.clone(), P_.mat.clone(), D_.mat[:, :C].clone()))
    what = "rowloss R%d C%d" % (R, C)
    FY._check(what + " loss", runs[0][0].reshape(1), l64, l32)
    FY._check(what + " p", runs[0][1], p64, p32)
    FY._check(what + " dz", runs[0][2], d64, d32)
    assert all(GS._same_bits(a, b) for a, b in zip(*runs))
    # without g_loss the upstream gradient is 1
    D1 = Out(R, ld)
    nat.call("posttrain_rowloss_bwd_f32", runs[0][1], R, C, ids_d, lab_d, n_labels, None, D1.mat, ld)
    torch.testing.assert_close(D1.mat[:, :C], 2.0 * runs[0][2], rtol=1e-6, atol=0.0)
    # the autograd node and its torch composition agree on which they are
    from two_stage_gnn_amd import post_train as PT
    zz = zin[:, :C].clone().requires_grad_(True)
    assert PT.row_loss_ok(zz)
    loss = PT.row_loss(zz, ids_d, lab_d)
    loss.backward(gradient=torch.tensor(0.5, device="cuda"))
    assert GS._same_bits(loss.detach().reshape(1), runs[0][0].reshape(1)) and GS._same_bits(zz.grad, runs[0][2])
    cpu = z.clone().requires_grad_(True)
    assert not PT.row_loss_ok(cpu)
    torch.testing.assert_close(PT.row_loss(cpu, ids, labels), l32.reshape(()))        # the torch composition is the fallback
