"""The EigenGCN half of the 2stg+ post-training phase on the GPU (Code/eigengcn/train_triplet_pre_train.py:170-249: one optimiser step
on the sampler's anchor at B = 1, ``loss = model.loss(model(...), label)``): ``eigen_stream.PostTrainStream`` (anchor gather launch +
the encoder on the gathered one-graph batch + the fused mlp2 + cross-entropy head), the eager drop-in
``eigen_stream.post_train_step`` and ``eigen_stream.evaluate_pred``.

Datasets and models: tests/eigen_stream_util.py's ``small`` configurations and ``big`` (labels b % 3 against label_dim 6).  Anchor
schedules put the largest graph first and then the smallest (everything the large one wrote must be overwritten or be padding) and
repeat an anchor.  Bounds against float64 are tests/test_gpu_eigen_triplet.py's ``_check`` (1e-5 of a tensor's largest entry on
outputs, 1e-4 on gradients, or 10 x what the same computation in fp32 on the CPU misses fp64 by).  The triplet gather on the same
datasets is held bit for bit by tests/test_gpu_eigen_stream.py, unchanged."""
import copy

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import eigen_ref as ER
import eigen_stream_util as U
import eigen_two_stage_util as EU
import test_eigen_triplet_host as H
import test_gpu_eigen_triplet as GT
import test_gpu_gat_stream as GS
from guard_buf import PAT
from test_gpu_eigen_stream import _bits, _expected_bits, _guarded, _read, _same_bits
from test_gpu_sag_stream import _poison

pytestmark = pytest.mark.gpu

ANCHORS = {"small": np.array([0, 2, 11, 11, 1, 3, 7]), "big": np.array([3, 0, 2, 2, 1])}
STEP_CASES = [("small", name, "base") for name in sorted(EU.CONFIGS)] + [("small", sorted(EU.CONFIGS)[0], "nomask"),
                                                                         ("small", sorted(EU.CONFIGS)[-1], "nocon"), ("big", "big", "base")]


def _stream(data, name, var="base", mode="train", **kw):
    from two_stage_gnn_amd import eigen_stream
    m = U.model(data, name, var, mode)
    objs = U.dataset(data, name)
    return m, objs, eigen_stream.PostTrainStream(m, objs, **kw)


def _label(objs, i):
    return int(objs[int(i)].graph["label"])


# ------------------------------------------------------------------------------------------------ 1. the gather launch alone
def anchor_numpy(ar, i):
    """csrc/eigen_stream.hip's ANCHOR form restated on the host arena, in the style of ``eigen_stream_util.gather_numpy`` (which
    states the triplet form): the record of graph ``i`` -> every array at the capacities of ONE largest piece per level; ``bptr_i``
    has row_cap_{i+1} + 2 entries, padding ``row_graph`` is 0, ``graph_ptr_i`` = (0, R_i); a word the launch does not write holds
    IPAT / NaN"""
    from two_stage_gnn_amd import eigen_triplet as ET
    L, J, Jf, ldf, nmax = ar.L, ar.J, ar.Jf, ar.ldf, ar.nmax
    nlev = L + 1
    Rc, Ec = ar.caps
    rec = ar.records[int(i)]
    n, z = [int(v) for v in rec[2:2 + nlev]], [int(v) for v in rec[6:6 + nlev]]
    out = {}
    for v in range(nlev):
        out["rowptr_%d" % v] = np.full(Rc[v] + nmax + 1, z[v], dtype=np.int32)
        out["col_%d" % v] = np.full(max(Ec[v], 1), U.IPAT, dtype=np.int32)
        out["val_%d" % v] = np.full(max(Ec[v], 1), U.FPAT, dtype=np.float32)
        out["graph_ptr_%d" % v] = np.array([0, n[v]], dtype=np.int32)
        out["row_graph_%d" % v] = np.zeros(Rc[v], dtype=np.int32)
        out["row_slot_%d" % v] = np.zeros(Rc[v], dtype=np.int32)
        out["slot_count_%d" % v] = np.array([int(n[v] > s) for s in range(nmax)], dtype=np.int32)
    for v in range(L):
        out["cluster_of_%d" % v] = np.full(Rc[v], -1, dtype=np.int32)
        out["coef_%d" % v] = np.zeros((Rc[v], J), dtype=np.float32)
        out["bptr_%d" % v] = np.full(Rc[v + 1] + 2, n[v], dtype=np.int32)
        out["members_%d" % v] = np.full(Rc[v], U.IPAT, dtype=np.int32)
    out["final"] = np.zeros((Rc[L], Jf), dtype=np.float32) if Jf else None
    out["x"] = np.zeros((Rc[0] + nmax, ldf), dtype=np.float32)
    o = int(rec[0])
    words = int(ET.piece_layout(n, z, J, Jf, ldf)[-1])
    u = ET.unpack_piece(ar.buf[o:o + words], n, z, J, Jf, ldf)
    for v, (rp, col, val) in enumerate(u["graphs"]):
        out["rowptr_%d" % v][:n[v]] = rp[:n[v]]
        out["col_%d" % v][:z[v]] = col
        out["val_%d" % v][:z[v]] = val
        out["row_slot_%d" % v][:n[v]] = np.arange(n[v])
    for v, lv in enumerate(u["levels"]):
        out["cluster_of_%d" % v][:n[v]] = lv["cluster_of"]
        out["coef_%d" % v][:n[v]] = lv["coef"]
        out["members_%d" % v][:n[v]] = lv["members"]
        out["bptr_%d" % v][:n[v + 1] + 1] = lv["bptr"][:n[v + 1] + 1]
    if Jf:
        out["final"][:n[L]] = u["final"]
    out["x"][:n[0]] = u["feats"]
    return out, n, z


@pytest.mark.parametrize("data,name", U.GATHER_CASES)
def test_anchor_gather_equals_assemble_at_b1_and_pads_as_specified(data, name):
    """the anchor launch alone, for every anchor, into guarded buffers prefilled with a NaN / -7 pattern: the [:R_i] / [:E_i] prefixes
    bit for bit ``eigen_triplet.assemble`` of the ONE resident piece (the eager B = 1 batch); EVERY word equal to the restatement
    ``anchor_numpy``; capacities are once the largest piece per level; guards intact; ``ids_out`` is the entry, ``position()`` the
    number of launches; a second walk gives the same bits"""
    from two_stage_gnn_amd import _native as nat
    from two_stage_gnn_amd import eigen_triplet as ET, resident as R
    m, objs, st = _stream(data, name)
    anchors = ANCHORS[data]
    sizes = U.SMALL_SIZES if data == "small" else U.BIG_SIZES
    assert sizes[anchors[0]] == max(sizes) and sizes[anchors[1]] == min(sizes) and len(set(anchors.tolist())) < len(anchors)
    ar = st.arena
    L, J, Jf = ar.L, ar.J, ar.Jf
    assert (st.row_caps, st.nnz_caps) == ar.caps == ar.top and st.B == 1 and st.ids_out.numel() == 1 and ar.batch == 1
    raw = _guarded(st)
    dev, cache = st.device, R.ResidentCache()
    first = None
    for rep in range(2):
        st.load(anchors)
        runs = []
        for k, i in enumerate(anchors):
            raw[0].fill_(U.IPAT)
            raw[1].view(torch.int32).fill_(PAT)
            st.gather()
            assert nat.last_kernel() == "eigen_anchor_gather_kernel"
            got = _read(raw, L)
            assert st.position() == k + 1 and st.ids_out.tolist() == [int(i)]
            runs.append(got)
            if rep:
                continue
            want, Rr, E = anchor_numpy(ar, i)
            for key, w in want.items():
                if w is not None:
                    assert torch.equal(got[key], _expected_bits(w)), (k, int(i), key)
            x, eb = ET.assemble([ET.resident_graph(objs[i], dev, cache, L, J, Jf)], dev)
            for key, t in EU.batch_arrays(eb, x).items():
                if t is None:
                    continue
                t = _bits(t).view(-1)
                lv = int(key[-1]) if key[-1].isdigit() else 0
                if key.startswith("rowptr"):
                    t = t[:Rr[lv] + 1]
                elif key.startswith(("col", "val")):
                    t = t[:E[lv]]
                elif key.startswith("bptr"):
                    t = t[:Rr[lv + 1] + 2]
                elif key == "x":
                    t = t[:Rr[0] * ar.ldf]
                assert torch.equal(got[key][:t.numel()], t), (k, int(i), key)
        if rep:
            for a, b in zip(first, runs):
                assert all(torch.equal(a[key], b[key]) for key in a)
        first = runs


# ------------------------------------------------------------------------------------------------ 2. the streamed step
def _streamed(m, st):
    m.zero_grad(set_to_none=True)
    loss, ypred = st.step()
    loss.backward()
    return loss.detach(), ypred.detach(), U.grads(m)


def _eager(m, obj):
    from two_stage_gnn_amd import eigen_stream
    m.zero_grad(set_to_none=True)
    loss, ypred = eigen_stream.post_train_step(m, obj)
    loss.backward()
    return loss.detach(), ypred.detach(), U.grads(m)


_REF = {}


def _ref(data, name, var, i):
    """tests/eigen_ref.py at B = 1 on graph i from the seeded parameters + ``F.cross_entropy`` + backward, in float64 and float32 on
    the CPU, computed once: {dtype: (ypred, loss, {parameter: grad})}"""
    key = (data, name, var, int(i))
    if key not in _REF:
        c = U.cfg(data, name, var)
        sd = U.seeded_state(U.model(data, name, var, dev="cpu"))
        d = U.dataset(data, name)[int(i)].graph
        out = {}
        for dt in (torch.float64, torch.float32):
            p = {k: v.to(dt).clone().requires_grad_(True) for k, v in sd.items()}
            x, adj, pooled, n0, nl, pm = H.dense_inputs(d, c, dt)
            y = ER.wave_pooling_forward(H._ref_params(p), x, adj, pooled, n0, nl, pm, c["num_layers"], c["pool_sizes"], c["J"], c["Jf"],
                                        concat=True, mask=c["mask"], con_final=c["con_final"], n_linear=len(c["pred_hidden"]) + 1)
            loss = F.cross_entropy(y, torch.tensor([int(d["label"])]))
            loss.backward()
            out[dt] = (y.detach(), loss.detach(), {k: (v.grad if v.grad is not None else torch.zeros_like(v)).detach() for k, v in p.items()})
        _REF[key] = out
    return _REF[key]


def _check_against_fp64(tag, m, loss, ypred, gs, ref):
    r64, r32 = ref[torch.float64], ref[torch.float32]
    assert float(r64[1]) > 0
    GT._check(tag + " ypred", ypred, r64[0], r32[0], 1e-5)
    GT._check(tag + " loss", loss, r64[1], r32[1], 1e-5)
    for k, _ in m.named_parameters():
        assert k in gs, k
        GT._check(tag + " " + k, gs[k], r64[2][k], r32[2][k], 1e-4)


@pytest.mark.parametrize("data,name,var", STEP_CASES)
def test_streamed_step_equals_the_eager_step_and_the_restatement(data, name, var):
    """every anchor from equal parameters (train mode, no dropout), streamed against ``eigen_stream.post_train_step`` on the same object
    and against tests/eigen_ref.py at B = 1 + float64 cross-entropy under ``test_gpu_eigen_triplet._check``.

    Bit for bit: the loss and ``ypred`` (every row of the forward is computed by the same row-local or per-graph kernels whatever the
    row count) and the four ``pred_model`` gradients (the head's launches depend on the readout row alone).  Held to the bound of the
    triplet stream's test instead — ``_check`` against float64 —: every conv gradient, whose split-K plan depends on the row count,
    which is the capacity for the stream and the graph's own for the eager step (the largest difference is printed)."""
    m, objs, st = _stream(data, name, var)
    anchors = ANCHORS[data]
    st.load(anchors)
    for k, i in enumerate(anchors):
        loss, ypred, gs = _streamed(m, st)
        assert st.ids_out.tolist() == [int(i)] and ypred.shape == (1, m.label_dim)
        le, ye, ge = _eager(m, objs[i])
        assert _same_bits(loss, le) and _same_bits(ypred, ye), (k, float(loss), float(le))
        assert set(gs) == set(ge)
        for key in gs:
            if key.startswith("pred_model"):
                assert _same_bits(gs[key], ge[key]), (k, key, float((gs[key] - ge[key]).abs().max()))
        print("%s %s %s entry %d graph %d: max|grad| %.3e, max|streamed - eager| gradient entry %.3e"
              % (data, name, var, k, i, max(float(v.abs().max()) for v in ge.values()), max(float((gs[n_] - ge[n_]).abs().max()) for n_ in ge)))
        ref = _ref(data, name, var, i)
        tag = "%s %s %s entry %d" % (data, name, var, k)
        _check_against_fp64(tag + " streamed", m, loss, ypred, gs, ref)
        _check_against_fp64(tag + " eager", m, le, ye, ge, ref)
    assert st.position() == len(anchors)


def test_one_layer_pred_model_is_composed():
    """a ``pred_model`` that is a single Linear lies outside the fused head: the stream composes ``pred_model`` + ``mp.cross_entropy``
    on ``labels[ids_out]`` and still equals the restatement"""
    from two_stage_gnn_amd import eigen_encoders as EE, eigen_stream, post_train as PT
    name = sorted(EU.CONFIGS)[0]
    c = dict(U.cfg("small", name), pred_hidden=[])
    m = EE.WavePoolingGcnEncoder(c["nmax"], U.FIN["small"], c["hidden"], c["emb"], c["label_dim"], c["num_layers"], num_pool_matrix=c["J"],
                                 num_pool_final_matrix=c["Jf"], pool_sizes=c["pool_sizes"], pred_hidden_dims=[], mask=c["mask"],
                                 args=H.args_of(c))
    m.load_state_dict(U.seeded_state(m))
    m = m.cuda().train()
    objs = U.dataset("small", name)
    st = eigen_stream.PostTrainStream(m, objs)
    assert PT.mlp2_layers(m) is None
    st.load(ANCHORS["small"][:2])
    names, _ = GS._traced(lambda: st.step()[0].backward())
    assert names[0] == "eigen_anchor_gather_f32" and "posttrain_mlp2_ce_fwd_f32" not in names and "softmax_ce_f32" in names
    m.zero_grad(set_to_none=True)
    loss, ypred = st.step()
    want = F.cross_entropy(ypred.detach(), torch.tensor([_label(objs, ANCHORS["small"][1])], device="cuda"))
    torch.testing.assert_close(loss.detach(), want, rtol=1e-5, atol=1e-6)


# ------------------------------------------------------------------------------------------------ 3. poisoned memory
@pytest.mark.parametrize("data,name", [("small", sorted(EU.CONFIGS)[0]), ("big", "big")])
def test_poisoned_capacity_buffers_and_allocator_memory_change_nothing(data, name):
    """the stream's two capacity buffers refilled with NaN / -7 before every step and torch.empty handing out memory that holds NaN:
    loss and every gradient are finite and equal the clean step's at rtol 1e-6 / atol 1e-7"""
    from two_stage_gnn_amd import _native as nat
    m, objs, st = _stream(data, name)
    anchors = ANCHORS[data]
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
        loss = ypred = gs = None
        st._ibuf.fill_(U.IPAT)
        st._fbuf.view(torch.int32).fill_(PAT)
        _poison(sizes)
        loss, ypred, gs = _streamed(m, st)
        assert np.isfinite(float(loss)) and all(bool(torch.isfinite(g).all()) for g in gs.values()), (k, int(i))
        torch.testing.assert_close(loss, clean[k][0], rtol=1e-6, atol=1e-7)
        torch.testing.assert_close(ypred, clean[k][1], rtol=1e-6, atol=1e-7)
        assert set(gs) == set(clean[k][2])
        for key, g in gs.items():
            torch.testing.assert_close(g, clean[k][2][key], rtol=1e-6, atol=1e-7, msg=lambda s_, key=key: "%s entry %d: %s" % (key, k, s_))


# ------------------------------------------------------------------------------------------------ 4. trace, host, capture
def test_launch_trace_and_no_host_in_the_loop():
    """a streamed step's library launches start with the ONE anchor gather launch and hold the fused head by name; torch itself
    dispatches no addmm / mm / softmax / nll operator and nothing from or to the host; under sync debug mode "error" two steps run
    without touching the host"""
    m, objs, st = _stream("big", "big")
    st.load(ANCHORS["big"])
    step = st.step_loss()
    step().backward()                                                         # (warm: allocator, library load)
    m.zero_grad(set_to_none=True)
    names, ops = GS._traced(lambda: step().backward())
    print("library launches of a streamed EigenGCN post-training step: %d\n%s\ntorch operators: %s" % (len(names), " ".join(names), " ".join(ops)))
    assert names[0] == "eigen_anchor_gather_f32" and names.count("eigen_anchor_gather_f32") == 1
    assert not [n for n in names if n in ("eigen_triplet_gather_f32", "eigen_assemble_f32", "softmax_ce_f32", "mlp2_triplet_fwd_f32")]
    assert names.count("posttrain_mlp2_ce_fwd_f32") == 1 and names.count("posttrain_mlp2_ce_bwd_f32") == 1
    assert not [o for o in ops if any(w in o for w in ("addmm", "aten.mm", "softmax", "nll_loss", "linear", "cross_entropy"))], ops
    assert not [o for o in ops if "_to_copy" in o or "_local_scalar" in o], ops   # nothing comes from or goes to the host
    torch.cuda.synchronize()
    pos = st.position()
    torch.cuda.set_sync_debug_mode("error")
    try:
        for _ in range(2):
            loss = step()
            loss.backward()
        with pytest.raises(RuntimeError):
            loss.cpu()                                                        # (the mode is live: a copy to the host IS flagged)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert st.position() == pos + 2 and np.isfinite(float(loss.detach()))


@pytest.mark.parametrize("data,name", [("small", sorted(EU.CONFIGS)[0]), ("big", "big")])
def test_replays_walk_the_anchors_and_move_the_parameters_as_uncaptured_steps(data, name):
    """the triplet phase's trainer, continued: ``FlatTrainer(model, lr, clip, weight_decay)`` takes one triplet-shaped warm step (its
    moments are no longer zero), then ``GraphedStep(trainer, st.step_loss())`` replays an epoch of anchors — ``ids_out`` per replay,
    ``position()`` = the number of replays — and moves the parameters as the same uncaptured streamed steps of a deep-copied model
    and trainer state do: the same route, so rtol 1e-5 / atol 1e-6"""
    from two_stage_gnn_amd import eigen_stream, message_passing as mp
    from two_stage_gnn_amd.data_parallel import FlatTrainer, GraphedStep
    anchors = ANCHORS[data]
    assert len(anchors) >= 5
    m1, objs, st1 = _stream(data, name)
    m2 = copy.deepcopy(m1)
    start = {k: v.detach().clone() for k, v in m1.state_dict().items()}
    st2 = eigen_stream.PostTrainStream(m2, objs)
    st2.load(anchors)
    tr2 = FlatTrainer(m2, lr=1e-3, clip=2.0, weight_decay=1e-4)
    step2 = st2.step_loss()
    for i in anchors:
        tr2.step(step2)
        assert st2.ids_out.tolist() == [int(i)]
    st1.load(anchors)
    gs = GraphedStep(FlatTrainer(m1, lr=1e-3, clip=2.0, weight_decay=1e-4), st1.step_loss())   # (warm-up steps are rolled back ...)
    assert gs.describe().startswith("one graph"), gs.describe()
    st1.load(anchors)                                                                          # ... the epoch starts here
    for i in anchors:
        gs.step()
        gs.synchronize()
        assert st1.ids_out.tolist() == [int(i)]
    assert st1.position() == len(anchors) and np.isfinite(gs.loss_value())
    mp.check_device_errors()
    moved = 0
    for (k, p1), (_, p2) in zip(m1.named_parameters(), m2.named_parameters()):
        torch.testing.assert_close(p1.detach(), p2.detach(), rtol=1e-5, atol=1e-6, msg=lambda s_, k=k: k + ": " + s_)
        moved += int(not torch.equal(p1.detach(), start[k]))
    assert moved >= 8


# ------------------------------------------------------------------------------------------------ 5. evaluation
@pytest.mark.parametrize("chunk", [1, 3, 7])
def test_evaluate_pred_equals_the_per_graph_loop(chunk):
    """``evaluate_pred`` at several chunk sizes: predictions and metrics equal those of the per-graph loop (``post_train_step`` in eval
    mode on one object at a time, arg-max with ties to the lowest class) exactly"""
    from two_stage_gnn_amd import eigen_stream, two_stage as TS
    name = sorted(EU.CONFIGS)[0]
    m = U.model("small", name, mode="train")
    objs = U.dataset("small", name)
    pred = eigen_stream.predict_pred(objs, m, chunk=chunk)
    got = eigen_stream.evaluate_pred(objs, m, chunk=chunk)
    assert m.training and pred.dtype == torch.int32
    m.eval()
    with torch.no_grad():
        rows = torch.cat([eigen_stream.post_train_step(m, o)[1] for o in objs]).cpu()
    m.train()
    loop = (rows == rows.max(dim=1, keepdim=True).values).int().argmax(dim=1)
    assert pred.cpu().tolist() == loop.tolist()
    y = np.array([_label(objs, i) for i in range(len(objs))])
    labels = np.unique(np.concatenate([y, loop.numpy()]))
    want = TS.metrics_from_confusion(TS.confusion_matrix(y, loop.numpy(), labels))
    assert got == want and set(got) == {"prec", "recall", "acc", "F1"}


# ------------------------------------------------------------------------------------------------ 6. refusals
def test_constructor_load_and_mine_refuse():
    from two_stage_gnn_amd import eigen_stream, eigen_triplet
    name = sorted(EU.CONFIGS)[0]
    objs = U.dataset("small", name)
    m = U.model("small", name)
    with pytest.raises(TypeError, match="bare eigen_encoders.WavePoolingGcnEncoder.*post_train_step"):
        eigen_stream.PostTrainStream(eigen_triplet.tripletnet(m, H.args_of(U.cfg("small", name))), objs)     # the wrapper, not the model
    with pytest.raises(TypeError, match="post_train_step"):
        eigen_stream.PostTrainStream(object(), objs)
    with pytest.raises(TypeError, match="GPU only.*post_train_step"):
        eigen_stream.PostTrainStream(U.model("small", name, dev="cpu"), objs)
    with pytest.raises(TypeError, match="dropout.*post_train_step"):
        eigen_stream.PostTrainStream(U.model("small", name, dropout=0.5), objs)
    bad = [EU.GraphObj(dict(o.graph)) for o in objs]
    bad[4].graph["label"] = 6
    with pytest.raises(ValueError, match="graph 4: label 6 lies outside \\[0, 6\\)"):
        eigen_stream.PostTrainStream(m, bad)
    del bad[4].graph["label"]
    with pytest.raises(ValueError, match="graph 4 carries no 'label'"):
        eigen_stream.PostTrainStream(m, bad)
    st = eigen_stream.PostTrainStream(m, objs, max_steps=4)
    assert len(st) == 1 and st.position() == 0 and st.labels.tolist() == [i % 3 for i in range(len(objs))]
    with pytest.raises(ValueError, match="exceeds"):
        st.load(ANCHORS["small"])                                              # seven entries into a buffer of four
    assert st.load(ANCHORS["small"][:4]) == 4 and st.load(ANCHORS["small"][:3].reshape(3, 1)) == 3
    with pytest.raises(ValueError, match="indices"):
        st.load(np.array([0, 12]))
    with pytest.raises(RuntimeError, match="not a triplet"):
        st.mine(torch.zeros(12, 6, device="cuda"), None, 1.0)
    fresh = eigen_stream.PostTrainStream(m, objs)
    with pytest.raises(RuntimeError, match="load"):
        fresh.step()
    st2 = eigen_stream.PostTrainStream(m, objs, max_steps=4)                    # the warm-up schedule serves a step: graph 0
    loss, ypred = st2.step()
    assert np.isfinite(float(loss)) and st2.ids_out.tolist() == [0]
    with pytest.raises(ValueError, match="label 9 lies outside"):
        o = EU.GraphObj(dict(objs[0].graph, label=9))
        eigen_stream.post_train_step(m, o)


# ------------------------------------------------------------------------------------------------ 7. the reference's own loop
@pytest.mark.parametrize("route", ["eager", "streamed"])
def test_three_steps_reproduce_the_reference_with_the_continued_trainer(route):
    """tests/golden/posttrain_eigen.npz (scripts/gen_golden_posttrain_eigen.py): the reference's model and FIRST Adam take one triplet
    step and then three post-training steps on three anchors of different sizes, the clip inactive in the first and active in the
    other two.  Here ONE ``FlatTrainer(lr, clip, weight_decay)`` takes the triplet step through ``eigen_triplet.tripletnet`` and then
    the three steps through ``eigen_stream.post_train_step`` (eager) or ``eigen_stream.PostTrainStream`` (streamed: the schedule names
    every anchor twice, the first entry for a step of its own without the optimiser — the ``ypred``, loss and pre-clip gradients that are
    compared —, the second for the trainer's step).  Per step, ``ypred`` and the loss at rtol = atol = 1e-4 and every pre-clip gradient at rtol 2e-3 / atol 2e-4 (the bounds of the
    ``triplet_eigen_*`` fixture tests); the parameters after every step within 8 x the yardstick of tests/fp32_yardstick.py formed by
    the float64 replay of the reference's own gradients through clip + Adam (``replay_adam``) against the fixture's fp32 parameters."""
    import test_posttrain_sag_eigen_host as PH
    from conftest import load_golden
    from fp32_yardstick import _check
    from two_stage_gnn_amd import eigen_stream, eigen_triplet as ET
    from two_stage_gnn_amd.data_parallel import FlatTrainer
    g = load_golden(PH.FIXTURE)
    c = H.cfg(g)
    m = GT._model(c)
    m.load_state_dict({k[2:]: torch.tensor(v) for k, v in g.items() if k.startswith("p.")}, strict=True)
    m = m.cuda().train()
    dicts, _ = H.graph_dicts(g)
    objs = [H.GraphObj(dict(d)) for d in dicts]
    names = [k for k, _ in m.named_parameters()]
    tr = FlatTrainer(m, lr=float(g["lr"]), clip=float(g["clip"]), weight_decay=float(g["weight_decay"]))    # built ONCE, before the triplet phase
    replay = PH.replay_adam(g)
    net = ET.tripletnet(m, H.args_of(c))
    crit, tgt = ET.MarginRankingLoss(margin=c["margin"]), torch.full((1,), -1.0, device="cuda")

    def params_within(pre, k):
        for n_ in names:
            _check("%s %s%s after" % (route, pre, n_), dict(m.named_parameters())[n_].detach(), torch.from_numpy(replay[k][n_]),
                   torch.from_numpy(g[pre + "p." + n_]))
    tr.step(lambda: crit(*net(*objs)[:2], tgt))
    params_within("triplet.", 0)
    m.map_model = torch.nn.Linear(c["emb"], 2).cuda()           # the head the driver installs now (:170-183): accepted and ignored
    dead = {k: v.detach().clone() for k, v in m.map_model.state_dict().items()}
    st = None
    if route == "streamed":
        st = eigen_stream.PostTrainStream(m, objs)
        st.load(np.repeat(np.arange(3), 2))
    for s in range(3):
        pre = "s%d." % s
        m.zero_grad(set_to_none=True)
        loss, ypred = eigen_stream.post_train_step(m, objs[s]) if st is None else st.step()     # (a backward of its own: nothing moves)
        loss.backward()
        assert st is None or st.ids_out.tolist() == [s]
        np.testing.assert_allclose(ypred.detach().cpu().numpy(), g[pre + "ypred"], rtol=1e-4, atol=1e-4)
        assert abs(float(loss.detach()) - float(g[pre + "loss"])) < 1e-4
        for n_ in names:
            got = dict(m.named_parameters())[n_].grad
            np.testing.assert_allclose(got.cpu().numpy(), g[pre + "g." + n_], rtol=2e-3, atol=2e-4, err_msg=pre + n_)
        m.zero_grad(set_to_none=True)
        if st is None:
            tr.step(lambda: eigen_stream.post_train_step(m, objs[s])[0])
        else:
            tr.step(st.step_loss())
            assert st.ids_out.tolist() == [s] and st.position() == 2 * s + 2
        params_within(pre, s + 1)
    assert all(torch.equal(v, m.map_model.state_dict()[k]) for k, v in dead.items()) and all(q.grad is None for q in m.map_model.parameters())
