"""The SAGPool half of the 2stg+ post-training phase on the GPU (Code/sag/train_triplet_pre_train.py:219-263: one optimiser step per
graph on ``F.nll_loss(model(data), data.y)``): ``sag_stream.PostTrainStream`` (anchor gather launch + ``sag_stack`` on the B = 1
capacity plan + the fused mlp3 + nll head), the eager drop-in ``sag_stream.post_train_step`` and ``sag_stream.test_dataset``.

Datasets: tests/sag_stream_util.py's ``small6`` and ``dd3`` with labels that cover the first and the last class.  Anchor schedules
put the largest graph first and then the smallest (everything the large one wrote must be overwritten or be padding) and repeat an
anchor.  ``torch_geometric`` is not installed, so parity with the reference's ``Net`` itself stays unpinned, as for the triplet step:
the step is pinned against the CPU oracle tests/test_gpu_sag_triplet.py uses (oracle/pyg_ref.py), in fp64 and fp32, extended by
``F.nll_loss``.  The triplet gather on the same datasets is held bit for bit by tests/test_gpu_sag_stream.py, unchanged."""
import copy

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import sag_stream_util as U
import test_gpu_gat_stream as GS
from guard_buf import GUARD, PAT
from test_gpu_sag_stream import IPAT, _Guarded, _bits, _grads, _poison
from test_gpu_sag_triplet import _bound, _oracle_embed, _params

pytestmark = pytest.mark.gpu

LABELS = {"small6": [0, 7, 3, 7, 0, 5], "dd3": [63, 0, 17]}             # C = 8 / 64: the first and the last class occur
ANCHORS = {"small6": np.array([4, 0, 2, 2, 5, 1, 3]), "dd3": np.array([1, 0, 2, 2, 1])}


def _datas(name, on_device=True):
    datas = U.datas(U.dataset(name)[3])
    for d, y in zip(datas, LABELS[name]):
        d.y = torch.tensor([y], device="cuda" if on_device else "cpu")
    return datas


def _stream(name, mode="eval", p_drop=0.0, **kw):
    from two_stage_gnn_amd import sag_stream
    m = U.net(name, mode, p_drop)
    datas = _datas(name)
    return m, datas, sag_stream.PostTrainStream(m, datas, **kw)


# ------------------------------------------------------------------------------------------------ 1. the gather launch alone
def _gather(st, ratio):
    from two_stage_gnn_amd import _native as nat
    from two_stage_gnn_amd.triplet_stream import HEAD
    ar, R, depth = st.arena, st.row_cap, st.plan.depth
    B = {"rowptr": _Guarded(R + 1, torch.int32), "col": _Guarded(st.nnz_cap, torch.int32), "x": _Guarded(R * ar.ld, torch.float32),
         "dinv": _Guarded(R, torch.float32), "self_w": _Guarded(R, torch.float32), "gp": _Guarded(4 * (depth + 1), torch.int32),
         "ids": _Guarded(1, torch.int32)}
    nat.call("sag_anchor_gather_f32", st.records, ar.n_graphs, st.buf, ar.off["rowptr"], ar.off["col"], ar.words, st.feats, ar.ld,
             ar.caps[0], ar.caps[1], st._sched[HEAD:], st.max_steps, st._sched, st._sched[4:HEAD], R, st.nnz_cap, float(ratio), depth,
             B["rowptr"].t, B["col"].t, B["x"].t, ar.ld, B["dinv"].t, B["self_w"].t, B["gp"].t, B["ids"].t)
    assert nat.last_kernel() == "sag_anchor_gather_kernel"
    return {k: v.get(k) for k, v in B.items()}


@pytest.mark.parametrize("name", ["small6", "dd3"])
def test_anchor_gather_equals_the_eager_b1_batch(name):
    """the anchor launch alone into guarded buffers prefilled with NaN / -1, for every anchor: every array against
    ``tripletnet.batch_of((data,))``, ``gcn_coef`` and ``SagPlan.get`` on that one object, bit for bit; padding as specified (empty rows:
    every row pointer from n on = nnz, +0 features and coefficients, columns past nnz not touched); the graph pointer rows are
    (0, k_l, k_l, k_l); capacities are ONCE the largest graph; guards intact; ``ids_out`` and ``position()``.  A capacity below the
    arena's bound is refused without a launch."""
    from two_stage_gnn_amd import _native as nat
    from two_stage_gnn_amd import sag_triplet
    from two_stage_gnn_amd.sag_stack import SagPlan, gcn_coef
    from two_stage_gnn_amd.triplet_stream import HEAD
    m, datas, st = _stream(name)
    net = sag_triplet.tripletnet(m)
    anchors = ANCHORS[name]
    sizes = U.SIZES[name]
    assert sizes[anchors[0]] == max(sizes) and sizes[anchors[1]] == min(sizes) and len(set(anchors.tolist())) < len(anchors)
    ar, R, fin = st.arena, st.row_cap, st.arena.fin
    assert R == max(sizes) and st.B == 1 and st.ids_out.numel() == 1
    for ratio in (U.RATIO, 0.3):
        st.load(anchors)
        for k, i in enumerate(anchors):
            got = _gather(st, ratio)
            assert st.position() == k + 1 and got["ids"].tolist() == [int(i)]
            b = net.batch_of((datas[i],))
            n, nnz = int(b.g.n_rows), int(b.g.nnz)
            rp = got["rowptr"]
            assert torch.equal(rp[:n + 1], b.g.rowptr.cpu()) and bool((rp[n:] == nnz).all()) and int(rp[R]) == nnz, (k, "rowptr")
            assert torch.equal(got["col"][:nnz], b.g.col.cpu()[:nnz]) and bool((got["col"][nnz:] == IPAT).all()), (k, "col")
            x = got["x"].view(R, ar.ld)
            assert torch.equal(x[:n, :fin], _bits(b.x)) and not bool(x[:n, fin:].any()) and not bool(x[n:].any()), (k, "x")
            dinv, self_w = gcn_coef(b.g)
            for what, want in (("dinv", dinv), ("self_w", self_w)):
                assert torch.equal(got[what][:n], _bits(want)) and not bool(got[what][n:].any()), (k, what)
            plan = SagPlan.get(b.sizes, ratio, b.x.device, depth=3)
            gp = got["gp"].view(4, 4)
            for l in range(4):
                kl = plan.levels[l].gp.cpu().tolist()
                assert kl[0] == 0 and gp[l].tolist() == [0, kl[1], kl[1], kl[1]], (k, ratio, l)
    small = torch.zeros(R, dtype=torch.int32, device="cuda")
    rc = nat.lib().tsgnn_sag_anchor_gather_f32(
        *[nat._arg(a) for a in (st.records, ar.n_graphs, st.buf, ar.off["rowptr"], ar.off["col"], ar.words, st.feats, ar.ld, ar.caps[0],
                                ar.caps[1], st._sched[HEAD:], st.max_steps, st._sched, st._sched[4:HEAD], R - 1, st.nnz_cap, 0.5, 3, small,
                                st.col, st._x, ar.ld, st.dinv, st.self_w, st.plan.gp_all, st.ids_out)], nat.stream_handle())
    assert rc == -1 and st.position() == len(anchors)     # TSGNN_EINVAL, nothing launched: the cursor stands where the last walk left it


# ------------------------------------------------------------------------------------------------ 2. the streamed step
def _streamed(m, st):
    m.zero_grad(set_to_none=True)
    loss, out = st.step()
    loss.backward()
    return loss.detach(), out.detach(), _grads(m)


def _eager(m, d):
    from two_stage_gnn_amd import sag_stream
    m.zero_grad(set_to_none=True)
    loss, out = sag_stream.post_train_step(m, d)
    loss.backward()
    return loss.detach(), out.detach(), _grads(m)


_ORACLE = {}


def _oracle(name, i):
    """the fp64 and fp32 CPU oracle's step on graph i alone (B = 1 forward, ``F.nll_loss``, backward), computed once:
    {dtype: (out, loss, {parameter: grad})}"""
    if (name, i) not in _ORACLE:
        fin, nhid, C, graphs = U.dataset(name)
        m = U._net(fin, nhid, C, "gcn", False, 0.0, seed=U.NET_SEED, dev="cpu")
        res = {}
        for dt in (torch.float64, torch.float32):
            p = _params(m, dt)
            x, ei = graphs[i]
            out = _oracle_embed(p, x.to(dt), ei, "gcn")
            loss = F.nll_loss(out, torch.tensor([LABELS[name][i]]))
            loss.backward()
            res[dt] = (out.detach(), float(loss.detach()), {k: v.grad for k, v in p.items()})
        _ORACLE[(name, i)] = res
    return _ORACLE[(name, i)]


def _check_vs_oracle(name, k, i, loss, out, gs):
    """test_gpu_sag_stream._check_vs_oracle's bounds for one graph: ``out`` at rtol = atol = 1e-5, the loss at 1e-5 or 10 x the fp32
    oracle's own error, gradients at 1e-4 of the tensor's largest entry (+ 1e-9) or 10 x the fp32 oracle's own error"""
    ref = _oracle(name, int(i))
    (o64, l64, g64), (o32, l32, g32) = ref[torch.float64], ref[torch.float32]
    assert l64 > 0.0
    diff = (out.cpu().double() - o64).abs()
    print("%s entry %d out: |hip - fp64| %.2e, |cpu fp32 - fp64| %.2e" % (name, k, float(diff.max()), float((o32.double() - o64).abs().max())))
    assert bool((diff <= 1e-5 + 1e-5 * o64.abs()).all()), (k, float(diff.max()))
    assert abs(float(loss) - l64) <= max(1e-5 * max(1.0, abs(l64)), 10 * abs(l32 - l64)), (k, float(loss), l64, l32)
    assert set(gs) == set(g64) and len(gs) == 18
    for key, r64 in g64.items():
        err = float((gs[key].cpu().double() - r64).abs().max())
        bound, e_cpu = _bound(r64, g32[key], 1e-4, 1e-9)
        assert err <= bound, (k, key, err, e_cpu, float(r64.abs().max()))


HEAD_KEYS = ("lin1.weight", "lin1.bias", "lin2.weight", "lin2.bias", "lin3.weight", "lin3.bias")


@pytest.mark.parametrize("mode", ["eval", "train"])
@pytest.mark.parametrize("name", ["small6", "dd3"])
def test_streamed_step_equals_the_eager_step_and_the_oracle(name, mode):
    """every anchor from equal parameters (eval mode; training mode with dropout_ratio 0), streamed against
    ``sag_stream.post_train_step`` on the same object and against the fp64 / fp32 CPU oracle.

    Bit for bit: the loss and ``out`` on both datasets (the node's forward sums a row in the same order at any row count, and the
    head sees the same readout row), the six head gradients on both datasets (the head's launches depend on the readout row alone),
    and every conv / score-layer gradient on ``small6`` (its narrow level 0 and 32-wide levels sum in the same order at any row
    count).  Held to the triplet stream test's bound instead — the oracle's, ``_check_vs_oracle`` —: the conv / score-layer gradients of
    ``dd3``, whose weight-gradient slab plan depends on the row count, which is the capacity for the stream and the graph's own for
    the eager step (the difference is printed)."""
    m, datas, st = _stream(name, mode)
    anchors = ANCHORS[name]
    st.load(anchors)
    for k, i in enumerate(anchors):
        loss, out, gs = _streamed(m, st)
        assert st.ids_out.tolist() == [int(i)]
        le, oe, ge = _eager(m, datas[i])
        assert out.shape == oe.shape == (1, m.num_classes)
        assert torch.equal(_bits(loss), _bits(le)) and torch.equal(_bits(out), _bits(oe)), (k, float(loss), float(le))
        assert set(gs) == set(ge)
        exact = list(gs) if name == "small6" else HEAD_KEYS
        for key in exact:
            assert torch.equal(_bits(gs[key]), _bits(ge[key])), (k, key, float((gs[key] - ge[key]).abs().max()))
        worst = max(float((gs[n_] - ge[n_]).abs().max()) for n_ in ge)
        print("%s %s entry %d graph %d: max|grad| %.3e, max|streamed - eager| gradient entry %.3e"
              % (name, mode, k, i, max(float(v.abs().max()) for v in ge.values()), worst))
        _check_vs_oracle(name, k, i, loss, out, gs)
        _check_vs_oracle(name, k, i, le, oe, ge)
    assert st.position() == len(anchors)


def test_dropout_mask_is_drawn_in_the_head_launch():
    """train mode, p = 0.5: the step's ``out`` is the head applied to the step's readout row with the mask
    ``mp.mlp3_dropout_mask`` regenerates from the launch's counter for B = 1, and two steps on the same anchor draw different masks"""
    from two_stage_gnn_amd import _native as nat
    from two_stage_gnn_amd import message_passing as mp
    m, datas, st = _stream("small6", "train", 0.5)
    st.load(np.array([4, 4]))
    masks, outs = [], []
    for _ in range(2):
        nat.trace = []
        try:
            loss, out = st.step()
            loss.backward()
            names = [t[0] for t in nat.trace]
        finally:
            nat.trace = None
        assert names.count("posttrain_mlp3_nll_fwd_f32") == 1 and names.count("posttrain_mlp3_nll_bwd_f32") == 1
        p, seed, used = mp.last_mlp3_dropout
        assert p == 0.5
        mask = mp.mlp3_dropout_mask(p, seed, used, 1, m.lin1.out_features)
        with torch.no_grad():
            r = st.readout()                                                  # (no gather in between: the same batch)
            h = F.relu(F.linear(r, m.lin1.weight, m.lin1.bias)) * mask * 2.0
            h = F.relu(F.linear(h, m.lin2.weight, m.lin2.bias))
            want = F.log_softmax(F.linear(h, m.lin3.weight, m.lin3.bias), dim=-1)
        torch.testing.assert_close(out.detach(), want, rtol=1e-5, atol=1e-6)
        assert abs(float(loss) + float(want[0, LABELS["small6"][4]])) <= 1e-5
        masks.append(mask.cpu())
        outs.append(out.detach().cpu())
        assert all(bool(torch.isfinite(q.grad).all()) for q in m.parameters())
    assert not torch.equal(masks[0], masks[1]) and not torch.equal(outs[0], outs[1])
    assert 0.2 < float(masks[0].mean()) < 0.8


# ------------------------------------------------------------------------------------------------ 3. poisoned memory
@pytest.mark.parametrize("name", ["small6", "dd3"])
def test_poisoned_capacity_buffers_and_allocator_memory_change_nothing(name):
    """the stream's capacity buffers refilled with NaN / -1 before every step and torch.empty handing the node memory that holds
    NaN: loss and every gradient are finite and equal the clean step's at rtol 1e-6 / atol 1e-7 (test_poisoned_padding_changes_nothing's)"""
    from two_stage_gnn_amd import _native as nat
    m, datas, st = _stream(name, "train")
    anchors = ANCHORS[name]
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
        loss = out = gs = None
        for t in (st.rowptr, st.col, st.plan.gp_all):
            t.fill_(IPAT)
        for t in (st._x, st.dinv, st.self_w):
            t.view(torch.int32).fill_(PAT)
        _poison(sizes)
        loss, out, gs = _streamed(m, st)
        assert np.isfinite(float(loss)) and all(bool(torch.isfinite(g).all()) for g in gs.values()), (k, int(i))
        torch.testing.assert_close(loss, clean[k][0], rtol=1e-6, atol=1e-7)
        torch.testing.assert_close(out, clean[k][1], rtol=1e-6, atol=1e-7)
        assert set(gs) == set(clean[k][2])
        for key, g in gs.items():
            torch.testing.assert_close(g, clean[k][2][key], rtol=1e-6, atol=1e-7, msg=lambda s_, key=key: "%s entry %d: %s" % (key, k, s_))


# ------------------------------------------------------------------------------------------------ 4. trace, host, capture
def test_launch_trace_and_no_host_in_the_loop():
    """a streamed step's library launches start with the ONE anchor gather launch, hold the capacity forms of the three levels and
    the fused head by name, and none of the launches the gather replaces; torch itself dispatches no addmm / mm / log_softmax / nll
    operator and no host-to-device copy; under sync debug mode "error" two steps run without touching the host"""
    m, datas, st = _stream("dd3", "train", 0.5)
    st.load(ANCHORS["dd3"])
    step = st.step_loss()
    step().backward()                                                         # (warm: allocator, library load)
    m.zero_grad(set_to_none=True)
    names, ops = GS._traced(lambda: step().backward())
    print("library launches of a streamed SAGPool post-training step: %d\n%s\ntorch operators: %s" % (len(names), " ".join(names), " ".join(ops)))
    assert names[0] == "sag_anchor_gather_f32" and names.count("sag_anchor_gather_f32") == 1 and "sag_triplet_gather_f32" not in names
    assert names.count("sag_pool_graph_cap_f32") == 3 and names.count("sag_pool_graph_bwd_cap_f32") == 3
    assert names.count("posttrain_mlp3_nll_fwd_f32") == 1 and names.count("posttrain_mlp3_nll_bwd_f32") == 1
    assert not [n for n in names if n in ("gcn_coef_f32", "row_maps", "scan_short_i32", "csr_filter_fill", "sag_pool_graph_f32",
                                          "sag_pool_graph_bwd_f32", "mlp3_fwd_f32", "mlp3_fwd_drop_f32", "mlp3_bwd2_f32", "softmax_ce_f32")]
    assert not [o for o in ops if any(w in o for w in ("addmm", "aten.mm", "log_softmax", "nll_loss", "linear", "bernoulli", "dropout"))], ops
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


@pytest.mark.parametrize("name", ["small6", "dd3"])
def test_replays_walk_the_anchors_and_move_the_parameters_as_uncaptured_steps(name):
    """``GraphedStep(FlatTrainer(model, lr=1e-3, clip=0), st.step_loss())``: an epoch of replays walks the schedule (``ids_out`` per
    replay, ``position()`` = the number of replays) and moves the parameters as the same uncaptured streamed steps of a deep-copied
    model do — the same route, so rtol 1e-5 / atol 1e-6"""
    from two_stage_gnn_amd import message_passing as mp, sag_stream
    from two_stage_gnn_amd.data_parallel import FlatTrainer, GraphedStep
    anchors = ANCHORS[name]
    assert len(anchors) >= 5
    m1, datas, st1 = _stream(name, "train")
    m2 = copy.deepcopy(m1)
    start = {k: v.detach().clone() for k, v in m1.state_dict().items()}
    st2 = sag_stream.PostTrainStream(m2, datas)
    st2.load(anchors)
    tr2 = FlatTrainer(m2, lr=1e-3, clip=0)
    step2 = st2.step_loss()
    for i in anchors:
        tr2.step(step2)
        assert st2.ids_out.tolist() == [int(i)]
    st1.load(anchors)
    gs = GraphedStep(FlatTrainer(m1, lr=1e-3, clip=0), st1.step_loss())     # (its warm-up steps consume entries and are rolled back ...)
    assert gs.describe().startswith("one graph"), gs.describe()
    st1.load(anchors)                                                       # ... so the epoch starts here: cursor := 0
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
    assert moved >= 12


# ------------------------------------------------------------------------------------------------ 5. evaluation
@pytest.mark.parametrize("chunk", [1, 3, 7])
def test_test_dataset_equals_the_per_graph_loop(chunk):
    """the reference's ``test()`` in eval mode on a model left in train mode: the accuracy equals the per-graph loop's exactly
    (``model(data)`` on one graph at a time, arg-max against the label); the mean nll lies within 8 x the fp32 yardstick of the
    float64 value, both from the CPU oracle's B = 1 forwards (tests/fp32_yardstick.py's rule on one number: the fp32 oracle's own
    distance from the fp64 oracle, or 2^-23 of the value)"""
    from two_stage_gnn_amd import sag_stream
    m = U.net("small6", "train", 0.5)
    datas = _datas("small6")
    acc, nll = sag_stream.test_dataset(m, datas, chunk=chunk)
    assert m.training                                                         # (the mode was restored)
    m.eval()
    with torch.no_grad():
        rows = torch.cat([m(d) for d in datas]).cpu()
    m.train()
    y = torch.tensor(LABELS["small6"])
    assert acc == float((rows.argmax(dim=1) == y).sum()) / len(datas)
    ref = [_oracle("small6", i) for i in range(len(datas))]
    n64 = sum(-float(r[torch.float64][0][0, LABELS["small6"][i]]) for i, r in enumerate(ref)) / len(datas)
    n32 = float(sum(-r[torch.float32][0][0, LABELS["small6"][i]] for i, r in enumerate(ref)) / len(datas))
    yard = max(abs(n32 - n64), 2.0 ** -23 * abs(n64))
    print("test_dataset chunk %d: nll %.9g, fp64 oracle %.9g, fp32 oracle %.9g: %.3f x the yardstick" % (chunk, nll, n64, n32, abs(nll - n64) / yard))
    assert abs(nll - n64) <= 8 * yard, (nll, n64, n32)
    host = _datas("small6", on_device=False)
    assert sag_stream.test_dataset(m, host, chunk=chunk) == (acc, nll)         # labels on the host: the same numbers
    host[2].y = torch.tensor([8])
    with pytest.raises(ValueError, match="labels span"):
        sag_stream.test_dataset(m, host, chunk=chunk)


# ------------------------------------------------------------------------------------------------ 6. refusals
def test_constructor_load_and_mine_refuse(monkeypatch):
    from two_stage_gnn_amd import post_train as PT, sag_stream, sag_triplet
    datas = _datas("small6")
    for kw in ({"conv": "sage"}, {"fused": False}):
        with pytest.raises(TypeError, match="post_train_step"):
            sag_stream.PostTrainStream(U.net("small6", **kw), datas)
    with pytest.raises(TypeError, match="bare sag_layers.Net.*post_train_step"):
        sag_stream.PostTrainStream(sag_triplet.tripletnet(U.net("small6")), datas)       # the wrapper, not the model
    with pytest.raises(TypeError, match="GPU only.*post_train_step"):
        sag_stream.PostTrainStream(U.net("small6", dev="cpu"), datas)
    with monkeypatch.context() as mk:                                          # a head outside the fused launches' envelope
        mk.setattr(PT, "mlp3_nll_ok", lambda model, r: False)
        with pytest.raises(TypeError, match="head.*post_train_step"):
            sag_stream.PostTrainStream(U.net("small6"), datas)
    with pytest.raises(ValueError, match="graph 3: label 8 lies outside"):
        sag_stream.PostTrainStream(U.net("small6"), datas, labels=[0, 1, 2, 8, 4, 5])
    m, datas, st = _stream("small6", max_steps=4)
    assert len(st) == 1 and st.position() == 0 and st.labels.tolist() == LABELS["small6"]
    with pytest.raises(ValueError, match="exceeds"):
        st.load(ANCHORS["small6"])                                             # seven entries into a buffer of four
    assert st.load(ANCHORS["small6"][:4]) == 4 and st.load(ANCHORS["small6"][:3].reshape(3, 1)) == 3
    with pytest.raises(ValueError, match="indices"):
        st.load(np.array([0, 6]))
    with pytest.raises(RuntimeError, match="not a triplet"):
        st.mine(torch.zeros(6, 8, device="cuda"), None, 1.0)
    fresh = sag_stream.PostTrainStream(U.net("small6"), datas)
    with pytest.raises(RuntimeError, match="load"):
        fresh.step()
    m2, datas2, st2 = _stream("small6", max_steps=4)                            # the warm-up schedule serves a step: graph 0
    loss, out = st2.step()
    assert np.isfinite(float(loss)) and st2.ids_out.tolist() == [0]
