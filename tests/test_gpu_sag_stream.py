"""The SAGPool triplet stream on the GPU (two_stage_gnn_amd/sag_stream.py, csrc/sag_stream.hip, the capacity forms of the per-graph level
kernels): the gather launch alone against ``tripletnet.batch()`` + ``SagPlan`` for every schedule entry, one streamed step per entry
against the eager drop-in and the fp64 oracle's three B = 1 forwards, the same steps on poisoned allocator memory, the launch trace of
a step, no host in the loop, an epoch walked by replays of one hipGraph, and the constructor's refusals.

Datasets, schedules and the oracle: tests/sag_stream_util.py (margin 1.5 keeps the hinge active in every entry).  Tolerances are those
of tests/test_gpu_sag_triplet.py for the same node against the same oracle: rtol = atol = 1e-5 on outputs (distances: or 10 x the fp32
CPU oracle's own error), gradients 1e-4 of the tensor's largest entry or 10 x the fp32 oracle's own error."""
import copy

import numpy as np
import pytest
import torch

import sag_stream_util as U
from guard_buf import GUARD, PAT
from test_gpu_sag_triplet import _bound

pytestmark = pytest.mark.gpu

IPAT = -1


def _stream(name, mode="eval", p_drop=0.0, **kw):
    from two_stage_gnn_amd import sag_stream, sag_triplet
    fin, nhid, C, graphs = U.dataset(name)
    m = U.net(name, mode, p_drop)
    net = sag_triplet.tripletnet(m)
    datas = U.datas(graphs)
    return m, net, datas, sag_stream.TripletStream(net, datas, **kw)


def _crit():
    from two_stage_gnn_amd.sag_triplet import MarginRankingLoss
    return MarginRankingLoss(margin=U.MARGIN), torch.full((1,), -1.0, device="cuda")


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


# ------------------------------------------------------------------------------------------------ 2. the gather launch alone
class _Guarded:
    """n words on the device prefilled with one pattern (a NaN for float32, -1 for int32), GUARD words of it behind"""

    def __init__(self, n, dtype):
        self.n, self.pat = n, PAT if dtype == torch.float32 else IPAT
        self.bits = torch.full((n + GUARD,), self.pat, dtype=torch.int32, device="cuda")
        self.t = self.bits[:n].view(dtype)

    def get(self, what):
        torch.cuda.synchronize()
        b = self.bits.cpu()
        assert bool((b[self.n:] == self.pat).all()), "%s: guard words overwritten" % what
        return b[:self.n]


def _gather(st, ratio):
    """the stream's gather launch into guarded buffers of the stream's capacities -> {name: int32 bit view on the CPU}"""
    from two_stage_gnn_amd import _native as nat
    from two_stage_gnn_amd.triplet_stream import HEAD
    ar, R, depth = st.arena, st.row_cap, st.plan.depth
    B = {"rowptr": _Guarded(R + 1, torch.int32), "col": _Guarded(st.nnz_cap, torch.int32), "x": _Guarded(R * ar.ld, torch.float32),
         "dinv": _Guarded(R, torch.float32), "self_w": _Guarded(R, torch.float32), "gp": _Guarded(4 * (depth + 1), torch.int32),
         "ids": _Guarded(3, torch.int32)}
    nat.call("sag_triplet_gather_f32", st.records, ar.n_graphs, st.buf, ar.off["rowptr"], ar.off["col"], ar.words, st.feats, ar.ld,
             ar.caps[0], ar.caps[1], st._sched[HEAD:], st.max_steps, st._sched, st._sched[4:HEAD], R, st.nnz_cap, float(ratio), depth,
             B["rowptr"].t, B["col"].t, B["x"].t, ar.ld, B["dinv"].t, B["self_w"].t, B["gp"].t, B["ids"].t)
    return {k: v.get(k) for k, v in B.items()}


@pytest.mark.parametrize("name", ["small6", "dd3"])
def test_gather_launch_equals_batch_and_sagplan_for_every_entry(name):
    """every array the launch writes against ``tripletnet.batch()``, ``gcn_coef`` and ``SagPlan.get`` on the same three objects: bit
    for bit; padding as specified (empty rows, +0 features and coefficients, columns past the batch's nnz not touched); guards intact;
    ``ids_out`` and ``position()``.  Ratio 0.3 (where float32 and float64 disagree on ceil) for the graph pointers as well."""
    from two_stage_gnn_amd.sag_stack import SagPlan, gcn_coef
    m, net, datas, st = _stream(name)
    sched = U.SCHEDULES[name]
    st.load(sched)
    ar, R, fin = st.arena, st.row_cap, st.arena.fin
    assert R == 3 * max(U.SIZES[name]) and st.nnz_cap >= 1
    calls = 0
    for ratio in (U.RATIO, 0.3):
        st.load(sched)
        for k, ids in enumerate(sched):
            got = _gather(st, ratio)
            calls += 1
            assert st.position() == k + 1
            b = net.batch(*[datas[i] for i in ids])
            n_tot, nnz = int(b.g.n_rows), int(b.g.nnz)
            assert got["ids"].tolist() == ids.tolist()
            rp = got["rowptr"]
            assert torch.equal(rp[:n_tot + 1], b.g.rowptr.cpu()) and bool((rp[n_tot:] == nnz).all()), (k, "rowptr")
            assert torch.equal(got["col"][:nnz], b.g.col.cpu()[:nnz]) and bool((got["col"][nnz:] == IPAT).all()), (k, "col")
            x = got["x"].view(R, ar.ld)
            assert torch.equal(x[:n_tot, :fin], _bits(b.x)) and not bool(x[:n_tot, fin:].any()) and not bool(x[n_tot:].any()), (k, "x")
            dinv, self_w = gcn_coef(b.g)
            for what, want in (("dinv", dinv), ("self_w", self_w)):
                assert torch.equal(got[what][:n_tot], _bits(want)) and not bool(got[what][n_tot:].any()), (k, what)
            plan = SagPlan.get(b.sizes, ratio, b.x.device, depth=3)
            gp = got["gp"].view(4, 4)
            for l in range(4):
                assert gp[l].tolist() == plan.levels[l].gp.cpu().tolist(), (k, ratio, l)
    assert calls == 10
    if name == "small6":
        assert (np.diff(np.array(U.SIZES[name])[sched].sum(1))[:1] < 0).all()         # the second entry is smaller: stale rows would show


# ------------------------------------------------------------------------------------------------ 4. the streamed step
def _grads(m):
    return {k: p.grad.detach().clone() for k, p in m.named_parameters() if p.grad is not None}


def _streamed_entry(m, st, crit, tgt):
    m.zero_grad(set_to_none=True)
    outs = st.embed()
    loss = crit(outs[0], outs[1], tgt)
    loss.backward()
    return outs, loss.detach(), _grads(m)


def _check_vs_oracle(name, k, ids, outs, loss, gs, skipped):
    ref = U.oracle(name, ids)
    (dp64, dn64, e64, l64, g64), (dp32, dn32, e32, l32, g32) = ref[torch.float64], ref[torch.float32]
    assert l64 > 0.0                                          # the hinge is active
    for what, got, r64, r32 in (("embed_a", outs[2], e64[0], e32[0]), ("embed_p", outs[3], e64[1], e32[1]),
                                ("embed_n", outs[4], e64[2], e32[2]), ("dist_p", outs[0], dp64, dp32), ("dist_n", outs[1], dn64, dn32)):
        diff = (got.detach().cpu().double() - r64).abs()
        err, e_cpu = float(diff.max()), float((r32.double() - r64).abs().max())
        print("%s entry %d %s: |hip - fp64| %.2e, |cpu fp32 - fp64| %.2e" % (name, k, what, err, e_cpu))
        within = bool((diff <= 1e-5 + 1e-5 * r64.abs()).all())
        if what.startswith("dist"):
            within = within or err <= 10.0 * e_cpu
        assert within, (k, what, err, e_cpu)
    assert abs(float(loss) - l64) <= max(1e-5 * max(1.0, abs(l64)), 10 * abs(l32 - l64))
    if len(set(ids.tolist())) == 1:                           # a = p = n: d_p - d_n is identically zero, the gradient pure rounding
        skipped.append(ids.tolist())
        return
    assert set(gs) == set(g64) and len(gs) == 18
    for key, r64 in g64.items():
        err = float((gs[key].cpu().double() - r64).abs().max())
        bound, e_cpu = _bound(r64, g32[key], 1e-4, 1e-9)
        assert err <= bound, (k, key, err, e_cpu, float(r64.abs().max()))


@pytest.mark.parametrize("mode", ["eval", "train"])
@pytest.mark.parametrize("name", ["small6", "dd3"])
def test_streamed_step_equals_the_drop_in_and_the_oracle(name, mode):
    """every schedule entry from equal parameters (eval mode; training mode with dropout_ratio 0): against ``net(a, p, n)`` distances and
    embeddings at rtol = atol = 1e-5 (the largest gradient difference is printed), against the oracle at the bounds of
    test_step_vs_three_single_graph_oracle_calls.
    Measured on an MI355X (profiles/r16/sag_stream.txt keeps the lines this test prints): small6 gives the drop-in's gradients bit for
    bit (the narrow level 0 and 32-wide levels sum a row in the same order at any row count); dd3 differs by 1.9e-9 to 4.2e-7 at
    max|grad| 1.8 to 2.8 (the slab plan of the weight gradients depends on the row count, here the capacity); embeddings lie within
    5.2e-7 of the fp64 oracle, whose own fp32 run misses by 4.0e-7."""
    m, net, datas, st = _stream(name, mode)
    sched = U.SCHEDULES[name]
    st.load(sched)
    crit, tgt = _crit()
    skipped = []
    for k, ids in enumerate(sched):
        outs, loss, gs = _streamed_entry(m, st, crit, tgt)
        assert st.ids_out.tolist() == ids.tolist()
        m.zero_grad(set_to_none=True)
        outd = net(*[datas[i] for i in ids])
        crit(outd[0], outd[1], tgt).backward()
        gd = _grads(m)
        for a, b in zip(outs, outd):
            assert a.shape == b.shape
            torch.testing.assert_close(a, b, rtol=1e-5, atol=1e-5)
        worst = max(float((gs[n_] - gd[n_]).abs().max()) for n_ in gd)
        print("%s %s entry %d %s: max|grad| %.3e, max|streamed - drop-in| gradient entry %.3e"
              % (name, mode, k, ids.tolist(), max(float(v.abs().max()) for v in gd.values()), worst))
        _check_vs_oracle(name, k, ids, outs, loss, gs, skipped)
    assert len(skipped) == 1 and st.position() == len(sched)


def test_dropout_stays_in_the_tail_kernel():
    """p = 0.5 in training mode: the step still launches mlp3_triplet_fwd_f32 (the mask's counter lives on the device) and every loss
    is finite"""
    from two_stage_gnn_amd import _native as nat
    m, net, datas, st = _stream("small6", "train", 0.5)
    st.load(U.SCHEDULES["small6"])
    crit, tgt = _crit()
    losses = []
    nat.trace = []
    try:
        for _ in U.SCHEDULES["small6"]:
            losses.append(_streamed_entry(m, st, crit, tgt)[1])
        names = [t[0] for t in nat.trace]
    finally:
        nat.trace = None
    assert names.count("mlp3_triplet_fwd_f32") == 5 and names.count("mlp3_triplet_bwd_f32") == 5
    assert all(np.isfinite(float(l)) for l in losses)
    assert all(bool(torch.isfinite(p.grad).all()) for p in m.parameters())


# ------------------------------------------------------------------------------------------------ 5. poisoned padding
def _poison(nbytes):
    """fill the caching allocator's free memory with NaN: allocate, fill and free tensors of the step's sizes (the allocator hands
    the same blocks to the next step's torch.empty calls)"""
    ts = [torch.empty(max(n // 4, 1), dtype=torch.float32, device="cuda") for n in nbytes for _ in range(3)]
    for t in ts:
        t.fill_(float("nan"))
    torch.cuda.synchronize()
    del ts


@pytest.mark.parametrize("name", ["small6", "dd3"])
def test_poisoned_padding_changes_nothing(name):
    """torch.empty hands the node memory that holds NaN: loss and every gradient are finite and equal the unpoisoned step's (the
    kernels are the same and sum in a fixed order: rtol 1e-6 / atol 1e-7, what the project allows two runs of one route).  A
    padding row that nobody zeroes would put 0 * NaN into the weight-gradient slabs"""
    from two_stage_gnn_amd import _native as nat
    m, net, datas, st = _stream(name, "train")
    sched = U.SCHEDULES[name]
    crit, tgt = _crit()
    st.load(sched)
    nat.trace = []
    try:
        clean = [_streamed_entry(m, st, crit, tgt) for _ in sched]
        sizes = sorted({a.untyped_storage().nbytes() for t in nat.trace for a in t[1] if isinstance(a, torch.Tensor)})
    finally:
        nat.trace = None
    assert len(sizes) > 8
    st.load(sched)
    for k, ids in enumerate(sched):
        outs = loss = gs = None
        _poison(sizes)
        outs, loss, gs = _streamed_entry(m, st, crit, tgt)
        assert np.isfinite(float(loss)) and all(bool(torch.isfinite(g).all()) for g in gs.values()), (k, ids.tolist())
        torch.testing.assert_close(loss, clean[k][1], rtol=1e-6, atol=1e-7)
        assert set(gs) == set(clean[k][2])
        for key, g in gs.items():
            torch.testing.assert_close(g, clean[k][2][key], rtol=1e-6, atol=1e-7, msg=lambda s_, key=key: "%s entry %d: %s" % (key, k, s_))


# ------------------------------------------------------------------------------------------------ 6. the launch trace
@pytest.mark.parametrize("name", ["small6", "dd3"])
def test_launch_trace_of_a_streamed_step(name):
    from two_stage_gnn_amd import _native as nat
    m, net, datas, st = _stream(name, "train")
    st.load(U.SCHEDULES[name])
    crit, tgt = _crit()
    st.loss(crit, tgt)().backward()                               # (warm: allocator, library load)
    m.zero_grad(set_to_none=True)
    nat.trace = []
    try:
        st.loss(crit, tgt)().backward()
        names = [t[0] for t in nat.trace]
    finally:
        nat.trace = None
    print("library launches of a streamed SAGPool step (%s): %d\n%s" % (name, len(names), " ".join(names)))
    assert names[0] == "sag_triplet_gather_f32" and names.count("sag_triplet_gather_f32") == 1
    assert names.count("sag_pool_graph_cap_f32") == 3 and names.count("sag_pool_graph_bwd_cap_f32") == 3
    assert not [n for n in names if n in ("gcn_coef_f32", "row_maps", "scan_short_i32", "csr_filter_fill", "sag_pool_graph_f32",
                                          "sag_pool_graph_bwd_f32")]
    assert names.count("mlp3_triplet_fwd_f32") == 1 and names.count("mlp3_triplet_bwd_f32") == 1
    if name == "small6":
        assert names.count("gcn_propagate_affine_f32") == 1 and "gcn_propagate_re_f32" not in names
    else:
        assert names.count("gcn_propagate_re_f32") == 1 and names.count("gat_bwd_products_f32") == 2      # levels 1 and 2: merged


# ------------------------------------------------------------------------------------------------ 7. no host in the loop
def test_no_host_in_the_loop():
    """after one warm call, forward + backward of two streamed steps under sync debug mode "error" """
    m, net, datas, st = _stream("small6", "train")
    st.load(U.SCHEDULES["small6"])
    crit, tgt = _crit()
    step = st.loss(crit, tgt)
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
    assert all(bool(torch.isfinite(p.grad).all()) for p in m.parameters() if p.grad is not None)


# ------------------------------------------------------------------------------------------------ 8. replays
@pytest.mark.parametrize("name", ["small6", "dd3"])
def test_replays_walk_the_schedule_and_move_the_parameters_as_uncaptured_steps(name):
    """``GraphedStep(FlatTrainer(...), st.loss(...))``: five replays walk the schedule (``ids_out`` per replay, ``position() == 5``) and
    move the parameters as five uncaptured streamed steps of a deep-copied model do — the same route, so rtol 1e-5 / atol 1e-6"""
    from two_stage_gnn_amd import message_passing as mp, sag_stream, sag_triplet
    from two_stage_gnn_amd.data_parallel import FlatTrainer, GraphedStep
    sched = U.SCHEDULES[name]
    m1, net1, datas, st1 = _stream(name, "train")
    m2 = copy.deepcopy(m1)
    start = {k: v.detach().clone() for k, v in m1.state_dict().items()}
    crit, tgt = _crit()
    st2 = sag_stream.TripletStream(sag_triplet.tripletnet(m2), datas)
    st2.load(sched)
    tr2 = FlatTrainer(m2, lr=1e-3, clip=2.0)
    step2 = st2.loss(crit, tgt)
    for ids in sched:
        tr2.step(step2)
        assert st2.ids_out.tolist() == ids.tolist()
    st1.load(sched)
    gs = GraphedStep(FlatTrainer(m1, lr=1e-3, clip=2.0), st1.loss(crit, tgt))   # (its warm-up steps consume entries and are rolled back ...)
    assert gs.describe().startswith("one graph"), gs.describe()
    st1.load(sched)                                                             # ... so the epoch starts here: cursor := 0
    for ids in sched:
        gs.step()
        gs.synchronize()
        assert st1.ids_out.tolist() == ids.tolist()
    assert st1.position() == len(sched) == 5 and np.isfinite(gs.loss_value())
    mp.check_device_errors()
    moved = 0
    for (k, p1), (_, p2) in zip(m1.named_parameters(), m2.named_parameters()):
        torch.testing.assert_close(p1.detach(), p2.detach(), rtol=1e-5, atol=1e-6, msg=lambda s_, k=k: k + ": " + s_)
        moved += int(not torch.equal(p1.detach(), start[k]))
    assert moved >= 12


# ------------------------------------------------------------------------------------------------ 9. refusals
def test_constructor_and_load_refuse(monkeypatch):
    from two_stage_gnn_amd import sag_stream, sag_triplet, triplet
    fin, nhid, C, graphs = U.dataset("small6")
    datas = U.datas(graphs)
    for kw in ({"conv": "sage"}, {"fused": False}):
        with pytest.raises(TypeError, match="eager drop-in"):
            sag_stream.TripletStream(sag_triplet.tripletnet(U.net("small6", **kw)), datas)
    with pytest.raises(TypeError, match="GPU only.*eager drop-in"):
        sag_stream.TripletStream(sag_triplet.tripletnet(U.net("small6", dev="cpu")), datas)
    with pytest.raises(TypeError, match="eager drop-in"):
        sag_stream.TripletStream(object(), datas)
    with monkeypatch.context() as mk:                              # a head the tail kernel does not take (TSGNN_TRIPLET_TAIL=0)
        mk.setattr(triplet, "FUSED_TAIL", False)
        with pytest.raises(TypeError, match="head.*eager drop-in"):
            sag_stream.TripletStream(sag_triplet.tripletnet(U.net("small6")), datas)
    m, net, datas, st = _stream("small6", max_steps=4)
    assert len(st) == 1 and st.position() == 0
    with pytest.raises(ValueError, match="exceeds"):
        st.load(U.SCHEDULES["small6"])                             # five entries into a buffer of four
    assert st.load(U.SCHEDULES["small6"][:4]) == 4
    with pytest.raises(ValueError, match="indices"):
        st.load(np.array([[0, 1, 6]]))
    # the warm-up schedule serves a step: graph 0 three times
    crit, tgt = _crit()
    m2, net2, datas2, st2 = _stream("small6", max_steps=4)
    assert np.isfinite(float(st2.loss(crit, tgt)())) and st2.ids_out.tolist() == [0, 0, 0]
