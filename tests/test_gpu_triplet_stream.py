"""The triplet stream on the GPU (two_stage_gnn_amd/triplet_stream.py, csrc/triplet_stream.hip): the gather launch word for word
against the existing collate -> pull -> expand route, replays that walk the schedule, one streamed step against the eager drop-in and
the CPU oracle's three B = 1 forwards, an epoch from one hipGraph, no host in the loop, and the launch's host validator.

Dataset and schedule: tests/triplet_stream_util.py (7 graphs, nmax 48; a full graph, a one-node graph, a CSR tail, an isolated node;
the schedule's entries shrink, repeat an object in two roles and repeat one object three times)."""
import copy

import numpy as np
import pytest
import torch

import triplet_stream_util as U
from oracle import dense_ref as R

pytestmark = pytest.mark.gpu

MARGIN, HID = 10.0, 128
POISON, GUARD, NGUARD = 12345, 777, 16


def _model(seed=6):
    from two_stage_gnn_amd import dense_encoders as E

    class A:
        bias = True
    torch.manual_seed(seed)
    m = E.GcnEncoderGraph(U.FIN, HID, HID, 2, 3, bn=True, args=A(), final_dim="output_dim")
    with torch.no_grad():
        for k, p in m.named_parameters():
            if "conv" in k and k.endswith("bias"):
                p.copy_(torch.randn_like(p) * 0.3)           # padded and ghost rows then carry values that can win the max readout
        m.map_model.weight.mul_(0.25)                        # distances of a few units: the margin-10 hinge is active for every entry
    return m.cuda()


def _stream(m, graphs):
    from two_stage_gnn_amd import triplet
    net = triplet.tripletnet(m)
    return net, triplet.TripletStream(net, graphs)


def _guarded(stream):
    """every output array of the gather launch re-pointed into a buffer of its own: poison in the array (a word the kernel does not
    write shows), guard words behind it.  -> {name: (buffer, words of the array)}"""
    dev, g, b = stream.device, stream.g, stream.batch
    bufs = {}

    def take(name, like):
        n = like.numel()
        if like.dtype == torch.float32:
            buf = torch.full((n + NGUARD,), float("nan"), dtype=torch.float32, device=dev)
            buf[n:] = float(GUARD)
        else:
            buf = torch.full((n + NGUARD,), POISON, dtype=torch.int32, device=dev)
            buf[n:] = GUARD
        bufs[name] = (buf, n)
        return buf[:n].view(like.shape)
    ell, w, (tail_ptr, tail_col) = g._ell
    g.graph_ptr, g.slot_count = take("graph_ptr", g.graph_ptr), take("slot_count", g.slot_count)
    g.row_graph, g.row_slot = take("row_graph", g.row_graph), take("row_slot", g.row_slot)
    b.tail_col = take("tail_col", tail_col)
    g._ell = (take("ell", ell), w, (take("tail_ptr", tail_ptr), b.tail_col))
    b.ell_slots, b.tail_slots = take("ell_slots", b.ell_slots), take("tail_slots", b.tail_slots)
    g._ell_slots = (b.ell_slots, b.tail_slots)
    stream.x = b.x = take("x", stream.x)
    stream.ids_out = take("ids_out", stream.ids_out)
    return bufs


def _tu_dataset(graphs):
    """the same graphs as a CSR-resident TU dataset (what the existing collate reads)"""
    from two_stage_gnn_amd.tu_data import TUDataset
    rec, per = U.restate(graphs)
    gp = np.concatenate([[0], np.cumsum(rec[:, 0])]).astype(np.int64)
    rowptr = np.concatenate([[0]] + [p[0][1:] + rec[i, 4] for i, p in enumerate(per)]).astype(np.int64)
    col = np.concatenate([p[1] + gp[i] for i, p in enumerate(per)]).astype(np.int64)
    n = int(gp[-1])
    return TUDataset(gp, rowptr, col, np.zeros(len(graphs), dtype=np.int64), np.zeros(n, dtype=np.int64), None, U.FIN), rec, per


@pytest.mark.parametrize("nmax", [48, 64])
def test_gather_equals_collate_pull_expand_word_for_word(nmax):
    """nmax 48: the largest graph fills every slot (ghost_slots = nmax); nmax 64: the same graphs with ghost slots to spare
    (ghost_slots = 49 < nmax, the benchmark's situation)"""
    from two_stage_gnn_amd import ingest
    graphs = U.dataset(nmax=nmax)
    net, st = _stream(_model(), graphs)
    ghost = min(nmax, 49)
    assert st.row_cap == 160 and st.arena.caps[0] == 3 * 48 and st.g.ghost_slots_fixed == ghost and st.tail_cap >= st.arena.caps[2] > 0
    assert st.arena.nmax == nmax and st.g.nmax == nmax
    bufs = _guarded(st)
    st.load(U.SCHEDULE)
    ds, rec, per = _tu_dataset(graphs)
    B, dev = 3, st.device
    ref = ingest.CapacityBatch(B, nmax, st.row_cap, int(3 * rec[:, 1].max()) + 8, U.FIN, dev, ghost_slots=ghost, tail_cap=st.tail_cap)
    R_ = st.row_cap + nmax
    feats = torch.from_numpy(st.arena.feats).to(dev)
    for k, ids in enumerate(U.SCHEDULE):
        st.gather()
        ref.collate(ds, ids)
        ref.pull()
        torch.cuda.synchronize()
        n, ntail = ref.rows, ref.tail
        assert n == rec[ids, 0].sum() and ntail == rec[ids, 2].sum() and (ntail > 0) == (0 in ids)
        rell, _, (rtp, rtc) = ref.g._ell
        sell, _, (stp, stc) = st.g._ell
        for name, got, want in (("graph_ptr", st.g.graph_ptr, ref.g.graph_ptr), ("slot_count", st.g.slot_count, ref.g.slot_count),
                                ("row_graph", st.g.row_graph, ref.g.row_graph), ("row_slot", st.g.row_slot, ref.g.row_slot),
                                ("ell", sell, rell), ("tail_ptr", stp, rtp), ("tail_col", stc[:ntail], rtc[:ntail]),
                                ("ell_slots", st.batch.ell_slots, ref.ell_slots), ("tail_slots", st.batch.tail_slots[:ntail], ref.tail_slots[:ntail])):
            assert got.shape == want.shape and torch.equal(got, want), (k, name, int((got != want).sum()))
        assert st.ids_out.tolist() == ids.tolist()
        # x: the arena's feature rows on the real rows, exactly zero everywhere else (no NaN left: every word was written)
        rows = torch.cat([torch.arange(int(rec[i, 3]), int(rec[i, 3] + rec[i, 0])) for i in ids]).to(dev)
        assert st.x.shape == (R_, 12) and torch.equal(st.x[:n], feats[rows]) and not bool(st.x[n:].ne(0).any())
        assert not bool(torch.isnan(st.x).any())
        for name, (buf, words) in bufs.items():
            want_guard = float(GUARD) if buf.dtype == torch.float32 else GUARD
            assert bool((buf[words:] == want_guard).all()), (k, name)
            if name not in ("tail_col", "tail_slots") and buf.dtype != torch.float32:
                assert not bool((buf[:words] == POISON).any()), (k, name)
        assert not bool((bufs["tail_col"][0][:ntail] == POISON).any()) and not bool((bufs["tail_slots"][0][:ntail] == POISON).any())
    assert st.position() == len(U.SCHEDULE)


def test_replays_walk_the_schedule_and_wrap():
    graphs = U.dataset()
    net, st = _stream(_model(), graphs)
    T = st.load(U.SCHEDULE)
    assert T == 5 and len(st) == 5 and st.position() == 0
    st.gather()                                                   # (library load and allocator warm-up outside the capture)
    torch.cuda.synchronize()
    assert st.position() == 1
    st.load(U.SCHEDULE)
    assert st.position() == 0                                     # load() resets the cursor
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        st.gather()
    assert st.position() == 0                                     # (capturing runs nothing)
    for k in range(T + 2):
        graph.replay()
        torch.cuda.synchronize()
        assert st.ids_out.tolist() == U.SCHEDULE[k % T].tolist(), k
    assert st.position() == T + 2
    st.load(U.SCHEDULE[::-1].copy()[:3])                          # a shorter schedule into the same buffer: the captured launch serves it
    assert st.position() == 0
    for k in range(4):
        graph.replay()
        torch.cuda.synchronize()
        assert st.ids_out.tolist() == U.SCHEDULE[::-1][k % 3].tolist(), k
    with pytest.raises(ValueError, match="exceeds"):
        st.load(np.zeros((T + 1, 3), dtype=np.int64))
    # a ticket counter that a launch cut short left behind: load() clears it with the schedule, and the cursor advances again
    st._sched[4] = 7
    st.load(U.SCHEDULE)
    assert int(st._sched[4]) == 0
    graph.replay()
    graph.replay()
    assert st.position() == 2 and int(st._sched[4]) == 0 and st.ids_out.tolist() == U.SCHEDULE[1].tolist()


def test_max_steps_sizes_the_buffer_before_the_first_schedule():
    from two_stage_gnn_amd import triplet
    graphs = U.dataset()
    st = triplet.TripletStream(triplet.tripletnet(_model()), graphs, max_steps=6)
    assert len(st) == 1 and st.position() == 0                    # the one-entry schedule [0, 0, 0]: enough for a warm-up
    st.gather()
    assert st.position() == 1 and st.ids_out.tolist() == [0, 0, 0]
    assert st.load(U.SCHEDULE) == 5 and st.position() == 0
    st.gather()
    assert st.position() == 1 and st.ids_out.tolist() == U.SCHEDULE[0].tolist()
    with pytest.raises(ValueError, match="exceeds"):
        st.load(np.zeros((7, 3), dtype=np.int64))


def _oracle_step(p_ref, graphs, ids):
    """the reference's step: three B = 1 forwards, distances, margin loss; -> (loss, dp, dn, embeds, grads)"""
    for v in p_ref.values():
        v.grad = None
    emb = []
    for i in ids:
        d = graphs[i].graph
        x, adj = torch.from_numpy(d["feats"])[None], torch.from_numpy(d["adj"])[None]
        emb.append(R.gcn_encoder(p_ref, x, adj, bn=True, final_dim="output_dim")[1])
    dp = torch.nn.functional.pairwise_distance(emb[0], emb[1], 2)
    dn = torch.nn.functional.pairwise_distance(emb[0], emb[2], 2)
    loss = torch.nn.MarginRankingLoss(margin=MARGIN)(dp, dn, torch.tensor([-1.0]))
    loss.backward()
    return loss.detach(), dp.detach(), dn.detach(), [e.detach() for e in emb], {k: v.grad for k, v in p_ref.items() if v.grad is not None}


@pytest.mark.parametrize("nmax", [48, 64])
def test_streamed_step_equals_the_drop_in_and_the_oracle(nmax):
    """every schedule entry, from the same parameters: loss and the five outputs of the streamed step against ``net(a, p, n)`` at
    rtol = atol = 1e-5, every parameter gradient at atol = 2e-5 * max|grad| (the largest entry of the step's whole gradient, as
    tests/test_tu_data.py:287-289 scales "the same graphs, capacity-padded against exact"), and against the CPU oracle's three
    B = 1 forwards at the tolerances of test_triplet_fused_stack_with_per_graph_statistics.  Gradients are compared from equal
    parameters, never after Adam.  Measured on an MI355X: the largest |stream - drop-in| gradient entry is 0 to 3.0e-8 per entry at
    bounds of 2.1e-5 to 3.3e-5 (max|grad| 1.06 to 1.67); for [1, 1, 1] the whole gradient is rounding (1e-8) and both routes give
    the same bits."""
    from two_stage_gnn_amd import _native as nat
    from two_stage_gnn_amd.triplet import MarginRankingLoss
    graphs = U.dataset(nmax=nmax)
    m = _model()
    net, st = _stream(m, graphs)
    assert st.g.ghost_slots_fixed == min(nmax, 49)
    st.load(U.SCHEDULE)
    crit, tgt = MarginRankingLoss(margin=MARGIN), torch.tensor([-1.0]).cuda()
    p_ref = {k: v.detach().cpu().clone().requires_grad_(True) for k, v in m.state_dict().items()}

    def grads_of():
        return {k: p.grad.detach().clone() for k, p in m.named_parameters() if p.grad is not None}

    for k, ids in enumerate(U.SCHEDULE):
        m.zero_grad(set_to_none=True)
        nat.trace = []
        outs = st.embed()
        loss = crit(outs[0], outs[1], tgt)
        loss.backward()
        names = [t[0] for t in nat.trace]
        nat.trace = None
        gs = grads_of()
        assert st.ids_out.tolist() == ids.tolist()
        assert "triplet_gather_f32" in names and "row_post_bwd_f32" in names and "row_maps" not in names, names
        m.zero_grad(set_to_none=True)
        outd = net(*[graphs[i] for i in ids])
        lossd = crit(outd[0], outd[1], tgt)
        lossd.backward()
        gd = grads_of()
        torch.testing.assert_close(loss.detach(), lossd.detach(), rtol=1e-5, atol=1e-5)
        for a, b in zip(outs, outd):
            torch.testing.assert_close(a.detach(), b.detach(), rtol=1e-5, atol=1e-5)
        assert gs.keys() == gd.keys() and len(gs) >= 8
        scale = max(float(v.abs().max()) for v in gd.values())
        worst = max(float((gs[n_] - gd[n_]).abs().max()) for n_ in gd)
        print("entry %d %s: loss %.6f, max|grad| %.3e, max|stream - drop-in| %.3e (bound %.3e)" % (k, ids.tolist(), float(loss.detach()), scale, worst,
                                                                                                  2e-5 * scale))
        for n_ in gd:
            err = float((gs[n_] - gd[n_]).abs().max())
            assert err <= 2e-5 * scale, (k, n_, err, scale)
        # the oracle
        lo, dpo, dno, embo, go = _oracle_step(p_ref, graphs, ids)
        assert float(dpo - dno) + MARGIN > 0                       # the hinge is active
        torch.testing.assert_close(outs[0].detach().cpu(), dpo, rtol=1e-4, atol=1e-4)
        torch.testing.assert_close(outs[1].detach().cpu(), dno, rtol=1e-4, atol=1e-4)
        for a, b in zip(outs[2:], embo):
            torch.testing.assert_close(a.detach().cpu(), b, rtol=1e-4, atol=1e-4)
        assert set(go) == set(gs) and len(go) >= 8                 # every gradient of the step is compared, none skipped
        for n_, ref in go.items():
            err = float((gs[n_].cpu() - ref).abs().max())
            assert err <= 2e-3 * float(ref.abs().max()) + 1e-6, (k, n_, err, float(ref.abs().max()))


def test_an_epoch_from_one_hipgraph_equals_eager_steps():
    from two_stage_gnn_amd import _native as nat
    from two_stage_gnn_amd.data_parallel import FlatTrainer, GraphedStep
    from two_stage_gnn_amd.triplet import MarginRankingLoss, tripletnet
    graphs = U.dataset()
    m1 = _model()
    m2 = copy.deepcopy(m1)
    T, lr = len(U.SCHEDULE), 1e-3
    crit, tgt = MarginRankingLoss(margin=MARGIN), torch.tensor([-1.0]).cuda()
    # eager: the drop-in fed the same objects in the same order
    net2, tr2 = tripletnet(m2), FlatTrainer(m2, lr=lr, clip=2.0)
    eager = []
    for ids in U.SCHEDULE:
        tr2.zero_grad()
        out = net2(*[graphs[i] for i in ids])
        loss = crit(out[0], out[1], tgt)
        tr2.backward(loss)
        tr2.gather_grads()
        tr2.apply()
        eager.append(float(loss.detach()))
    # streamed: one hipGraph, T replays
    net1, st = _stream(m1, graphs)
    st.load(U.SCHEDULE)
    tr1 = FlatTrainer(m1, lr=lr, clip=2.0)
    gs = GraphedStep(tr1, st.loss(crit, tgt))                                   # (its warm-up steps consume entries ...)
    st.load(U.SCHEDULE)                                                         # ... so the epoch starts here: cursor := 0
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
    nat.trace = []
    try:
        tr1.zero_grad()
        tr1.backward(st.loss(crit, tgt)())
        names = [t[0] for t in nat.trace]
    finally:
        nat.trace = None
    assert all(w in names for w in ("triplet_gather_f32", "row_ln_fwd_f32", "row_post_bwd_f32")), names
    assert "ell_spmm_f32" not in names and "row_maps" not in names, names


def test_no_host_in_the_loop():
    from two_stage_gnn_amd.data_parallel import FlatTrainer, GraphedStep
    from two_stage_gnn_amd.triplet import MarginRankingLoss
    graphs = U.dataset()
    m = _model()
    net, st = _stream(m, graphs)
    st.load(U.SCHEDULE)
    crit, tgt = MarginRankingLoss(margin=MARGIN), torch.tensor([-1.0]).cuda()
    gs = GraphedStep(FlatTrainer(m, lr=1e-3, clip=2.0), st.loss(crit, tgt))
    st.load(U.SCHEDULE)
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
    gs.synchronize()                                              # (the replays run on the step's own stream)
    assert st.position() == T + 1 and np.isfinite(gs.loss_value())


def test_validator_refuses_without_a_launch():
    from two_stage_gnn_amd import _native as nat
    graphs = U.dataset()
    net, st = _stream(_model(), graphs)
    st.load(U.SCHEDULE)
    ar, g, b = st.arena, st.g, st.batch
    ell, ell_w, (tail_ptr, tail_col) = g._ell
    good = [st.records, ar.n_graphs, st.buf, ar.off["rowptr"], ar.off["col"], ar.off["tail_ptr"], ar.off["tail_col"], ar.words, st.feats,
            ar.ld, ar.caps[0], ar.caps[2], st._sched[8:], st.max_steps, st._sched, st._sched[4:8], 3, ar.nmax, st.row_cap, st.tail_cap, ell_w,
            g.graph_ptr, g.slot_count, g.row_graph, g.row_slot, ell, tail_ptr, tail_col, b.ell_slots, b.tail_slots, st.x, st.x.stride(0),
            st.ids_out]
    PTRS = (0, 2, 8, 12, 14, 15, 21, 22, 23, 24, 25, 26, 27, 30, 32)
    odd = lambda t: t.view(-1)[1:]                                # 4 bytes off a 16-byte boundary
    cases = [("null %d" % i, i, None) for i in PTRS]
    cases += [("ell_slots without tail_slots", 29, None), ("B = 0", 16, 0), ("B = 9", 16, 9), ("row_cap below the arena's bound", 18, ar.caps[0] - 1),
              ("tail_cap below the arena's bound", 19, ar.caps[2] - 1), ("no schedule", 13, 0), ("ell_w", 20, 12),
              ("misaligned records", 0, odd(st.records)), ("misaligned arena", 2, odd(st.buf)), ("misaligned feats", 8, odd(st.feats)),
              ("misaligned ell", 25, odd(ell)), ("misaligned ell_slots", 28, odd(b.ell_slots)), ("misaligned x", 30, odd(st.x)),
              ("misaligned state", 14, st._sched[2:]), ("section offset off 16 bytes", 4, ar.off["col"] + 1),
              ("ldx != ldf", 31, st.x.stride(0) + 4)]
    torch.cuda.synchronize()
    before = st.position()
    nat.trace = []
    try:
        for what, i, v in cases:
            args = list(good)
            args[i] = v
            with pytest.raises(RuntimeError, match="triplet_gather_f32 failed"):
                nat.call("triplet_gather_f32", *args)
        assert nat.trace == []                                    # nothing was launched
        nat.call("triplet_gather_f32", *good)
        assert len(nat.trace) == 1 and nat.trace[0][2].startswith("triplet_gather_kernel")
    finally:
        nat.trace = None
    torch.cuda.synchronize()
    assert st.position() == before + 1


def test_constructor_refuses_other_models():
    from two_stage_gnn_amd import dense_encoders as E
    from two_stage_gnn_amd import triplet

    class A:
        bias = True
    graphs = U.dataset()
    m = E.GcnEncoderGraph(U.FIN, HID, HID, 2, 3, bn=False, args=A(), final_dim="output_dim").cuda()
    with pytest.raises(TypeError, match="eager drop-in"):
        triplet.TripletStream(triplet.tripletnet(m), graphs)
    sp = E.SoftPoolingGcnEncoder(U.NMAX, U.FIN, 32, 32, 2, 3, 32, assign_ratio=0.25, num_pooling=1, bn=True, args=A(),
                                 assign_input_dim=U.FIN, final_dim="output_dim").cuda()
    with pytest.raises(TypeError, match="eager drop-in"):
        triplet.TripletStream(triplet.tripletnet(sp), graphs)


def test_a_schedule_word_past_n_graphs_is_clamped_into_the_records():
    """the raw entry point told that the table holds G - 2 records (it holds G): schedule words G - 1 and G - 2 — outside the launch's
    range, inside the allocation — must give, word for word in every output array and in ids_out, what the same schedule with every
    index replaced by min(index, G - 3) gives (csrc/stream_protocol.h, stream_entry_id)"""
    from two_stage_gnn_amd import _native as nat
    graphs = U.dataset()
    net, st = _stream(_model(), graphs)
    G = len(graphs)
    sched = np.asarray([[G - 1, 1, G - 2], [0, G - 2, G - 1], [G - 1, G - 1, 2], [3, G - 3, G - 2]], dtype=np.int64)
    ar, g, b = st.arena, st.g, st.batch
    ell, ell_w, (tail_ptr, tail_col) = g._ell
    outs = {"graph_ptr": g.graph_ptr, "slot_count": g.slot_count, "row_graph": g.row_graph, "row_slot": g.row_slot, "ell": ell,
            "tail_ptr": tail_ptr, "tail_col": tail_col, "ell_slots": b.ell_slots, "tail_slots": b.tail_slots, "x": st.x, "ids_out": st.ids_out}

    def run(schedule):
        st.load(schedule)
        got = []
        for _ in range(len(schedule)):
            for t in outs.values():
                t.view(torch.int32).fill_(POISON)                 # (words a launch does not write: the same in both passes)
            nat.call("triplet_gather_f32", st.records, G - 2, st.buf, ar.off["rowptr"], ar.off["col"], ar.off["tail_ptr"],
                     ar.off["tail_col"], ar.words, st.feats, ar.ld, ar.caps[0], ar.caps[2], st._sched[8:], st.max_steps, st._sched,
                     st._sched[4:8], 3, ar.nmax, st.row_cap, st.tail_cap, ell_w, g.graph_ptr, g.slot_count, g.row_graph, g.row_slot, ell,
                     tail_ptr, tail_col, b.ell_slots, b.tail_slots, st.x, st.x.stride(0), st.ids_out)
            torch.cuda.synchronize()
            got.append({k: t.view(torch.int32).clone() for k, t in outs.items()})
        assert st.position() == len(schedule)
        return got

    want_ids = np.minimum(sched, G - 3)
    stale, clamped = run(sched), run(want_ids)
    for k in range(len(sched)):
        assert clamped[k]["ids_out"].tolist() == want_ids[k].tolist()
        for name in outs:
            assert torch.equal(stale[k][name], clamped[k][name]), (k, name, int((stale[k][name] != clamped[k][name]).sum()))
