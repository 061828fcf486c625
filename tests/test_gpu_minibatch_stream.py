"""The mini-batch stream on the GPU (two_stage_gnn_amd/minibatch_stream.py, csrc/batch_stream.hip): the gather launch word for word
against collate -> pull -> expand, against a numpy restatement and (B <= 8) against the triplet gather; the one-hot feature mode;
the cursor; one streamed step against the exact batch and the CPU oracle; an epoch from one hipGraph; no host in the loop; the launch
trace; poisoned capacity; the constructor's refusals.

Dataset and schedules: tests/minibatch_stream_util.py (24 graphs, nmax 48 / 64, fin 9; a full graph, a one-node graph, a CSR tail, an
isolated node, three classes; per batch size a schedule whose first entry fills the slot exactly)."""
import copy

import numpy as np
import pytest
import torch

import minibatch_stream_util as U
from oracle import dense_ref as R

pytestmark = pytest.mark.gpu

HID = 128
POISON, GUARD, NGUARD = 12345, 777, 16


def _model(seed=6, final_dim="number_classes", bn=True, concat=True, fin=U.FIN):
    from two_stage_gnn_amd import dense_encoders as E

    class A:
        bias = True
    torch.manual_seed(seed)
    m = E.GcnEncoderGraph(fin, HID, HID, U.N_CLASSES, 3, concat=concat, bn=bn, args=A(), final_dim=final_dim)
    with torch.no_grad():
        for k, p in m.named_parameters():
            if "conv" in k and k.endswith("bias"):
                p.copy_(torch.randn_like(p) * 0.3)           # padded and ghost rows then carry values that can win the max readout
    return m.cuda()


_cache = {}


def _data(nmax=U.NMAX, onehot=False):
    """graph objects and the same graphs as a TU dataset, built once per variant and left unchanged"""
    key = (nmax, onehot)
    if key not in _cache:
        graphs = U.dataset(nmax=nmax, onehot=onehot)
        _cache[key] = (graphs, U.tu_dataset(graphs))
    return _cache[key]


def _exact(st, row_cap, tail_cap):
    """the stream's slot rebuilt at EXACTLY these capacities (the constructor rounds row_cap up to 32; the launch takes any)"""
    from two_stage_gnn_amd import ingest
    ar = st.arena
    st.row_cap, st.tail_cap = int(row_cap), int(tail_cap)
    st.batch = ingest.CapacityBatch(st.B, ar.nmax, st.row_cap, 4, ar.fin, st.device, ghost_slots=min(ar.nmax, ar.largest + 1),
                                    tail_cap=st.tail_cap)
    st.g, st.x, st.label = st.batch.g, st.batch.x, st.batch.label


def _stream(m, B, nmax=U.NMAX, onehot=False, features="table", exact=True, tu=False, **kw):
    """-> (stream, schedule, graphs, ds); the slot at the plan's exact capacities unless ``exact`` is False"""
    from two_stage_gnn_amd import minibatch_stream as MS
    graphs, ds = _data(nmax, onehot)
    sched, row_cap, tail_cap = U.plan(B, graphs)
    U.check_plan(B, sched, row_cap, graphs)
    st = MS.MiniBatchStream(m, ds if tu else graphs, B, nmax=nmax, row_cap=row_cap, tail_cap=tail_cap, features=features, **kw)
    assert st.row_cap == (row_cap + 31) // 32 * 32 and st.tail_cap == tail_cap
    if exact:
        _exact(st, row_cap, tail_cap)
    return st, sched, graphs, ds


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
            buf = torch.full((n + NGUARD,), POISON, dtype=like.dtype, device=dev)
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
    stream.label = b.label = take("label", stream.label)
    return bufs


def _bits(bufs):
    return {k: v[0].clone() for k, v in bufs.items()}


def _same_bits(a, b):
    return all(torch.equal(a[k].view(torch.int32) if a[k].dtype == torch.float32 else a[k],
                           b[k].view(torch.int32) if b[k].dtype == torch.float32 else b[k]) for k in a)


def _outputs(st, ntail):
    sell, _, (stp, stc) = st.g._ell
    return {"graph_ptr": st.g.graph_ptr, "slot_count": st.g.slot_count, "row_graph": st.g.row_graph, "row_slot": st.g.row_slot,
            "ell": sell, "tail_ptr": stp, "tail_col": stc[:ntail], "ell_slots": st.batch.ell_slots, "tail_slots": st.batch.tail_slots[:ntail]}


# ------------------------------------------------------------------------------------------------ 1. the gather launch alone
@pytest.mark.parametrize("nmax", [48, 64])
@pytest.mark.parametrize("B", U.BATCHES)
def test_gather_equals_collate_pull_expand_and_the_restatement_word_for_word(B, nmax):
    """nmax 48: graph 0 fills every slot (ghost_slots = nmax); nmax 64: ghost slots to spare.  The slot's row_cap is the first
    entry's row count exactly (no multiple of 8 or 32 in general).  Every entry is launched twice in a row."""
    from two_stage_gnn_amd import _native as nat
    from two_stage_gnn_amd import ingest
    from two_stage_gnn_amd.triplet_stream import HEAD
    st, sched, graphs, ds = _stream(_model(), B, nmax)
    row_cap, tail_cap, dev = st.row_cap, st.tail_cap, st.device
    ghost = min(nmax, 49)
    assert st.g.ghost_slots_fixed == ghost and st.arena.nmax == nmax and st.g.nmax == nmax and row_cap == sum(U.SIZES[i] for i in sched[0])
    assert row_cap < B * 48 or B == 1                              # below the arena's bound (B times the largest graph)
    bufs = _guarded(st)
    twice = np.repeat(sched, 2, axis=0)
    st.load(twice)
    rec = st.arena.records.astype(np.int64)
    ref = ingest.CapacityBatch(B, nmax, row_cap, int(rec[sched, 1].sum(1).max()) + 8, U.FIN, dev, ghost_slots=ghost, tail_cap=tail_cap)
    old = None
    if B <= 8:                                                    # the triplet gather on the same arena, schedule and capacities
        old = ingest.CapacityBatch(B, nmax, row_cap, 4, U.FIN, dev, ghost_slots=ghost, tail_cap=tail_cap)
        old_sched, old_ids = st._sched.clone(), torch.zeros(B, dtype=torch.int32, device=dev)
    R_ = row_cap + nmax
    feats = torch.from_numpy(st.arena.feats).to(dev)
    prev = None
    for k, ids in enumerate(twice):
        st.gather()
        torch.cuda.synchronize()
        now = _bits(bufs)
        if k % 2:
            assert _same_bits(prev, now), k                       # the same entry again: bit for bit
            continue
        prev = now
        ref.collate(ds, ids)
        ref.pull()
        torch.cuda.synchronize()
        n, ntail = ref.rows, ref.tail
        assert n == rec[ids, 0].sum() <= row_cap and ntail == rec[ids, 2].sum() <= tail_cap and (ntail > 0) == (U.TAIL in ids)
        rell, _, (rtp, rtc) = ref.g._ell
        want = {"graph_ptr": ref.g.graph_ptr, "slot_count": ref.g.slot_count, "row_graph": ref.g.row_graph, "row_slot": ref.g.row_slot,
                "ell": rell, "tail_ptr": rtp, "tail_col": rtc[:ntail], "ell_slots": ref.ell_slots, "tail_slots": ref.tail_slots[:ntail]}
        got = _outputs(st, ntail)
        for name in want:
            assert got[name].shape == want[name].shape and torch.equal(got[name], want[name]), (k, name, int((got[name] != want[name]).sum()))
        assert st.ids_out.tolist() == ids.tolist()
        assert st.label.dtype == torch.int64 and torch.equal(st.label, ref.label) and st.label.tolist() == [graphs[i].graph["label"] for i in ids]
        # the numpy restatement
        py = U.restate_launch(graphs, ids.tolist(), nmax, row_cap)
        for name in got:
            assert np.array_equal(got[name].cpu().numpy(), py[name]), (k, name)
        assert np.array_equal(st.label.cpu().numpy(), py["label"]) and np.array_equal(st.ids_out.cpu().numpy(), py["ids"])
        assert np.array_equal(st.x.cpu().numpy().view(np.int32), py["x"].view(np.int32))
        # x: the arena's feature rows on the real rows, exactly +0 everywhere else (no NaN left: every word was written)
        rows = torch.cat([torch.arange(int(rec[i, 3]), int(rec[i, 3] + rec[i, 0])) for i in ids]).to(dev)
        assert st.x.shape == (R_, U.LD) and torch.equal(st.x[:n], feats[rows])
        assert not bool(st.x[n:].view(torch.int32).ne(0).any()) and not bool(torch.isnan(st.x).any())
        for name, (buf, words) in bufs.items():
            want_guard = float(GUARD) if buf.dtype == torch.float32 else GUARD
            assert bool((buf[words:] == want_guard).all()), (k, name)
            if name not in ("tail_col", "tail_slots") and buf.dtype != torch.float32:
                assert not bool((buf[:words] == POISON).any()), (k, name)
        assert not bool((bufs["tail_col"][0][:ntail] == POISON).any()) and not bool((bufs["tail_slots"][0][:ntail] == POISON).any())
        if old is not None:
            ar, og = st.arena, old.g
            oell, ell_w, (otp, otc) = og._ell
            for _ in range(2):                                    # (its cursor walks the doubled schedule too)
                nat.call("triplet_gather_f32", st.records, ar.n_graphs, st.buf, ar.off["rowptr"], ar.off["col"], ar.off["tail_ptr"],
                         ar.off["tail_col"], ar.words, st.feats, ar.ld, row_cap, tail_cap, old_sched[HEAD:], st.max_steps, old_sched,
                         old_sched[4:HEAD], B, nmax, row_cap, tail_cap, ell_w, og.graph_ptr, og.slot_count, og.row_graph, og.row_slot, oell,
                         otp, otc, old.ell_slots, old.tail_slots, old.x, old.x.stride(0), old_ids)
            torch.cuda.synchronize()
            wold = {"graph_ptr": og.graph_ptr, "slot_count": og.slot_count, "row_graph": og.row_graph, "row_slot": og.row_slot, "ell": oell,
                    "tail_ptr": otp, "tail_col": otc[:ntail], "ell_slots": old.ell_slots, "tail_slots": old.tail_slots[:ntail]}
            for name in wold:
                assert torch.equal(got[name], wold[name]), (k, name)
            assert torch.equal(st.ids_out, old_ids) and torch.equal(st.x.view(torch.int32), old.x.view(torch.int32))
    # every launch advanced the cursor once and left its ticket counters (shards and top) at zero; grids from 12 workgroups (fewer
    # than shards) to 148 (shards of unequal size)
    assert st.position() == len(twice) and not bool(st._tickets.any())


# ------------------------------------------------------------------------------------------------ 2. the one-hot feature mode
@pytest.mark.parametrize("B,nmax", [(3, 48), (33, 64), (128, 48)])
def test_one_hot_mode_equals_the_table_mode_bit_for_bit(B, nmax):
    """features="node-label" (no table on the device: the launch writes the rows from the nodes' labels) against the float table that
    holds those one-hot rows, and against the ingest expansion of the same batch"""
    from two_stage_gnn_amd import ingest
    m = _model()
    tab, sched, graphs, ds = _stream(m, B, nmax, onehot=True)
    hot, _, _, _ = _stream(m, B, nmax, onehot=True, features="node-label", tu=True)
    assert hot.feats is None and hot.node_label is not None and tab.feats is not None and tab.node_label is None
    assert hot.arena.fin == tab.arena.fin == U.FIN
    bt, bh = _guarded(tab), _guarded(hot)
    tab.load(sched)
    hot.load(sched)
    ref = ingest.CapacityBatch(B, nmax, tab.row_cap, int(tab.arena.records[:, 1].astype(np.int64)[sched].sum(1).max()) + 8, U.FIN, tab.device,
                               ghost_slots=min(nmax, 49), tail_cap=tab.tail_cap)
    for k, ids in enumerate(sched):
        tab.gather()
        hot.gather()
        ref.collate(ds, ids)
        ref.pull()
        torch.cuda.synchronize()
        a, b = _bits(bt), _bits(bh)
        ntail = ref.tail
        for name in a:
            words = slice(None) if name not in ("tail_col", "tail_slots") else slice(0, ntail)
            x, y = a[name][words], b[name][words]
            if x.dtype == torch.float32:
                x, y = x.view(torch.int32), y.view(torch.int32)
            assert torch.equal(x, y), (k, name)
        assert torch.equal(hot.x.view(torch.int32), ref.x.view(torch.int32)), k
        n = ref.rows
        assert float(hot.x[:n].sum()) == n and float(hot.x[:n].max(dim=1).values.min()) == 1.0 and not bool(hot.x[n:].view(torch.int32).ne(0).any())


# ------------------------------------------------------------------------------------------------ 3. the cursor
def test_replays_walk_the_schedule_and_wrap():
    B = 9
    st, sched, graphs, ds = _stream(_model(), B, exact=False)
    T = st.load(sched)
    assert T == 5 and len(st) == 5 and st.position() == 0
    st.gather()                                                   # (library load and allocator warm-up outside the capture)
    torch.cuda.synchronize()
    assert st.position() == 1
    st.load(sched)
    assert st.position() == 0                                     # load() resets the cursor
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        st.gather()
    assert st.position() == 0                                     # (capturing runs nothing)
    for k in range(T + 2):
        graph.replay()
        torch.cuda.synchronize()
        assert st.ids_out.tolist() == sched[k % T].tolist(), k
        assert st.label.tolist() == [graphs[i].graph["label"] for i in sched[k % T]], k
    assert st.position() == T + 2
    st.load(sched[::-1].copy()[:3])                               # a shorter schedule into the same buffer: the captured launch serves it
    assert st.position() == 0
    for k in range(4):
        graph.replay()
        torch.cuda.synchronize()
        assert st.ids_out.tolist() == sched[::-1][k % 3].tolist(), k
    with pytest.raises(ValueError, match="exceeds"):
        st.load(np.ones((T + 1, B), dtype=np.int64))
    over = sched.copy()
    over[2] = U.FULL                                              # B copies of the largest graph: more rows than the slot has
    assert st.fits(over).tolist() == [True, True, False, True, True]
    with pytest.raises(ValueError, match="entry 2 has %d rows.*eager route" % (B * 48)):
        st.load(over)
    assert st.position() == 4 and len(st) == 3                    # a refused schedule leaves the loaded one alone
    with pytest.raises(RuntimeError, match="no negative to mine"):
        st.mine(None, None, 1.0)
    # a ticket counter that a launch cut short left behind: load() clears it with the schedule, and the cursor advances again
    st._tickets[0] = 7
    st._tickets[32 * 32] = 3
    st.load(sched)
    assert not bool(st._tickets.any())
    graph.replay()
    graph.replay()
    assert st.position() == 2 and not bool(st._tickets.any()) and st.ids_out.tolist() == sched[1].tolist()


def test_max_steps_sizes_the_buffer_before_the_first_schedule():
    B = 8
    st, sched, graphs, ds = _stream(_model(), B, exact=False, max_steps=6)
    assert len(st) == 1 and st.position() == 0                    # the one-entry schedule of B copies of the smallest graph: a warm-up
    st.gather()
    assert st.position() == 1 and st.ids_out.tolist() == [U.ONE_NODE] * B
    assert st.load(sched) == 5 and st.position() == 0
    st.gather()
    assert st.position() == 1 and st.ids_out.tolist() == sched[0].tolist()
    with pytest.raises(ValueError, match="exceeds"):
        st.load(np.ones((7, B), dtype=np.int64))


# ------------------------------------------------------------------------------------------------ 4. one streamed step per entry
def _grads_of(m):
    return {k: p.grad.detach().clone() for k, p in m.named_parameters() if p.grad is not None}


def _oracle_step(p_ref, graphs, ids):
    """the reference's step on the dense batch: GcnEncoderGraph.forward + cross-entropy -> (loss, ypred, grads)"""
    for v in p_ref.values():
        v.grad = None
    x = torch.from_numpy(np.stack([graphs[i].graph["feats"] for i in ids]))
    adj = torch.from_numpy(np.stack([graphs[i].graph["adj"] for i in ids]))
    y = torch.tensor([graphs[i].graph["label"] for i in ids])
    ypred = R.gcn_encoder(p_ref, x, adj, bn=True, final_dim="number_classes")[1]
    loss = torch.nn.functional.cross_entropy(ypred, y)
    loss.backward()
    return loss.detach(), ypred.detach(), {k: v.grad for k, v in p_ref.items() if v.grad is not None}


@pytest.mark.parametrize("B,nmax", [(8, 48), (32, 64)])
def test_streamed_step_equals_the_exact_batch_and_the_oracle(B, nmax):
    """every schedule entry, from the same parameters: loss and ypred of the streamed step against ``eager_step(ids)`` on the exact,
    unpadded batch at rtol = atol = 1e-5, every parameter gradient at atol = 2e-5 * max|grad|, ypred and the loss against the CPU
    oracle's dense batch at 1e-4 and its gradients at 2e-3 * max|grad of that parameter| + 1e-6 (the bounds of
    test_gpu_triplet_stream.test_streamed_step_equals_the_drop_in_and_the_oracle).  Gradients are compared from equal parameters,
    never after Adam.  Whether ypred comes out bit for bit equal to the exact batch's is printed, not asserted."""
    m = _model()
    st, sched, graphs, ds = _stream(m, B, nmax, exact=False)
    st.load(sched)
    p_ref = {k: v.detach().cpu().clone().requires_grad_(True) for k, v in m.state_dict().items()}
    for k, ids in enumerate(sched):
        m.zero_grad(set_to_none=True)
        loss, ypred = st.step()
        loss.backward()
        gs = _grads_of(m)
        assert st.ids_out.tolist() == ids.tolist() and ypred.shape == (B, U.N_CLASSES)
        m.zero_grad(set_to_none=True)
        losse, yprede = st.eager_step(ids)
        losse.backward()
        ge = _grads_of(m)
        torch.testing.assert_close(loss.detach(), losse.detach(), rtol=1e-5, atol=1e-5)
        torch.testing.assert_close(ypred.detach(), yprede.detach(), rtol=1e-5, atol=1e-5)
        assert gs.keys() == ge.keys() and len(gs) >= 10
        scale = max(float(v.abs().max()) for v in ge.values())
        worst = max(float((gs[n_] - ge[n_]).abs().max()) for n_ in ge)
        print("B %d entry %d: loss %.6f, max|grad| %.3e, max|stream - exact| %.3e (bound %.3e), ypred bit for bit: %s, max|ypred diff| %.3e"
              % (B, k, float(loss.detach()), scale, worst, 2e-5 * scale, bool(torch.equal(ypred, yprede)),
                 float((ypred.detach() - yprede.detach()).abs().max())))
        for n_ in ge:
            err = float((gs[n_] - ge[n_]).abs().max())
            assert err <= 2e-5 * scale, (k, n_, err, scale)
        lo, yo, go = _oracle_step(p_ref, graphs, ids)
        torch.testing.assert_close(ypred.detach().cpu(), yo, rtol=1e-4, atol=1e-4)
        torch.testing.assert_close(loss.detach().cpu(), lo, rtol=1e-4, atol=1e-4)
        assert set(go) == set(gs)                                   # every gradient of the step is compared, none skipped
        for n_, ref in go.items():
            err = float((gs[n_].cpu() - ref).abs().max())
            assert err <= 2e-3 * float(ref.abs().max()) + 1e-6, (k, n_, err, float(ref.abs().max()))


# ------------------------------------------------------------------------------------------------ 5. an epoch
def test_an_epoch_from_one_hipgraph_equals_eager_steps():
    """epoch_schedule -> load -> T replays of one GraphedStep -> eager_loss(rest), against eager steps over the same ids: per-step
    losses at rtol 1e-4, every final parameter at rtol 1e-4 with atol 1e-6.  The atol is for entries near zero, where a relative bound
    says nothing: 1e-6 is a thousandth of ONE Adam step of lr 1e-3 (an entry moves by about lr per step whatever its gradient's size)
    and about 30 ulp of the largest parameters (|p| ~ 0.3).  Measured on an MI355X: largest difference 3.0e-8 after 5 steps, largest
    relative difference 1.4e-4, on an entry of magnitude ~1e-4."""
    from two_stage_gnn_amd import minibatch_stream as MS
    from two_stage_gnn_amd.data_parallel import FlatTrainer, GraphedStep
    graphs, ds = _data()
    B, lr = 5, 1e-3
    full, rest = MS.epoch_schedule(len(graphs), B, np.random.default_rng(7))
    assert full.shape == (4, B) and rest.shape == (4,)
    m1 = _model()
    m2 = copy.deepcopy(m1)

    def eager_step(tr, st, ids):
        tr.zero_grad()
        loss = st.eager_loss(ids)
        tr.backward(loss)
        tr.gather_grads()
        tr.apply()
        return float(loss.detach())
    st2, tr2 = MS.MiniBatchStream(m2, ds, B, nmax=U.NMAX), FlatTrainer(m2, lr=lr, clip=2.0)
    eager = [eager_step(tr2, st2, ids) for ids in full] + [eager_step(tr2, st2, rest)]
    st1 = MS.MiniBatchStream(m1, ds, B, nmax=U.NMAX, max_steps=len(full))
    assert st1.row_cap == (48 + 45 + 40 + 36 + 33 + 31) // 32 * 32 and st1.fits(full).all()      # the default: the B largest graphs
    tr1 = FlatTrainer(m1, lr=lr, clip=2.0)
    gs = GraphedStep(tr1, st1.loss())                             # (its warm-up steps consume the warm-up entry ...)
    st1.load(full)                                                # ... so the epoch starts here: cursor := 0
    streamed = []
    for _ in range(len(full)):
        gs.step()
        streamed.append(gs.loss_value())
    gs.synchronize()                                              # (the documented loop: wait for the replays before eager work)
    assert st1.position() == len(full)
    streamed.append(eager_step(tr1, st1, rest))
    print("losses streamed %s eager %s" % (streamed, eager))
    np.testing.assert_allclose(streamed, eager, rtol=1e-4)
    steps = len(full) + 1
    diff = max(float((p1.detach() - p2.detach()).abs().max()) for p1, p2 in zip(m1.parameters(), m2.parameters()))
    rel = max(float(((p1.detach() - p2.detach()).abs() / p2.detach().abs().clamp_min(1e-12)).max()) for p1, p2 in zip(m1.parameters(), m2.parameters()))
    print("after %d steps: max parameter difference %.3e, max relative difference %.3e (asserted: rtol 1e-4, atol 1e-6)" % (steps, diff, rel))
    for (name, p1), p2 in zip(m1.named_parameters(), m2.parameters()):
        np.testing.assert_allclose(p1.detach().cpu().numpy(), p2.detach().cpu().numpy(), rtol=1e-4, atol=1e-6, err_msg=name)


# ------------------------------------------------------------------------------------------------ 6. no host in the loop
def test_no_host_in_the_loop():
    from two_stage_gnn_amd.data_parallel import FlatTrainer, GraphedStep
    m = _model()
    st, sched, graphs, ds = _stream(m, 32, 64, onehot=True, features="node-label", exact=False, tu=True)
    st.load(sched)
    gs = GraphedStep(FlatTrainer(m, lr=1e-3, clip=2.0), st.loss())
    st.load(sched)
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


# ------------------------------------------------------------------------------------------------ 7. the launch trace
def test_launch_trace_is_the_capacity_batch_step_behind_the_gather():
    from two_stage_gnn_amd import _native as nat
    m = _model()
    st, sched, graphs, ds = _stream(m, 32, 64, exact=False)
    st.load(sched)
    st.loss()().backward()                                        # (warm: allocator, library load)

    def traced(fn):
        m.zero_grad(set_to_none=True)
        nat.trace = []
        try:
            fn().backward()
            return [t[0] for t in nat.trace], [t[2] for t in nat.trace]
        finally:
            nat.trace = None
    names, kernels = traced(st.loss())
    plain, _ = traced(lambda: m.loss(m(st.x, st.g)[1], st.label))   # the capacity-batch step on the batch that is already there
    print("library launches of a streamed mini-batch step: %d\n%s" % (len(names), " ".join(names)))
    assert names[0] == "batch_gather_f32" and kernels[0].startswith("batch_gather_kernel") and names[1:] == plain
    assert "batch_gather_f32" not in plain and len(plain) >= 6
    assert not [n for n in names if n in ("row_maps", "ell_spmm_f32", "ingest_pull_expand_ack_f32", "ingest_expand_ack_f32")], names


# ------------------------------------------------------------------------------------------------ 8. poisoned capacity
def _poison_allocator(nbytes):
    """fill the caching allocator's free memory with NaN: allocate, fill and free tensors of the step's sizes (the allocator hands
    the same blocks to the next step's torch.empty calls)"""
    ts = [torch.empty(max(n // 4, 1), dtype=torch.float32, device="cuda") for n in nbytes for _ in range(3)]
    for t in ts:
        t.fill_(float("nan"))
    torch.cuda.synchronize()
    del ts


@pytest.mark.parametrize("B,nmax", [(8, 48), (32, 64)])
def test_poisoned_capacity_buffers_and_allocator_memory_change_nothing(B, nmax):
    """before every step the slot's arrays hold poison (NaN feature rows, poison words in every int array, the CSR tail past the
    entry's own included) and the allocator's free blocks hold NaN: loss, ypred and every gradient are bit for bit the clean run's"""
    from two_stage_gnn_amd import _native as nat
    m = _model()
    st, sched, graphs, ds = _stream(m, B, nmax, exact=False)

    def entry():
        m.zero_grad(set_to_none=True)
        loss, ypred = st.step()
        loss.backward()
        return loss.detach().clone(), ypred.detach().clone(), _grads_of(m)
    st.load(sched)
    nat.trace = []
    try:
        clean = [entry() for _ in sched]
        sizes = sorted({a.untyped_storage().nbytes() for t in nat.trace for a in t[1] if isinstance(a, torch.Tensor)})
    finally:
        nat.trace = None
    assert len(sizes) > 8
    st.load(sched)
    g, b = st.g, st.batch
    ell, _, (tail_ptr, tail_col) = g._ell
    for k, ids in enumerate(sched):
        for t in (g.graph_ptr, g.slot_count, g.row_graph, g.row_slot, ell, tail_ptr, tail_col, b.ell_slots, b.tail_slots, st.ids_out, st.label):
            t.fill_(POISON)
        st.x.fill_(float("nan"))
        _poison_allocator(sizes)
        loss, ypred, gs = entry()
        assert st.ids_out.tolist() == ids.tolist()
        assert torch.equal(loss, clean[k][0]) and torch.equal(ypred, clean[k][1]), (k, float(loss), float(clean[k][0]))
        assert set(gs) == set(clean[k][2])
        for key, v in gs.items():
            assert torch.equal(v, clean[k][2][key]), (k, key, float((v - clean[k][2][key]).abs().max()))


# ------------------------------------------------------------------------------------------------ 9. refusals
def test_validator_refuses_without_a_launch():
    from two_stage_gnn_amd import _native as nat
    from two_stage_gnn_amd.triplet_stream import HEAD
    st, sched, graphs, ds = _stream(_model(), 9, exact=False)
    st.load(sched)
    ar, g, b = st.arena, st.g, st.batch
    ell, ell_w, (tail_ptr, tail_col) = g._ell
    names = [p[1] for p in nat.parse_header()["tsgnn_batch_gather_f32"][1]][:-1]
    good = dict(zip(names, [st.records, ar.n_graphs, st.buf, ar.off["rowptr"], ar.off["col"], ar.off["tail_ptr"], ar.off["tail_col"], ar.words,
                            st.feats, ar.ld, None, ar.fin, st.labels, st.max_n, st.max_tail, st._sched[HEAD:], st.max_steps, st._sched,
                            st._tickets, st.B, ar.nmax, st.row_cap, st.tail_cap, ell_w, g.graph_ptr, g.slot_count, g.row_graph, g.row_slot,
                            ell, tail_ptr, tail_col, b.ell_slots, b.tail_slots, st.x, st.x.stride(0), st.ids_out, st.label]))
    assert len(good) == len(names) == 37
    odd = lambda t: t.view(-1)[1:]                                # 4 bytes off a 16-byte boundary
    nl = torch.zeros(ar.total_nodes, dtype=torch.int32, device=st.device)
    cases = [{k: None} for k in names if isinstance(good[k], torch.Tensor)]
    cases += [dict(node_label=nl), dict(B=0), dict(B=129), dict(row_cap=st.max_n - 1), dict(tail_cap=st.max_tail - 1), dict(max_n=ar.nmax + 1),
              dict(sched_cap=0), dict(ell_w=12), dict(feats=None, node_label=nl, fin=U.FIN + 4), dict(records=odd(st.records)),
              dict(arena=odd(st.buf)), dict(feats=odd(st.feats)), dict(ell=odd(ell)), dict(ell_slots=odd(b.ell_slots)), dict(x=odd(st.x)),
              dict(state=st._sched[2:]), dict(label_out=st.label.view(torch.int32)[1:]), dict(off_col=ar.off["col"] + 1),
              dict(ldx=st.x.stride(0) + 4)]
    torch.cuda.synchronize()
    before = st.position()
    nat.trace = []
    try:
        for kw in cases:
            with pytest.raises(RuntimeError, match="batch_gather_f32 failed"):
                nat.call("batch_gather_f32", *[{**good, **kw}[k] for k in names])
        assert nat.trace == []                                    # nothing was launched
        nat.call("batch_gather_f32", *[good[k] for k in names])
        assert len(nat.trace) == 1 and nat.trace[0][2].startswith("batch_gather_kernel")
    finally:
        nat.trace = None
    torch.cuda.synchronize()
    assert st.position() == before + 1


@pytest.mark.parametrize("B", [3, 65])
def test_a_schedule_word_past_n_graphs_is_clamped_into_the_records(B):
    """the raw entry point told that the table holds G - 2 records (it holds G): schedule words G - 1 and G - 2 — outside the launch's
    range, inside the allocation — must give, word for word in every output array, in ids_out and in the labels, what the same
    schedule with every index replaced by min(index, G - 3) gives (csrc/stream_protocol.h, stream_entry_id).  B = 65: the words of
    threads 63 and 64, one in each of the prologue's two waves."""
    from two_stage_gnn_amd import _native as nat
    from two_stage_gnn_amd.triplet_stream import HEAD
    st, _, graphs, ds = _stream(_model(), B, exact=False)
    G = len(graphs)
    small = [i for i, n in enumerate(U.SIZES) if n <= 11 and i < G - 3]
    sched = np.asarray([[small[(i + e) % len(small)] for i in range(B)] for e in range(3)], dtype=np.int64)
    sched[0, 0], sched[0, B - 1] = G - 1, G - 2
    sched[1, B // 2] = G - 1
    sched[2, B - 2], sched[2, B - 1] = G - 2, G - 1
    ar, g, b = st.arena, st.g, st.batch
    ell, ell_w, (tail_ptr, tail_col) = g._ell
    outs = {"graph_ptr": g.graph_ptr, "slot_count": g.slot_count, "row_graph": g.row_graph, "row_slot": g.row_slot, "ell": ell,
            "tail_ptr": tail_ptr, "tail_col": tail_col, "ell_slots": b.ell_slots, "tail_slots": b.tail_slots, "x": st.x, "ids_out": st.ids_out,
            "label": st.label}

    def run(schedule):
        st.load(schedule)
        got = []
        for _ in range(len(schedule)):
            for t in outs.values():
                t.view(torch.int32).fill_(POISON)                 # (words a launch does not write: the same in both passes)
            nat.call("batch_gather_f32", st.records, G - 2, st.buf, ar.off["rowptr"], ar.off["col"], ar.off["tail_ptr"], ar.off["tail_col"],
                     ar.words, st.feats, ar.ld, None, ar.fin, st.labels, st.max_n, st.max_tail, st._sched[HEAD:], st.max_steps, st._sched,
                     st._tickets, st.B, ar.nmax, st.row_cap, st.tail_cap, ell_w, g.graph_ptr, g.slot_count, g.row_graph, g.row_slot, ell,
                     tail_ptr, tail_col, b.ell_slots, b.tail_slots, st.x, st.x.stride(0), st.ids_out, st.label)
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


def test_constructor_refusals_name_the_eager_route():
    from two_stage_gnn_amd import dense_encoders as E
    from two_stage_gnn_amd import minibatch_stream as MS
    from two_stage_gnn_amd import triplet
    from two_stage_gnn_amd.tu_data import TUDataset
    graphs, ds = _data()
    good = _model()
    for bad in (triplet.tripletnet(_model(final_dim="output_dim")), _model(bn=False), _model(concat=False), _model(final_dim="output_dim"),
                _model().cpu()):
        with pytest.raises(TypeError, match="eager route"):
            MS.MiniBatchStream(bad, ds, 8)
    for B in (0, 129):
        with pytest.raises(ValueError, match="eager route"):
            MS.MiniBatchStream(good, ds, B)
    bare = TUDataset(ds.graph_ptr, ds.rowptr, ds.col, ds.graph_label, None, None, 0)
    with pytest.raises(ValueError, match="without node labels.*eager route"):
        MS.MiniBatchStream(good, bare, 8, features="node-label")
    with pytest.raises(TypeError, match="feature width 9 is not the model's 12.*eager route"):
        MS.MiniBatchStream(_model(fin=12), ds, 8)
    with pytest.raises(ValueError, match="below the dataset's largest graph.*eager route"):
        MS.MiniBatchStream(good, ds, 8, row_cap=40)
    st = MS.MiniBatchStream(good, bare, 8)                          # no attributes, no node labels: constant features of the model's width
    assert st.arena.fin == U.FIN and bool((st.feats[:, :U.FIN] == 1).all()) and st.row_cap == 288
    with pytest.raises(ValueError, match="1 to 8 integer"):
        st.eager_loss(np.arange(9))
    # max_steps asks for a warm-up entry: B copies of the smallest graph, and a ValueError that says so when not even those fit
    with pytest.raises(ValueError, match="max_steps asks for a warm-up entry"):
        MS.MiniBatchStream(good, ds, 128, row_cap=48, max_steps=3)
    tight = MS.MiniBatchStream(good, ds, 64, row_cap=64, max_steps=3)             # 64 copies of the one-node graph fill the slot exactly
    assert tight.row_cap == 64 and len(tight) == 1
    # the graph-object route in the node-label mode: a subset that lacks the largest node label keeps the model's width
    graphs1, _ = _data(onehot=True)
    some = [g for g in graphs1 if int(np.max(g.graph["node_label"])) < U.FIN - 1]
    assert 0 < len(some) < len(graphs1)
    sub = MS.MiniBatchStream(good, some, 2, features="node-label")
    assert sub.arena.fin == U.FIN and sub.feats is None
