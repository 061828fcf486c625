"""The SAGPool mini-batch stream on the GPU (two_stage_gnn_amd/sag_stream.py ``MiniBatchStream``, csrc/sag_batch_stream.hip):

  1. the gather launch alone, through the C ABI, into guarded buffers: every word against the numpy restatement
     (tests/sag_minibatch_util.launch_np) and ``SagPlan``'s host graph pointers, for B = 1 .. 128, two ratios, three capacities (exactly
     the first entry's, no multiple of 4, the default), every launch twice, cursor and ticket words after each; B = 3 and B = 1 bit for
     bit against the two existing gather launches at equal capacities;
  2. one streamed step per entry against ``eager_step`` on the same ids and ``Net(use_batch=True)`` on a hand-collated batch (logp and
     loss bit for bit at dropout 0; parameter gradients at rtol = atol = 1e-5, the rule tests/test_gpu_sag_stream.py applies between its
     stream and its drop-in: the slab plans differ with the capacity), and against the fp64 / fp32 CPU oracle ``pyg_ref.sag_net`` with
     the batch vector at the bounds of tests/test_gpu_sag_triplet.py for this node (outputs rtol = atol = 1e-5; the loss that or 10 x
     the fp32 oracle's own error; gradients 1e-4 of the tensor's largest entry or 10 x the fp32 oracle's own error);
  3. B = 128; poisoned capacity buffers and allocator memory; the in-kernel dropout mask; an epoch from one hipGraph with its remainder
     through ``eager_loss``; no host in the loop and the launch trace; every refusal of the constructor, ``load`` and ``mine``.
Datasets, schedules, the restatement and the oracle: tests/sag_minibatch_util.py."""
import copy

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import sag_minibatch_util as M
import sag_stream_util as U0
from guard_buf import GUARD, PAT
from test_gpu_sag_triplet import _bound

pytestmark = pytest.mark.gpu

IPAT = -1


def _stream(name, B, mode="train", p_drop=0.0, sched=None, **kw):
    """``sched``: a schedule the stream has to hold; where the default capacity (the B largest DISTINCT graphs) does not — dd3's
    entries name a graph twice — the stream is built at the schedule's own capacity"""
    from two_stage_gnn_amd import sag_stream as S
    m = M.net(name, mode, p_drop)
    datas = M.datas(name)
    if sched is not None:
        rec = S.size_records(datas)
        caps = S.default_level_caps(rec, B, M.RATIO, M.DEPTH)
        if not S.fits_mask(sched, rec, B, caps[0], S.default_nnz_cap(rec, B), caps, M.RATIO).all():
            kw.update(S.schedule_capacity(rec, sched, M.RATIO, M.DEPTH))
    return m, datas, S.MiniBatchStream(m, datas, B, **kw)


# ------------------------------------------------------------------------------------------------ 1. the gather launch alone
class _Guarded:
    """n words on the device prefilled with one pattern (a NaN for float32, -1 for the integers), GUARD words of it behind"""

    def __init__(self, n, dtype):
        self.n, self.dtype = n, dtype
        w = 2 if dtype == torch.int64 else 1
        self.pat = PAT if dtype == torch.float32 else IPAT
        self.bits = torch.full((w * n + GUARD,), self.pat, dtype=torch.int32, device="cuda")
        self.t = self.bits[:w * n].view(dtype)

    def get(self, what):
        torch.cuda.synchronize()
        b = self.bits.cpu()
        w = 2 if self.dtype == torch.int64 else 1
        assert bool((b[w * self.n:] == self.pat).all()), "%s: guard words overwritten" % what
        return b[:w * self.n].view(torch.int64 if self.dtype == torch.int64 else torch.int32).numpy()


def _launch(st, B, ratio, row_cap, nnz_cap, level_caps, ldg, depth=M.DEPTH, entry="sag_batch_gather_f32"):
    """a gather launch on the stream's arena, schedule buffer and ticket words into guarded buffers of the given capacities ->
    {name: int32 / int64 bit view on the CPU}"""
    from two_stage_gnn_amd import _native as nat
    from two_stage_gnn_amd.triplet_stream import HEAD
    ar, R = st.arena, row_cap
    G = {"rowptr": _Guarded(R + 1, torch.int32), "col": _Guarded(nnz_cap, torch.int32), "x": _Guarded(R * ar.ld, torch.float32),
         "dinv": _Guarded(R, torch.float32), "self_w": _Guarded(R, torch.float32), "gp": _Guarded(ldg * (depth + 1), torch.int32),
         "ids": _Guarded(B, torch.int32)}
    if entry == "sag_batch_gather_f32":
        G["label"] = _Guarded(B, torch.int64)
        caps = np.asarray(level_caps, dtype=np.int64)
        nat.call(entry, st.records, ar.n_graphs, st.buf, ar.off["rowptr"], ar.off["col"], ar.words, st.feats, ar.ld, st.labels, st.max_n,
                 st.max_nnz, st._sched[HEAD:], st.max_steps, st._sched, st._tickets, B, R, nnz_cap, caps.ctypes.data, float(ratio), depth,
                 G["rowptr"].t, G["col"].t, G["x"].t, ar.ld, G["dinv"].t, G["self_w"].t, G["gp"].t, ldg, G["ids"].t, G["label"].t)
        assert nat.last_kernel() == "sag_batch_gather_kernel"
    else:                                                     # the triplet / anchor launch on the same arena and schedule
        nat.call(entry, st.records, ar.n_graphs, st.buf, ar.off["rowptr"], ar.off["col"], ar.words, st.feats, ar.ld, B * st.max_n,
                 B * st.max_nnz, st._sched[HEAD:], st.max_steps, st._sched, st._sched[4:HEAD], R, nnz_cap, float(ratio), depth,
                 G["rowptr"].t, G["col"].t, G["x"].t, ar.ld, G["dinv"].t, G["self_w"].t, G["gp"].t, G["ids"].t)
    return {k: v.get(k) for k, v in G.items()}


def _bits32(a):
    return np.ascontiguousarray(a).view(np.int32).reshape(-1)


def _capacities(S, rec, sched, B, ratio, mode):
    """(row_cap, nnz_cap, level_caps): "exact" — the schedule's own (the first entry is its largest: row_cap IS its row count);
    "odd" — a row_cap that is no multiple of 4; "default" — the B largest graphs"""
    if mode == "default":
        caps = S.default_level_caps(rec, B, ratio, M.DEPTH)
        return caps[0], S.default_nnz_cap(rec, B), caps
    sc = S.schedule_capacity(rec, sched, ratio, M.DEPTH)
    caps = list(sc["level_caps"])
    if mode == "odd":
        caps[0] += 1 if (caps[0] + 1) % 4 else 2
        caps[2] += 3
    return caps[0], sc["nnz_cap"] + (5 if mode == "odd" else 0), caps


GATHER_CASES = [("small12", B) for B in (1, 2, 3, 4, 5, 31, 32, 33, 64, 65, 127, 128)] + [("fin1", 3), ("fin1", 5), ("dd3", 2), ("dd3", 5)]


@pytest.mark.parametrize("name,B", GATHER_CASES)
def test_gather_launch_equals_the_restatement_word_for_word(name, B):
    """every word the launch writes, padding included, against the numpy restatement; ``graph_ptr`` against ``SagPlan``'s host values at
    every level; labels and ``ids_out``; guards intact; every launch twice, bit for bit; cursor and ticket words after each launch"""
    from two_stage_gnn_amd import sag_stream as S
    from two_stage_gnn_amd.sag_stack import SagPlan
    fin, nhid, C, graphs, labels = M.dataset(name)
    sched = M.schedule(name, B)
    m, datas, st = _stream(name, B)                                # (its arena, schedule buffer and ticket words; the launches below
    rec, per = U0.restate(graphs)                                  # write into guarded buffers of their own capacities)
    ar, ldg = st.arena, (B + 1 + 3) // 4 * 4
    twice = np.repeat(sched, 2, axis=0)
    launches = 0
    for ratio in (0.5, 0.8):
        for mode in ("exact", "odd", "default"):
            R, nnz_cap, caps = _capacities(S, rec, sched, B, ratio, mode)
            assert S.fits_mask(sched, rec, B, R, nnz_cap, caps, ratio).all()
            if mode == "exact":
                assert R == int(np.array(M.SIZES[name])[sched[0]].sum())
            if mode == "odd":
                assert R % 4
            st.load(twice)
            prev = None
            for k, ids in enumerate(twice):
                got = _launch(st, B, ratio, R, nnz_cap, caps, ldg)
                launches += 1
                assert st.position() == k + 1 and not bool(st._tickets.any()), (k, "cursor / tickets")
                want = M.launch_np(rec, per, labels, ids, ratio, M.DEPTH, R, nnz_cap, caps, ldg, ar.ld, col_fill=IPAT)
                for key in ("rowptr", "col", "ids", "label"):
                    assert np.array_equal(got[key], want[key]), (ratio, mode, k, key)
                for key in ("x", "dinv", "self_w"):
                    assert np.array_equal(got[key], _bits32(want[key])), (ratio, mode, k, key)
                gp = got["gp"].reshape(M.DEPTH + 1, ldg)
                assert np.array_equal(gp, want["gp"]), (ratio, mode, k, "gp")
                plan = SagPlan(np.array(M.SIZES[name])[ids], ratio, "cpu", M.DEPTH)
                for l in range(M.DEPTH + 1):
                    assert gp[l, :B + 1].tolist() == plan.levels[l].gp.tolist(), (ratio, mode, k, l)
                if k % 2:
                    assert all(np.array_equal(got[key], prev[key]) for key in got), (ratio, mode, k, "second launch differs")
                prev = got
    assert launches == 12 * len(sched)


@pytest.mark.parametrize("name,B", [("small12", 3), ("small12", 1), ("dd3", 3), ("dd3", 1)])
def test_b3_and_b1_equal_the_existing_gather_launches_bit_for_bit(name, B):
    """at the triplet / anchor launch's capacities (B times the largest graph at every level) and its [depth + 1, 4] pointers"""
    from two_stage_gnn_amd import sag_stream as S
    rec = S.size_records(M.datas(name, "cpu"))
    R, nnz_cap = B * int(rec[:, 0].max()), max(B * int(rec[:, 1].max()), 1)
    m, datas, st = _stream(name, B, level_caps=[B * k for k in S.k_chain(R // B, M.RATIO)], nnz_cap=nnz_cap)
    sched = M.schedule(name, 3)[:, :B]
    assert st.plan.ldg == 4 and st.row_cap == R == B * st.max_n
    old = "sag_triplet_gather_f32" if B == 3 else "sag_anchor_gather_f32"
    for ratio in (0.5, 0.8):
        caps = [B * k for k in S.k_chain(st.max_n, ratio)]
        st.load(sched)
        new = [_launch(st, B, ratio, R, nnz_cap, caps, 4) for _ in sched]
        st.load(sched)
        for k, ids in enumerate(sched):
            got = _launch(st, B, ratio, R, nnz_cap, caps, 4, entry=old)
            assert got["ids"].tolist() == ids.tolist()
            for key in got:
                assert np.array_equal(got[key], new[k][key]), (ratio, k, key)


def _walk(st, sched, tickets):
    """three launches of a three-entry schedule: after each the cursor, every ticket word (zero again) and ``ids_out``"""
    assert st.load(sched) == 3 and st.position() == 0
    for k, ids in enumerate(sched):
        st.gather()
        assert st.position() == k + 1, (k, "cursor")
        assert not bool(tickets().any()), (k, "ticket words")
        assert st.ids_out.tolist() == ids.tolist(), (k, "ids_out")


@pytest.mark.parametrize("row_cap,workgroups", [(32, 1), (992, 31), (1024, 32), (1056, 33), (2112, 66)])
def test_sharded_ticket_at_its_grid_edges(row_cap, workgroups):
    """``stream_ticket_sharded`` (csrc/stream_protocol.h) where its arithmetic changes: 32 rows per workgroup, so ``row_cap`` sets the
    grid — one workgroup, S = gridDim.x = 31, S = 32 with one member per shard, 33 (shard 0 has two members, the others one) and 66
    (two shards of three, thirty of two)"""
    from two_stage_gnn_amd import sag_stream as S
    m, datas, st = _stream("fin1", 2, row_cap=row_cap)
    assert st.row_cap == row_cap and (row_cap + 31) // 32 == workgroups and int(st.level_caps[0]) == row_cap
    assert st.level_caps.tolist() == [min(c, row_cap) for c in [row_cap] + S.default_level_caps(st.arena.records, 2, M.RATIO, M.DEPTH)[1:]]
    _walk(st, np.array([[2, 3], [0, 1], [3, 0]], dtype=np.int64), lambda: st._tickets)


def test_flat_ticket_on_a_1d_and_a_2d_grid():
    """``stream_ticket_flat``: ``sag_triplet_gather`` at its default capacity (gridDim.x workgroups) and ``gat_triplet_gather`` on small3
    (gridDim.x * gridDim.y): the cursor and the single counter after each of three launches"""
    import gat_stream_util as UG
    import test_gpu_gat_stream as TG
    import test_gpu_sag_stream as TS
    from two_stage_gnn_amd.triplet_stream import HEAD
    st = TS._stream("small6")[3]
    _walk(st, U0.SCHEDULES["small6"][:3], lambda: st._sched[4:HEAD])
    sg = TG._stream("small3")[3]
    _walk(sg, UG.schedule("small3")[:3], lambda: sg._sched[4:HEAD])


# ------------------------------------------------------------------------------------------------ 2. the streamed step
def _grads(m):
    return {k: p.grad.detach().clone() for k, p in m.named_parameters() if p.grad is not None}


def _run(m, fn):
    m.zero_grad(set_to_none=True)
    loss, logp = fn()
    loss.backward()
    return loss.detach().clone(), logp.detach().clone(), _grads(m)


class _Batch:
    """a hand-collated mini-batch: what a PyG DataLoader hands ``Net.forward``"""

    def __init__(self, datas, ids, labels):
        off, xs, eis, bv = 0, [], [], []
        for b, i in enumerate(ids):
            d = datas[int(i)]
            xs.append(d.x); eis.append(d.edge_index + off); bv.append(torch.full((d.x.size(0),), b, dtype=torch.long, device=d.x.device))
            off += int(d.x.size(0))
        self.x, self.edge_index, self.batch = torch.cat(xs), torch.cat(eis, dim=1), torch.cat(bv)
        self.y = torch.as_tensor(labels[[int(i) for i in ids]]).to(self.x.device)


def _net_step(m, batch):
    from two_stage_gnn_amd import message_passing as mp
    logp = m(batch)
    return mp.nll_loss(logp, batch.y), logp


def _check_entry(name, k, ids, m, datas, st, labels):
    """the streamed step of the cursor's entry against the exact batch two ways and against the oracle; every figure is printed"""
    ls, ps, gs = _run(m, st.step)
    assert st.ids_out.tolist() == ids.tolist() and st.label.tolist() == labels[ids].tolist()
    le, pe, ge = _run(m, lambda: st.eager_step(ids))
    ln, pn, gn = _run(m, lambda: _net_step(m, _Batch(datas, ids, labels)))
    assert ps.shape == (len(ids), M.DIMS[name][2])
    for what, lo, po in (("eager_step", le, pe), ("Net(use_batch=True)", ln, pn)):
        assert torch.equal(ps, po) and torch.equal(ls, lo), (k, what, float((ps - po).abs().max()), float(ls), float(lo))
    assert set(gs) == set(ge) == set(gn) and len(gs) == 18
    worst = max(float((gs[n_] - ge[n_]).abs().max()) for n_ in ge)
    print("%s B %d entry %d: max|grad| %.3e, max|streamed - exact| gradient entry %.3e"
          % (name, len(ids), k, max(float(v.abs().max()) for v in ge.values()), worst))
    for key in gs:
        torch.testing.assert_close(gs[key], ge[key], rtol=1e-5, atol=1e-5, msg=lambda s_, key=key: "%s entry %d: %s" % (key, k, s_))
        torch.testing.assert_close(gn[key], ge[key], rtol=1e-5, atol=1e-5, msg=lambda s_, key=key: "%s entry %d (Net): %s" % (key, k, s_))
    ref = M.oracle(name, ids)
    (p64, l64, g64), (p32, l32, g32) = ref[torch.float64], ref[torch.float32]
    diff = (ps.cpu().double() - p64).abs()
    e_cpu = float((p32.double() - p64).abs().max())
    print("%s B %d entry %d logp: |hip - fp64| %.2e, |cpu fp32 - fp64| %.2e; loss %.6f vs %.6f" % (name, len(ids), k, float(diff.max()), e_cpu,
                                                                                                 float(ls), l64))
    assert bool((diff <= 1e-5 + 1e-5 * p64.abs()).all()), (k, "logp", float(diff.max()), e_cpu)
    assert abs(float(ls) - l64) <= max(1e-5 * max(1.0, abs(l64)), 10 * abs(l32 - l64)), (k, float(ls), l64, l32)
    assert set(gs) == set(g64)
    for key, r64 in g64.items():
        err = float((gs[key].cpu().double() - r64).abs().max())
        bound, e32 = _bound(r64, g32[key], 1e-4, 1e-9)
        assert err <= bound, (k, key, err, e32, float(r64.abs().max()))


@pytest.mark.parametrize("name,B,mode", [("small12", 4, "train"), ("small12", 3, "eval"), ("dd3", 3, "train"), ("dd3", 2, "train")])
def test_streamed_step_equals_the_exact_batch_and_the_oracle(name, B, mode):
    """one streamed step per entry from equal parameters (dropout_ratio 0); small12 at the default capacity, dd3 (whose entries name a
    graph twice) at the schedule's own"""
    sched = M.schedule(name, B)
    m, datas, st = _stream(name, B, mode, sched=sched)
    labels = M.dataset(name)[4]
    assert st.fits(sched).all()
    st.load(sched)
    for k, ids in enumerate(sched):
        _check_entry(name, k, ids, m, datas, st, labels)
    assert st.position() == len(sched)


def test_batch_of_128_small_graphs_equals_the_exact_batch_and_the_oracle():
    """B = 128 (two waves of records, ldg 132) on 40 graphs of n = 1 .. 40, every graph three or four times per entry"""
    m, datas, st = _stream("many40", 128)
    labels = M.dataset("many40")[4]
    sched = M.schedule("many40", 128)
    assert st.fits(sched).all() and st.plan.ldg == 132 and st.plan.levels[0].B == 128
    st.load(sched)
    for k, ids in enumerate(sched):
        _check_entry("many40", k, ids, m, datas, st, labels)


# ------------------------------------------------------------------------------------------------ 3. poisoned padding
def _poison(nbytes):
    """fill the caching allocator's free memory with NaN: allocate, fill and free tensors of the step's sizes (the allocator hands
    the same blocks to the next step's torch.empty calls)"""
    ts = [torch.empty(max(n // 4, 1), dtype=torch.float32, device="cuda") for n in nbytes for _ in range(3)]
    for t in ts:
        t.fill_(float("nan"))
    torch.cuda.synchronize()
    del ts


@pytest.mark.parametrize("name,B", [("small12", 4), ("dd3", 2)])
def test_poisoned_capacity_buffers_and_allocator_memory_change_nothing(name, B):
    """before every step the capacity buffers hold poison (NaN rows and coefficients, -1 in every integer array) and the allocator's
    free blocks hold NaN: loss, logp and every gradient are bit for bit the clean run's"""
    from two_stage_gnn_amd import _native as nat
    sched = M.schedule(name, B)
    m, datas, st = _stream(name, B, sched=sched)
    st.load(sched)
    nat.trace = []
    try:
        clean = [_run(m, st.step) for _ in sched]
        sizes = sorted({a.untyped_storage().nbytes() for t in nat.trace for a in t[1] if isinstance(a, torch.Tensor)})
    finally:
        nat.trace = None
    assert len(sizes) > 8
    st.load(sched)
    for k, ids in enumerate(sched):
        for t in (st.rowptr, st.col, st.plan.gp_all, st.ids_out, st.label):
            t.fill_(IPAT)
        for t in (st._x, st.dinv, st.self_w):
            t.view(torch.int32).fill_(PAT)
        _poison(sizes)
        loss, logp, gs = _run(m, st.step)
        assert st.ids_out.tolist() == ids.tolist()
        assert torch.equal(loss, clean[k][0]) and torch.equal(logp, clean[k][1]), (k, float(loss), float(clean[k][0]))
        assert set(gs) == set(clean[k][2])
        for key, v in gs.items():
            assert torch.equal(v, clean[k][2][key]), (k, key, float((v - clean[k][2][key]).abs().max()))


# ------------------------------------------------------------------------------------------------ 4. dropout
def test_dropout_mask_is_drawn_in_the_head_launch():
    """train mode, p = 0.5: the step's logp is the head applied to the step's readout rows with the mask ``mp.mlp3_dropout_mask``
    regenerates from ``last_mlp3_dropout`` for B rows, and two steps on the same entry draw different masks"""
    from two_stage_gnn_amd import _native as nat
    from two_stage_gnn_amd import message_passing as mp
    B = 4
    m, datas, st = _stream("small12", B, "train", 0.5)
    labels = M.dataset("small12")[4]
    ids = np.array([4, 9, 2, 11])
    st.load(np.stack([ids, ids]))
    masks, outs = [], []
    for _ in range(2):
        nat.trace = []
        try:
            loss, logp = st.step()
            loss.backward()
            names = [t[0] for t in nat.trace]
        finally:
            nat.trace = None
        assert names.count("mlp3_fwd_drop_f32") == 1 and names[0] == "sag_batch_gather_f32"
        p, seed, used = mp.last_mlp3_dropout
        assert p == 0.5
        mask = mp.mlp3_dropout_mask(p, seed, used, B, m.lin1.out_features)
        with torch.no_grad():
            r = st.readout()                                                  # (no gather in between: the same batch)
            h = F.relu(F.linear(r, m.lin1.weight, m.lin1.bias)) * mask * 2.0
            h = F.relu(F.linear(h, m.lin2.weight, m.lin2.bias))
            want = F.log_softmax(F.linear(h, m.lin3.weight, m.lin3.bias), dim=-1)
        torch.testing.assert_close(logp.detach(), want, rtol=1e-5, atol=1e-6)
        y = torch.as_tensor(labels[ids]).cuda()
        assert abs(float(loss.detach()) - float(F.nll_loss(want, y))) <= 1e-5
        masks.append(mask.cpu())
        outs.append(logp.detach().cpu())
        assert all(bool(torch.isfinite(q.grad).all()) for q in m.parameters())
    assert masks[0].shape == (B, m.lin1.out_features)
    assert not torch.equal(masks[0], masks[1]) and not torch.equal(outs[0], outs[1])
    assert 0.2 < float(masks[0].mean()) < 0.8


# ------------------------------------------------------------------------------------------------ 5. an epoch
def test_an_epoch_from_one_hipgraph_equals_uncaptured_streamed_steps():
    """``epoch_schedule`` on 40 graphs at B = 8: the full entries from ONE ``GraphedStep`` (weight decay 1e-4, no clipping: the
    reference's Adam), the remainder through ``eager_loss``; against uncaptured streamed steps of a deep-copied model — the same route
    run two ways, so rtol 1e-5 / atol 1e-6 on every parameter (the rule of test_gpu_sag_stream's replay test).  ``ids_out`` walks the
    schedule and the parameters moved."""
    from two_stage_gnn_amd import message_passing as mp, sag_stream as S
    from two_stage_gnn_amd.data_parallel import FlatTrainer, GraphedStep
    from two_stage_gnn_amd.minibatch_stream import epoch_schedule
    B, G = 8, 37                                                                # (the first 37 graphs: four full entries and five left)
    full, rest = epoch_schedule(G, B, np.random.default_rng(11))
    assert full.shape == (4, B) and rest.shape == (5,)
    m1, datas = M.net("many40", "train"), M.datas("many40")[:G]
    st1 = S.MiniBatchStream(m1, datas, B, max_steps=len(full))
    m2 = copy.deepcopy(m1)
    start = {k: v.detach().clone() for k, v in m1.state_dict().items()}
    kw = dict(lr=5e-4, weight_decay=1e-4, clip=0)

    def eager_step(tr, st, ids):
        tr.zero_grad()
        loss = st.eager_loss(ids)
        tr.backward(loss)
        tr.gather_grads()
        tr.apply()
        return float(loss.detach())
    st2 = S.MiniBatchStream(m2, datas, B)
    st2.load(full)
    tr2 = FlatTrainer(m2, **kw)
    step2 = st2.loss()
    plain = []
    for ids in full:
        tr2.step(step2)
        assert st2.ids_out.tolist() == ids.tolist()
    plain.append(eager_step(tr2, st2, rest))
    assert len(st1) == 1 and st1.fits(full).all()                               # (the warm-up entry: B copies of the single node)
    tr1 = FlatTrainer(m1, **kw)
    gs = GraphedStep(tr1, st1.loss())                                           # (its warm-up steps consume the warm-up entry ...)
    assert gs.describe().startswith("one graph"), gs.describe()
    st1.load(full)                                                              # ... so the epoch starts here: cursor := 0
    for ids in full:
        gs.step()
        gs.synchronize()
        assert st1.ids_out.tolist() == ids.tolist()
    assert st1.position() == len(full) and np.isfinite(gs.loss_value())
    streamed = eager_step(tr1, st1, rest)
    mp.check_device_errors()
    assert abs(streamed - plain[0]) <= 1e-5 * max(1.0, abs(plain[0]))
    moved = 0
    for (k, p1), (_, p2) in zip(m1.named_parameters(), m2.named_parameters()):
        torch.testing.assert_close(p1.detach(), p2.detach(), rtol=1e-5, atol=1e-6, msg=lambda s_, k=k: k + ": " + s_)
        moved += int(not torch.equal(p1.detach(), start[k]))
    assert moved == 18


# ------------------------------------------------------------------------------------------------ 6. no host in the loop, the trace
def test_no_host_in_the_loop():
    from two_stage_gnn_amd.data_parallel import FlatTrainer, GraphedStep
    B = 4
    m, datas, st = _stream("small12", B, "train", 0.5)
    sched = M.schedule("small12", B)
    st.load(sched)
    gs = GraphedStep(FlatTrainer(m, lr=5e-4, weight_decay=1e-4, clip=0), st.loss())
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


@pytest.mark.parametrize("name,B", [("small12", 4), ("dd3", 3)])
def test_launch_trace_is_the_resident_step_behind_one_gather_launch(name, B):
    from two_stage_gnn_amd import _native as nat
    m, datas, st = _stream(name, B, "train", 0.5, sched=M.schedule(name, B))
    st.load(M.schedule(name, B))
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
    plain, _ = traced(lambda: st._head(st.readout(), st.label)[0])     # the resident step on the batch that is already there
    print("library launches of a streamed SAGPool mini-batch step (%s, B %d): %d\n%s" % (name, B, len(names), " ".join(names)))
    assert names[0] == "sag_batch_gather_f32" and kernels[0] == "sag_batch_gather_kernel" and names[1:] == plain
    assert "sag_batch_gather_f32" not in plain and len(plain) >= 8
    assert names.count("sag_pool_graph_cap_f32") == 3 and names.count("sag_pool_graph_bwd_cap_f32") == 3
    assert names.count("mlp3_fwd_drop_f32") == 1
    assert not [n for n in names if n in ("gcn_coef_f32", "row_maps", "scan_short_i32", "csr_filter_fill", "sag_pool_graph_f32",
                                          "sag_pool_graph_bwd_f32", "sag_triplet_gather_f32", "sag_anchor_gather_f32")], names


# ------------------------------------------------------------------------------------------------ 7. refusals
def test_constructor_load_and_mine_refuse(monkeypatch):
    from two_stage_gnn_amd import message_passing as mp, sag_stream as S
    datas = M.datas("small12")
    route = "eager route"
    for kw in ({"conv": "sage"}, {"fused": False}):
        with pytest.raises(TypeError, match=route):
            S.MiniBatchStream(M.net("small12", **kw), datas, 4)
    with pytest.raises(TypeError, match="GPU only.*" + route):
        S.MiniBatchStream(M.net("small12", dev="cpu"), datas, 4)
    with pytest.raises(TypeError, match=route):
        S.MiniBatchStream(object(), datas, 4)
    with pytest.raises(TypeError, match="use_batch=False.*network.py:32.*ONE graph.*" + route):
        S.MiniBatchStream(M.net("small12", use_batch=False), datas, 2)
    assert S.MiniBatchStream(M.net("small12", use_batch=False), datas, 1).B == 1          # (one graph per entry IS the reference's call)
    with monkeypatch.context() as mk:                              # a head outside mp.mlp3_ok at B rows
        mk.setattr(mp, "mlp3_ok", lambda *a: False)
        with pytest.raises(TypeError, match="head.*" + route):
            S.MiniBatchStream(M.net("small12"), datas, 4)
    for B in (0, 129):
        with pytest.raises(ValueError, match="outside 1..128.*" + route):
            S.MiniBatchStream(M.net("small12"), datas, B)
    for kw in (dict(row_cap=63), dict(nnz_cap=1), dict(level_caps=[200, 31, 50, 25]), dict(level_caps=[200, 100, 50]),
               dict(level_caps=[200, 100, 50, 25], row_cap=199)):
        with pytest.raises(ValueError, match=route):
            S.MiniBatchStream(M.net("small12"), datas, 4, **kw)
    with pytest.raises(ValueError, match="label.*" + route):
        S.MiniBatchStream(M.net("small12"), datas, 4, labels=[99] * len(datas))
    m, datas, st = _stream("small12", 4, max_steps=3)
    assert len(st) == 1 and st.position() == 0
    with pytest.raises(RuntimeError, match="no negative to mine"):
        st.mine(None, None, 1.0)
    sched = M.schedule("small12", 4)
    with pytest.raises(ValueError, match="exceeds"):
        st.load(sched)                                             # five entries into a buffer of three
    assert st.load(sched[:3]) == 3
    with pytest.raises(ValueError, match="indices"):
        st.load(np.array([[0, 1, 2, 12]]))
    with pytest.raises(ValueError, match="shape"):
        st.load(np.array([[0, 1, 2]]))
    with pytest.raises(ValueError, match="schedule entry 1 .*" + route):
        st.load(np.array([[0, 1, 2, 3], [10, 10, 10, 10]]))         # four times the largest graph: past the default capacity
    assert st.fits(np.array([[0, 1, 2, 3], [10, 10, 10, 10]])).tolist() == [True, False]
    for bad in (np.zeros(0, dtype=np.int64), np.arange(5), np.array([0.5]), np.array([12])):
        with pytest.raises(ValueError):
            st.eager_loss(bad)
    # the warm-up schedule serves a step: the smallest graph B times
    m2, datas2, st2 = _stream("small12", 4, max_steps=3)
    assert np.isfinite(float(st2.loss()().detach())) and st2.ids_out.tolist() == [0, 0, 0, 0]
    with pytest.raises(ValueError, match="max_steps.*no graph"):
        _stream("dd3", 3, max_steps=2, level_caps=S.k_chain(420, M.RATIO))       # one largest graph: three copies of none fit
