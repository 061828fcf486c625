"""The GAT triplet stream on the GPU (two_stage_gnn_amd/gat_stream.py, csrc/gat_stream.hip): the gather launch alone against
``gat_triplet.assemble`` for every schedule entry, one streamed step per entry against the eager drop-in and against three B = 1 dense
calls of the module, the reference's own fixtures as a dataset, the same steps on poisoned capacity buffers and allocator memory, the
launch trace of a step, no host in the loop, an epoch walked by replays of one hipGraph, and the constructor's refusals.

Datasets, models, schedules and the three-call reference: tests/gat_stream_util.py (margin 10 keeps the hinge active in every entry).
Tolerances are those tests/test_gpu_gat_triplet.py uses for the same node: ``_check_against`` (outputs rtol 1e-4 / atol 1e-5, every
parameter gradient within 5e-3 max|g| + 1e-6) against the module, ``test_drop_in_matches_the_reference_tripletnet``'s against the fixtures."""
import copy

import numpy as np
import pytest
import torch

import gat_stream_util as U
import test_gat_triplet_host as H
from conftest import load_golden
from guard_buf import GUARD, PAT

pytestmark = pytest.mark.gpu

IPAT = -1


def _stream(name, cfg="l2", mode="eval", **kw):
    from two_stage_gnn_amd import gat_stream, gat_triplet
    m = U.model(name, cfg, mode)
    net = gat_triplet.tripletnet(m)
    objs = U.dataset(name)
    return m, net, objs, gat_stream.TripletStream(net, objs, **kw)


def _crit():
    from two_stage_gnn_amd.gat_triplet import MarginRankingLoss
    return MarginRankingLoss(margin=U.MARGIN), torch.full((1,), -1.0, device="cuda")


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


# ------------------------------------------------------------------------------------------------ 1. the gather launch alone
INT_NAMES = ["rowptr", "rowptr_t", "col", "col_t", "src_e_t", "inv", "graph_ptr", "row_graph", "row_slot", "iso_idx", "iso_ptr"]


def _guarded(st):
    """the stream's arrays re-seated in two buffers of its own layout with GUARD words behind every array, every word a NaN (float) /
    -1 (int) pattern -> (ibuf, fbuf, ioff, isz, foff, fsz)"""
    _, _, _, isz, _, fsz = st.g._raw
    a4 = lambda v: (v + 3) // 4 * 4
    ioff = np.concatenate([[0], np.cumsum([a4(s + GUARD) for s in isz])])
    foff = np.concatenate([[0], np.cumsum([a4(s + GUARD) for s in fsz])])
    ibuf = torch.full((int(ioff[-1]),), IPAT, dtype=torch.int32, device="cuda")
    fbuf = torch.full((int(foff[-1]),), PAT, dtype=torch.int32, device="cuda").view(torch.float32)
    st._views(ibuf, fbuf, ioff, isz, foff, fsz)
    return ibuf, fbuf, ioff, isz, foff, fsz


def _read(raw, heads):
    """{array: int32 bit view on the CPU} after checking that nothing outside the arrays was written"""
    ibuf, fbuf, ioff, isz, foff, fsz = raw
    torch.cuda.synchronize()
    out = {}
    for buf, pat, offs, lens, names in ((ibuf.cpu(), IPAT, ioff, isz, INT_NAMES),
                                        (fbuf.view(torch.int32).cpu(), PAT, foff, fsz, ["row_mult", "iso_w", "x"] + ["iso_cols%d" % h for h in heads])):
        keep = torch.ones(buf.numel(), dtype=torch.bool)
        for o, n, name in zip(offs, lens, names):
            keep[int(o):int(o) + n] = False
            out[name] = buf[int(o):int(o) + n].clone()
        assert int(keep.sum()) >= GUARD * len(lens) and bool((buf[keep] == pat).all()), "guard words overwritten"
    return out


def _refill(raw):
    raw[0].fill_(IPAT)
    raw[1].view(torch.int32).fill_(PAT)


@pytest.mark.parametrize("name,cfg", [("small3", "l2"), ("small8", "l3"), ("big", "l2")])
def test_gather_launch_equals_assemble_for_every_entry(name, cfg):
    """every array the launch writes, for every schedule entry, into buffers prefilled with a NaN / -1 pattern: the [:R] / [:E] / [:I]
    parts bit for bit ``gat_triplet.assemble`` of the same three objects; behind them the padding as include/tsgnn.h states it (row
    pointers = E, feature rows +0, row_mult 0, indicator rows 0, row_graph 2, row_slot 0, graph_ptr[3] = R, iso_ptr[3] = I; columns,
    entry maps and the list past E / I not touched); guards intact; ``ids_out`` is the entry; a second launch of the same entry into
    refilled buffers gives the same bits."""
    from two_stage_gnn_amd import gat_triplet as GT, resident as R
    m, net, objs, st = _stream(name, cfg)
    sched = U.schedule(name)
    ar, Rc, heads = st.arena, st.row_cap, st.heads
    assert (st.row_cap, st.nnz_cap, st.iso_cap) == ar.caps and heads == sorted(set(U.MODELS[cfg][1]))
    raw = _guarded(st)
    dev, cache = st.device, R.ResidentCache()
    for rep in range(2):
        st.load(sched)
        runs = []
        for k, ids in enumerate(sched):
            _refill(raw)
            st.gather()
            got = _read(raw, heads)
            assert st.position() == k + 1 and st.ids_out.tolist() == ids.tolist()
            runs.append(got)
            if rep:
                continue
            x, g = GT.assemble([GT.resident_piece(objs[i], dev, cache) for i in ids], dev, heads)
            n, E, I = int(g.n_rows), int(g.nnz), int(g._iso_list[3])
            want = {"rowptr": g.rowptr, "rowptr_t": g._t[0], "graph_ptr": g.graph_ptr, "iso_ptr": g._iso_list[2]}
            for what, t in want.items():
                assert torch.equal(got[what][:t.numel()], t.cpu()), (k, what)
            for what, t in (("col", g.col), ("col_t", g._t[1]), ("src_e_t", g.src_e_t), ("inv", g._inv_e_t)):
                assert torch.equal(got[what][:E], t.cpu()[:E]) and bool((got[what][E:] == IPAT).all()), (k, what)
            for what, t in (("row_graph", g.row_graph), ("row_slot", g.row_slot)):
                assert torch.equal(got[what][:n], t.cpu()[:n]), (k, what)
            assert torch.equal(got["iso_idx"][:I], g._iso_list[0].cpu()[:I]) and bool((got["iso_idx"][I:] == IPAT).all()), (k, "iso_idx")
            assert torch.equal(got["iso_w"][:I], _bits(g._iso_list[1])[:I]) and bool((got["iso_w"][I:] == PAT).all()), (k, "iso_w")
            assert torch.equal(got["row_mult"][:n], _bits(g.row_mult)[:n]) and torch.equal(got["x"][:n * ar.ldf], _bits(x).view(-1)), (k, "x")
            for h in heads:
                assert torch.equal(got["iso_cols%d" % h][:n * h], _bits(g._iso_cols[h]).view(-1)[:n * h]), (k, h)
            # the padding
            assert bool((got["rowptr"][n:] == E).all()) and bool((got["rowptr_t"][n:] == E).all()), (k, "padding rows are empty")
            assert not bool(got["x"][n * ar.ldf:].any()) and not bool(got["row_mult"][n:].any()), (k, "+0")
            assert all(not bool(got["iso_cols%d" % h][n * h:].any()) for h in heads), (k, "indicator")
            assert bool((got["row_graph"][n:] == 2).all()) and not bool(got["row_slot"][n:].any()), (k, "row maps")
            assert got["graph_ptr"].tolist()[3] == n and got["iso_ptr"].tolist()[3] == I
        if rep:
            for a, b in zip(first, runs):
                assert all(torch.equal(a[key], b[key]) for key in a)
        first = runs
    need = ar.records[:, 2:5][sched].sum(1)
    assert need[:, 0].min() < Rc and (name != "big" or need[:, 0].max() == Rc)      # padding rows exist; big also fills the capacity


# ------------------------------------------------------------------------------------------------ 2. the streamed step
def _streamed_entry(m, st, crit, tgt):
    m.zero_grad(set_to_none=True)
    outs = st.embed()
    loss = crit(outs[0], outs[1], tgt)
    loss.backward()
    return outs, loss.detach(), U.grads(m)


def _check_against_module(m, outs, ref):
    """test_gpu_gat_triplet._check_against, on the cached three-call reference"""
    o2, _, g2 = ref
    for a, b in zip(outs, o2):
        torch.testing.assert_close(a, b, rtol=1e-4, atol=1e-5)
    for k, q in m.named_parameters():
        assert (q.grad is None) == (g2[k] is None), k
        if g2[k] is not None:
            bound = 5e-3 * float(g2[k].abs().max()) + 1e-6
            err = float((q.grad - g2[k]).abs().max())
            assert err <= bound, (k, err, bound)


@pytest.mark.parametrize("mode", ["eval", "train"])
@pytest.mark.parametrize("name,cfg", U.CASES)
def test_streamed_step_equals_the_drop_in_and_the_module(name, cfg, mode):
    """every schedule entry from equal parameters (eval mode; training mode with all dropouts 0): distances and embeddings bit for bit
    those of ``tripletnet.forward`` on the same objects (the rows are computed by the same row-local kernels, whatever the row count);
    outputs and every parameter gradient against three B = 1 dense calls of a deep copy of the module at ``_check_against``'s bounds.
    The largest gradient difference to the drop-in is printed: the slab plan of the weight gradients depends on the row count, here
    the capacity, so those sums are not bit for bit.  Every entry is checked against the module, the three of the small schedule that
    name the n = 1 graph or the edge-less graph ([2, 3, 9], [3, 2, 3], [7, 2, 0]) included."""
    m, net, objs, st = _stream(name, cfg, mode)
    sched = U.schedule(name)
    st.load(sched)
    crit, tgt = _crit()
    with_module = 0
    for k, ids in enumerate(sched):
        outs, loss, gs = _streamed_entry(m, st, crit, tgt)
        assert st.ids_out.tolist() == ids.tolist() and float(loss) > 0
        _check_against_module(m, outs, U.three_calls(name, cfg, ids))
        with_module += 1
        m.zero_grad(set_to_none=True)
        outd = net(*[objs[i] for i in ids])
        crit(outd[0], outd[1], tgt).backward()
        gd = U.grads(m)
        worst = max(float((gs[n_] - gd[n_]).abs().max()) for n_ in gd)
        print("%s %s %s entry %d %s: bit-identical outputs %s, max|grad| %.3e, max|streamed - drop-in| gradient entry %.3e"
              % (name, cfg, mode, k, ids.tolist(), [_same_bits(a, b) for a, b in zip(outs, outd)],
                 max(float(v.abs().max()) for v in gd.values()), worst))
        for what, a, b in zip(("dist_p", "dist_n", "embed_a", "embed_p", "embed_n"), outs, outd):
            assert _same_bits(a, b), (k, what, float((a - b).abs().max()))
    assert st.position() == len(sched) and with_module == len(sched)


# ------------------------------------------------------------------------------------------------ 3. the reference's fixtures
@pytest.mark.parametrize("name", H.FIXTURES)
def test_fixture_graphs_as_a_dataset(name):
    """the twelve graphs of a golden are the dataset, its four triplets the schedule: streamed steps meet
    test_drop_in_matches_the_reference_tripletnet's tolerances on outputs, loss and gradients"""
    from two_stage_gnn_amd import gat_encoders as G, gat_stream, gat_triplet as GT
    g = load_golden(name)
    fin, hid, emb, lab = (int(v) for v in g["dims"])
    m = G.DGATEncoderGraph(fin, hid, emb, lab, None, num_layers=int(g["num_layers"]), num_heads=[int(h) for h in g["heads"]],
                           final_dim=str(g["final_dim"]))
    m.load_state_dict({k[2:]: torch.tensor(v) for k, v in g.items() if k.startswith("p.")}, strict=True)
    m = m.cuda()
    objs = [H.GraphObj(a, f, n) for trip in H.triplets(g) for (a, f, n) in trip]
    st = gat_stream.TripletStream(GT.tripletnet(m), objs)
    T = int(g["n_triplets"])
    assert st.load(np.arange(3 * T).reshape(T, 3)) == T == 4
    crit = GT.MarginRankingLoss(margin=float(g["margin"]))
    for t in range(T):
        m.zero_grad(set_to_none=True)
        dp, dn, ea, e_p, en = st.embed()
        loss = crit(dp, dn, torch.full_like(dp, -1.0))
        loss.backward()
        assert st.ids_out.tolist() == [3 * t, 3 * t + 1, 3 * t + 2]
        np.testing.assert_allclose(dp.detach().cpu().numpy(), g["t%d.dist_p" % t], rtol=1e-4, atol=1e-5)
        np.testing.assert_allclose(dn.detach().cpu().numpy(), g["t%d.dist_n" % t], rtol=1e-4, atol=1e-5)
        np.testing.assert_allclose(torch.cat([ea, e_p, en]).detach().cpu().numpy(), g["t%d.embed" % t], rtol=1e-4, atol=1e-5)
        np.testing.assert_allclose(float(loss.detach()), float(g["t%d.loss" % t]), rtol=1e-4, atol=1e-5)
        for k, p in m.named_parameters():
            ref = g["t%d.g.%s" % (t, k)]
            got = p.grad.cpu().numpy() if p.grad is not None else np.zeros_like(ref)
            np.testing.assert_allclose(got, ref, rtol=2e-3, atol=1e-4, err_msg="%d %s" % (t, k))


# ------------------------------------------------------------------------------------------------ 4. poisoned padding
def _poison(nbytes):
    """fill the caching allocator's free memory with NaN: allocate, fill and free tensors of the step's sizes (the allocator hands
    the same blocks to the next step's torch.empty calls)"""
    ts = [torch.empty(max(n // 4, 1), dtype=torch.float32, device="cuda") for n in nbytes for _ in range(3)]
    for t in ts:
        t.fill_(float("nan"))
    torch.cuda.synchronize()
    del ts


@pytest.mark.parametrize("name,cfg", U.CASES)
def test_poisoned_padding_changes_nothing(name, cfg):
    """before every gather both capacity buffers of the stream hold NaN / -1 in every word and torch.empty hands the node memory that
    holds NaN: outputs and every gradient are finite and bit for bit the unpoisoned step's.  A padding row that leaked into a
    weight-gradient slab would put 0 * NaN there"""
    from two_stage_gnn_amd import _native as nat
    m, net, objs, st = _stream(name, cfg, "train")
    sched = U.schedule(name)
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
        st._ibuf.fill_(IPAT)
        st._fbuf.view(torch.int32).fill_(PAT)
        _poison(sizes)
        outs, loss, gs = _streamed_entry(m, st, crit, tgt)
        assert np.isfinite(float(loss)) and all(bool(torch.isfinite(o).all()) for o in outs), (k, ids.tolist())
        assert all(bool(torch.isfinite(g).all()) for g in gs.values()), (k, ids.tolist())
        assert _same_bits(loss, clean[k][1]) and all(_same_bits(a, b) for a, b in zip(outs, clean[k][0])), (k, ids.tolist())
        assert set(gs) == set(clean[k][2])
        for key, g in gs.items():
            assert _same_bits(g, clean[k][2][key]), (key, k, float((g - clean[k][2][key]).abs().max()))


# ------------------------------------------------------------------------------------------------ 5. the launch trace
class _Ops(torch.utils._python_dispatch.TorchDispatchMode):
    """the aten operators torch itself dispatches inside the block (forward and backward)"""

    def __init__(self):
        super().__init__()
        self.names = []

    def __torch_dispatch__(self, func, types, args=(), kwargs=None):
        self.names.append(str(func))
        return func(*args, **(kwargs or {}))


def _traced(fn):
    from two_stage_gnn_amd import _native as nat
    nat.trace = []
    try:
        with _Ops() as ops:
            fn()
        return [t[0] for t in nat.trace], list(ops.names)
    finally:
        nat.trace = None


@pytest.mark.parametrize("name,cfg", [("small3", "l2"), ("small8", "l3"), ("big", "l2")])
def test_launch_trace_of_a_streamed_step(name, cfg):
    """the library launches of a streamed step are those of the resident drop-in step on the same objects with ``gat_assemble_f32``
    replaced by ``gat_triplet_gather_f32``: no capacity form of any layer kernel was needed.  Torch's own operators in the step are
    among those of the resident step's ``embed`` + loss + backward, count by count (that step also zeroes the readout's workspace
    of its new batch; the only copies are autograd's, of a gradient into ``.grad``); none is a concatenation, an index, a gather or a scatter operator"""
    m, net, objs, st = _stream(name, cfg, "train")
    sched = U.schedule(name)
    st.load(sched)
    crit, tgt = _crit()
    trip = [objs[i] for i in sched[0]]
    for _ in range(2):                                            # (warm: allocator, library load, the resident pieces)
        m.zero_grad(set_to_none=True)
        crit(*net(*trip)[:2], tgt).backward()
    st.loss(crit, tgt)().backward()                               # (... and the stream's views of its schedule buffer)
    st.load(sched)
    m.zero_grad(set_to_none=True)
    box = {}

    def resident():
        box["b"] = net.batch(*trip)
    asm, _ = _traced(resident)
    res, res_ops = _traced(lambda: crit(*net.embed(box["b"])[:2], tgt).backward())
    m.zero_grad(set_to_none=True)
    got, got_ops = _traced(lambda: st.loss(crit, tgt)().backward())
    print("library launches of a streamed GAT step (%s %s): %d\n%s\ntorch operators: %s" % (name, cfg, len(got), " ".join(got), " ".join(got_ops)))
    assert asm == ["gat_assemble_f32"]
    assert got == ["gat_triplet_gather_f32"] + res
    assert got.count("gat_attn_fwd_f32") == U.MODELS[cfg][0] and "readout_max_fwd_f32" in got
    from collections import Counter
    assert not Counter(got_ops) - Counter(res_ops), Counter(got_ops) - Counter(res_ops)
    assert not [o for o in got_ops if any(w in o for w in ("cat", "index", "stack", "gather", "scatter"))]
    assert got_ops.count("aten.copy_.default") == res_ops.count("aten.copy_.default") <= sum(1 for p in m.parameters() if p.grad is not None)


# ------------------------------------------------------------------------------------------------ 6. no host in the loop
def test_no_host_in_the_loop():
    """after one warm call, forward + backward of two streamed steps under sync debug mode "error" """
    m, net, objs, st = _stream("small8", "l2", "train")
    st.load(U.schedule("small8"))
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


# ------------------------------------------------------------------------------------------------ 7. replays
@pytest.mark.parametrize("name,cfg", [("small8", "l2"), ("big", "l2")])
def test_replays_walk_the_schedule_and_move_the_parameters_as_uncaptured_steps(name, cfg):
    """``GraphedStep(FlatTrainer(...), st.loss(...))``: T replays walk the schedule (``ids_out`` per replay, ``position() == T``) and
    move the parameters as T uncaptured streamed steps of a deep-copied model do — the same route, so rtol 1e-5 / atol 1e-6 (the
    sibling streams' bound for this comparison); a second ``load`` restarts the walk at 0"""
    from two_stage_gnn_amd import gat_stream, gat_triplet, message_passing as mp
    from two_stage_gnn_amd.data_parallel import FlatTrainer, GraphedStep
    sched = U.schedule(name)
    T = len(sched)
    m1, net1, objs, st1 = _stream(name, cfg, "train")
    m2 = copy.deepcopy(m1)
    start = {k: v.detach().clone() for k, v in m1.state_dict().items()}
    crit, tgt = _crit()
    st2 = gat_stream.TripletStream(gat_triplet.tripletnet(m2), objs)
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
    assert st1.position() == T == len(st1) and np.isfinite(gs.loss_value())
    mp.check_device_errors()
    moved = 0
    for (k, p1), (_, p2) in zip(m1.named_parameters(), m2.named_parameters()):
        torch.testing.assert_close(p1.detach(), p2.detach(), rtol=1e-5, atol=1e-6, msg=lambda s_, k=k: k + ": " + s_)
        moved += int(not torch.equal(p1.detach(), start[k]))
    assert moved >= 8
    assert st1.load(sched[::-1].copy()[:3]) == 3 and st1.position() == 0        # a second load restarts the walk
    gs.step()
    gs.synchronize()
    assert st1.position() == 1 and st1.ids_out.tolist() == sched[-1].tolist()


# ------------------------------------------------------------------------------------------------ 8. refusals
def test_constructor_and_load_refuse(monkeypatch):
    from two_stage_gnn_amd import gat_fused, gat_stream, gat_triplet, resident
    from two_stage_gnn_amd import gat_encoders as G
    objs = U.dataset("small8")
    eager = "eager drop-in, tripletnet.forward\\(a, p, n\\)$"
    with pytest.raises(TypeError, match="gat_triplet.tripletnet.*" + eager):
        gat_stream.TripletStream(object(), objs)
    with pytest.raises(TypeError, match="gat_triplet.tripletnet.*" + eager):
        gat_stream.TripletStream(U.model("small8", "l2"), objs)                 # the bare encoder
    with pytest.raises(TypeError, match="GPU only.*" + eager):
        gat_stream.TripletStream(gat_triplet.tripletnet(U.model("small8", "l2", dev="cpu")), objs)
    with monkeypatch.context() as mk:
        mk.setattr(resident, "RESIDENT", False)
        with pytest.raises(TypeError, match="RESIDENT.*" + eager):
            gat_stream.TripletStream(gat_triplet.tripletnet(U.model("small8", "l2")), objs)
    with monkeypatch.context() as mk:                              # a layer whose heads fail gat_fused.heads_ok (TSGNN_GAT_FUSED=0)
        mk.setattr(gat_fused, "FUSED", False)
        with pytest.raises(TypeError, match="heads_ok.*" + eager):
            gat_stream.TripletStream(gat_triplet.tripletnet(U.model("small8", "l2")), objs)
    five = G.DGATEncoderGraph(8, 8, 8, 2, None, num_layers=6, num_heads=[1, 2, 3, 4, 5, 5], neg_input_slopes=[0.2] * 6, dropouts=[0.0] * 6,
                              final_dim="output_dim").cuda()
    with pytest.raises(TypeError, match="four distinct head counts.*" + eager):
        gat_stream.TripletStream(gat_triplet.tripletnet(five), objs)
    deep = G.DGATEncoderGraph(8, 8, 8, 2, None, num_layers=5, num_heads=[2] * 5, neg_input_slopes=[0.2] * 5, dropouts=[0.0] * 5,
                              final_dim="output_dim").cuda()
    with pytest.raises(TypeError, match="at most 4 layers.*" + eager):      # (gat_fused.pack_layers takes four)
        gat_stream.TripletStream(gat_triplet.tripletnet(deep), objs)
    for mode in ("eval", "train"):                                 # dropout > 0 is refused whatever the mode
        with pytest.raises(TypeError, match="dropout.*" + eager):
            gat_stream.TripletStream(gat_triplet.tripletnet(U.model("small8", "l2", mode, dropouts=[0.0, 0.3])), objs)
    with pytest.raises(ValueError, match="3 features per node, the model takes 8"):
        gat_stream.TripletStream(gat_triplet.tripletnet(U.model("small8", "l2")), U.dataset("small3"))
    bad = list(objs)
    bad[4] = H.make_obj(4, 5, nmax=U.NMAX_SMALL, fin=8)
    bad[4].graph["feats"][9, 1] = 0.5
    with pytest.raises(ValueError, match="graph 4: one representative"):
        gat_stream.TripletStream(gat_triplet.tripletnet(U.model("small8", "l2")), bad)
    m, net, objs, st = _stream("small8", max_steps=4)
    assert len(st) == 1 and st.position() == 0
    with pytest.raises(ValueError, match="exceeds"):
        st.load(U.schedule("small8"))                              # ten entries into a buffer of four
    assert st.load(U.schedule("small8")[:4]) == 4
    with pytest.raises(ValueError, match="indices"):
        st.load(np.array([[0, 1, 11]]))
    # the warm-up schedule serves a step: graph 0 three times
    crit, tgt = _crit()
    m2, net2, objs2, st2 = _stream("small8", max_steps=4)
    assert np.isfinite(float(st2.loss(crit, tgt)())) and st2.ids_out.tolist() == [0, 0, 0]
    # dropout that turns up after construction: embed() refuses
    for hd in m2.modules():
        if isinstance(hd, G.DGATHead):
            hd.dropout = 0.25
    m2.train()
    with pytest.raises(RuntimeError, match="dropout.*" + eager):
        st2.embed()
    with pytest.raises(RuntimeError, match="load"):
        st3 = gat_stream.TripletStream(gat_triplet.tripletnet(U.model("small8", "l2")), objs)
        st3.gather()
