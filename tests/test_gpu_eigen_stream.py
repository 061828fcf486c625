"""The EigenGCN triplet stream on the GPU (two_stage_gnn_amd/eigen_stream.py, csrc/eigen_stream.hip, the capacity form of
csrc/eigen_pool.hip): the gather launch alone against ``eigen_triplet.assemble`` and the padding rules for every schedule entry, the
capacity pooling launch alone, one streamed step per entry against the eager drop-in and the fp64 restatement, the reference's own
fixtures as datasets, the same steps on poisoned capacity buffers and allocator memory, the launch trace of a step, no host in the
loop, an epoch walked by replays of one hipGraph, and the constructor's refusals.

Datasets, models, schedules and references: tests/eigen_stream_util.py (margin 10 keeps the hinge active in every entry).  Bounds
against float64 are tests/test_gpu_eigen_triplet.py's ``_check``: 1e-5 of a tensor's largest entry on outputs, 1e-4 on gradients, or
10 x what the same computation in fp32 on the CPU misses fp64 by, with ``_db2_floor`` for the last bias."""
import copy
from collections import Counter

import numpy as np
import pytest
import torch

import eigen_ref as ER
import eigen_stream_util as U
import eigen_two_stage_util as EU
import test_eigen_triplet_host as H
import test_gpu_eigen_triplet as GT
from guard_buf import GUARD, PAT, Out

pytestmark = pytest.mark.gpu


def _stream(data, name, var="base", mode="train", **kw):
    from two_stage_gnn_amd import eigen_stream, eigen_triplet
    m = U.model(data, name, var, mode)
    net = eigen_triplet.tripletnet(m, H.args_of(U.cfg(data, name, var)))
    objs = U.dataset(data, name)
    return m, net, objs, eigen_stream.TripletStream(net, objs, **kw)


def _crit():
    from two_stage_gnn_amd.eigen_triplet import MarginRankingLoss
    return MarginRankingLoss(margin=U.MARGIN), torch.full((1,), -1.0, device="cuda")


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


# ------------------------------------------------------------------------------------------------ 1. the gather launch alone
def _names(L):
    ints = [k % i for i in range(L + 1) for k in ("rowptr_%d", "col_%d", "graph_ptr_%d", "row_graph_%d", "row_slot_%d", "slot_count_%d")]
    ints += [k % i for i in range(L) for k in ("cluster_of_%d", "bptr_%d", "members_%d")]
    return ints, ["val_%d" % i for i in range(L + 1)] + ["coef_%d" % i for i in range(L)] + ["final", "x"]


def _guarded(st):
    """the stream's arrays re-seated in two buffers of its own layout with GUARD words behind every array, every word a NaN (float) /
    IPAT (int) pattern"""
    ioff, isz, foff, fsz = st.layout(guard=GUARD)
    ibuf = torch.full((int(ioff[-1]),), U.IPAT, dtype=torch.int32, device="cuda")
    fbuf = torch.full((int(foff[-1]),), PAT, dtype=torch.int32, device="cuda").view(torch.float32)
    st._views(ibuf, fbuf, ioff, isz, foff, fsz)
    return ibuf, fbuf, ioff, isz, foff, fsz


def _read(raw, L):
    """{array: int32 bit view on the CPU} after checking that nothing outside the arrays was written"""
    ibuf, fbuf, ioff, isz, foff, fsz = raw
    torch.cuda.synchronize()
    out = {}
    inames, fnames = _names(L)
    for buf, pat, offs, lens, names in ((ibuf.cpu(), U.IPAT, ioff, isz, inames), (fbuf.view(torch.int32).cpu(), PAT, foff, fsz, fnames)):
        assert len(names) == len(lens)
        keep = torch.ones(buf.numel(), dtype=torch.bool)
        for o, n, name in zip(offs, lens, names):
            keep[int(o):int(o) + n] = False
            out[name] = buf[int(o):int(o) + n].clone()
        assert int(keep.sum()) >= GUARD * len(lens) and bool((buf[keep] == pat).all()), "guard words overwritten"
    return out


def _expected_bits(a):
    """an array of ``eigen_stream_util.gather_numpy`` as the int32 words the guarded buffer must hold (a NaN: the prefill pattern)"""
    a = np.ascontiguousarray(a).reshape(-1)
    if a.dtype == np.float32:
        w = a.view(np.int32).copy()
        w[np.isnan(a)] = PAT
        return torch.from_numpy(w)
    return torch.from_numpy(a.astype(np.int32))


@pytest.mark.parametrize("data,name", U.GATHER_CASES)
def test_gather_launch_equals_assemble_and_pads_as_specified(data, name):
    """every array the launch writes, for every schedule entry, into guarded buffers prefilled with a NaN / -7 pattern: the [:R_i] /
    [:E_i] prefixes bit for bit ``eigen_triplet.assemble`` of the three resident pieces; EVERY word equal to the restatement
    ``eigen_stream_util.gather_numpy`` (rowptr_i behind R_i = E_i up to row_cap_i + Nmax, graph_ptr_i[3] = R_i, row_graph 2, row_slot 0,
    cluster_of -1, coef / final / x rows +0, slot counts, bptr_i behind the closing entry = R_i; col_i, val_i past E_i and members_i past
    R_i still hold the prefill pattern); guards intact; ``ids_out`` is the entry; a second walk gives the same bits"""
    from two_stage_gnn_amd import eigen_triplet as ET, resident as R
    m, net, objs, st = _stream(data, name)
    sched = U.schedule(data)
    ar = st.arena
    L, J, Jf = ar.L, ar.J, ar.Jf
    assert (st.row_caps, st.nnz_caps) == ar.caps
    raw = _guarded(st)
    dev, cache = st.device, R.ResidentCache()
    first = None
    for rep in range(2):
        st.load(sched)
        runs = []
        for k, ids in enumerate(sched):
            raw[0].fill_(U.IPAT)
            raw[1].view(torch.int32).fill_(PAT)
            st.gather()
            got = _read(raw, L)
            assert st.position() == k + 1 and st.ids_out.tolist() == ids.tolist()
            runs.append(got)
            if rep:
                continue
            want, Rr, E = U.gather_numpy(ar, ids)
            for key, w in want.items():
                if w is not None:
                    assert torch.equal(got[key], _expected_bits(w)), (k, ids.tolist(), key)
            x, eb = ET.assemble([ET.resident_graph(objs[i], dev, cache, L, J, Jf) for i in ids], dev)
            arrs = EU.batch_arrays(eb, x)
            for key, t in arrs.items():
                if t is None:
                    continue
                t = _bits(t).view(-1)
                lv = int(key[-1]) if key[-1].isdigit() else 0
                if key.startswith("rowptr"):
                    t = t[:Rr[lv] + 1]
                elif key.startswith(("col", "val")):
                    t = t[:E[lv]]
                elif key.startswith("bptr"):
                    t = t[:Rr[lv + 1] + 4]
                elif key == "x":
                    t = t[:Rr[0] * ar.ldf]
                assert t.numel() > 0 or key.startswith(("col", "val")), key
                assert torch.equal(got[key][:t.numel()], t), (k, ids.tolist(), key)
        if rep:
            for a, b in zip(first, runs):
                assert all(torch.equal(a[key], b[key]) for key in a)
        first = runs


# ------------------------------------------------------------------------------------------------ 2. the capacity pooling launch alone
@pytest.mark.parametrize("ghost_mode", [1, 2])
@pytest.mark.parametrize("J", [1, 5])
@pytest.mark.parametrize("C", [12, 128])
def test_pool_fwd_cap_alone(C, J, ghost_mode):
    """tsgnn_eigen_pool_fwd_cap_f32 through the C ABI on three graphs (one with unassigned rows, one with ONE cluster) whose pooled
    level has 7 padding rows: real rows, readout and winners bit for bit tsgnn_eigen_pool_fwd_f32's; padding and ghost rows +0; the
    columns beyond J C of a wider leading dimension and the guard untouched; real rows against tests/eigen_ref.py's ``pool`` in
    float64 at the bound of tests/test_gpu_eigen_pool.py (rtol = atol = 1e-5)"""
    from two_stage_gnn_amd import _native as nat, eigen_pool as ep
    rng = np.random.default_rng(C + J + ghost_mode)
    nmax, sizes = 19, [13, 19, 9]
    res = [EU.make_result(rng, n, [3], unassigned=(b == 0), one_cluster=(b == 2)) for b, n in enumerate(sizes)]
    eb = ep.collate(res, nmax, J, 0)
    g, lv = eb.g0, eb.levels[0]
    g1 = lv.g
    K, pad, ldo = int(g1.n_rows), 7, J * C + 4
    z = torch.from_numpy(rng.standard_normal((g.n_rows + nmax, C)).astype(np.float32)).cuda()
    if ghost_mode == 1:
        z[g.n_rows:] = 0.0
    plain = torch.full((K + nmax, J * C), float("nan"), device="cuda")
    ro = [torch.empty(3, C, device="cuda") for _ in range(2)]
    arg = [torch.empty(3, C, dtype=torch.int32, device="cuda") for _ in range(2)]
    nat.call("eigen_pool_fwd_f32", z, z.stride(0), C, g.graph_ptr, 3, nmax, g.n_rows, ghost_mode, g1.graph_ptr, lv.bptr, lv.members, lv.coef, J, 0,
             plain, plain.stride(0), K, nmax, None, ro[0], C, arg[0])
    out = Out(K + pad + nmax, ldo)
    nat.call("eigen_pool_fwd_cap_f32", z, z.stride(0), C, g.graph_ptr, 3, nmax, g.n_rows, ghost_mode, g1.graph_ptr, lv.bptr, lv.members, lv.coef,
             J, 0, out.mat, ldo, K + pad, nmax, None, ro[1], C, arg[1])
    owned = torch.zeros(K + pad + nmax, ldo, dtype=torch.bool)
    owned[:, :J * C] = True
    out.rest_untouched("eigen_pool_fwd_cap", owned)
    got = out.mat[:, :J * C]
    assert bool((_bits(got) != PAT).all()), "a row of the capacity form stayed unwritten"
    assert _same_bits(got[:K], plain[:K]) and _same_bits(ro[0], ro[1]) and torch.equal(arg[0], arg[1])
    assert not bool(_bits(got[K:]).any()) and not bool(_bits(plain[K:]).any())             # padding and ghost rows: +0
    with pytest.raises(RuntimeError):                                                       # pooled levels only
        nat.call("eigen_pool_fwd_cap_f32", z, z.stride(0), C, g.graph_ptr, 3, nmax, g.n_rows, ghost_mode, None, None, None, lv.coef, J, 1,
                 out.mat, ldo, 0, 0, plain, None, 0, None)
    _, _, _, _, pm = ep.dense_inputs(res, nmax, J, 0)
    x64 = torch.zeros(3, nmax, C, dtype=torch.float64)
    gp = g.graph_ptr.cpu().tolist()
    for b in range(3):
        x64[b, :sizes[b]] = z[gp[b]:gp[b + 1]].cpu().double()
    y64 = ER.pool(pm[0], x64)
    gp1 = g1.graph_ptr.cpu().tolist()
    for b in range(3):
        np.testing.assert_allclose(got[gp1[b]:gp1[b + 1]].cpu().double().numpy(), y64[b, :gp1[b + 1] - gp1[b]].numpy(), rtol=1e-5, atol=1e-5)
        assert not bool(y64[b, gp1[b + 1] - gp1[b]:].any())


# ------------------------------------------------------------------------------------------------ 3. the streamed step
def _streamed_entry(m, st, crit, tgt):
    m.zero_grad(set_to_none=True)
    outs = st.embed()
    loss = crit(outs[0], outs[1], tgt)
    loss.backward()
    return outs, loss.detach(), U.grads(m)


def _check_against_fp64(tag, m, outs, loss, ref, cancel=None):
    """``cancel`` (entries whose positive and negative are one graph: every exact gradient is zero):
    ``eigen_stream_util.cancelling_scale``, the size of the two parts that cancel; 1e-4 of it is the floor"""
    r64, r32 = ref[torch.float64], ref[torch.float32]
    GT._check(tag + " dist_p", outs[0], r64[0], r32[0], 1e-5)
    GT._check(tag + " dist_n", outs[1], r64[1], r32[1], 1e-5)
    for b in range(3):
        GT._check(tag + " embed %d" % b, outs[2 + b], r64[2][b], r32[2][b], 1e-5)
    GT._check(tag + " loss", loss, r64[3], r32[3], 1e-5)
    last_bias = [k for k in r64[4] if k.startswith("pred_model") and k.endswith("bias")][-1]
    for k, q in m.named_parameters():
        assert q.grad is not None, k
        floor = GT._db2_floor(1.0, 1.0) if k == last_bias else 0.0
        if cancel is not None:
            assert not bool(r64[4][k].any()) and not bool(r32[4][k].any()), k     # (the case the floor is for, and no other)
            floor += 1e-4 * cancel[k]
        GT._check(tag + " " + k, q.grad, r64[4][k], r32[4][k], 1e-4, floor=floor)


@pytest.mark.parametrize("data,name,var", U.CASES)
def test_streamed_step_equals_the_drop_in_and_the_restatement(data, name, var):
    """every schedule entry from equal parameters: distances and embeddings bit for bit those of ``tripletnet.forward`` on the same
    objects (every row is computed by the same row-local or per-graph kernels whatever the row count; no kernel on the forward path
    picks its summation order from the row count); outputs, loss and every parameter gradient against
    ``test_eigen_triplet_host.ref_step`` in float64 under ``test_gpu_eigen_triplet._check``.  The largest gradient difference to the
    drop-in is printed, not asserted: the split-K plan of the weight gradients depends on the row count, here the capacity.
    Entries whose positive and negative are the same graph ([i, i, i] and [3, 2, 2]) have exactly zero gradients, where ``_check``'s
    relative rule allows nothing: they get the floor of ``eigen_stream_util.cancelling_scale`` (the drop-in on the same objects
    leaves the same rounding: up to 1.2e-7 on conv_first.weight of the small dataset, measured)."""
    m, net, objs, st = _stream(data, name, var)
    sched = U.schedule(data)
    st.load(sched)
    crit, tgt = _crit()
    for k, ids in enumerate(sched):
        outs, loss, gs = _streamed_entry(m, st, crit, tgt)
        assert st.ids_out.tolist() == ids.tolist() and float(loss) > 0
        _check_against_fp64("%s %s %s entry %d" % (data, name, var, k), m, outs, loss, U.ref_step(data, name, var, ids),
                            cancel=U.cancelling_scale(data, name, var, ids[1]) if ids[1] == ids[2] else None)
        m.zero_grad(set_to_none=True)
        outd = net(*[objs[i] for i in ids])
        crit(outd[0], outd[1], tgt).backward()
        gd = U.grads(m)
        worst = max(float((gs[n_] - gd[n_]).abs().max()) for n_ in gd)
        print("%s %s %s entry %d %s: bit-identical outputs %s, max|grad| %.3e, max|streamed - drop-in| gradient entry %.3e"
              % (data, name, var, k, ids.tolist(), [_same_bits(a, b) for a, b in zip(outs, outd)],
                 max(float(v.abs().max()) for v in gd.values()), worst))
        for what, a, b in zip(("dist_p", "dist_n", "embed_a", "embed_p", "embed_n"), outs, outd):
            assert _same_bits(a, b), (k, what, float((a - b).abs().max()))
    assert st.position() == len(sched)


# ------------------------------------------------------------------------------------------------ 4. the reference's fixtures
def test_fixture_list():
    assert len(H.NAMES) == 6


@pytest.mark.parametrize("name", H.NAMES)
def test_fixture_graphs_as_a_dataset(name):
    """the three graphs of a golden (symmetric at every level: checked here on the CPU) are the dataset, its triplet the schedule:
    the streamed step meets test_drop_in_matches_the_reference_tripletnet's tolerances on outputs, loss and gradients"""
    from two_stage_gnn_amd import eigen_stream, eigen_triplet as ET
    g = H.load(name)
    c = H.cfg(g)
    m = GT._model(c)
    m.load_state_dict({k[2:]: torch.tensor(v) for k, v in g.items() if k.startswith("p.")}, strict=True)
    dicts, _ = H.graph_dicts(g)
    L = len(c["pool_sizes"])
    for d in dicts:
        assert all(s[3] for s in ET.pack_host(d, L, c["J"], c["Jf"])["graphs"])
    objs = [H.GraphObj(d) for d in dicts]
    st = eigen_stream.TripletStream(ET.tripletnet(m, H.args_of(c)), objs)
    ids = [0, 0, 2] if c["same_ap"] else [0, 1, 2]
    assert st.load(np.array([ids])) == 1
    dp, dn, ea, e_p, en = st.embed()
    loss = ET.MarginRankingLoss(margin=c["margin"])(dp, dn, torch.full_like(dp, -1.0))
    loss.backward()
    assert st.ids_out.tolist() == ids and float(loss) > 0
    np.testing.assert_allclose(dp.detach().cpu().numpy(), g["dist_p"], rtol=1e-4, atol=1e-4)
    np.testing.assert_allclose(dn.detach().cpu().numpy(), g["dist_n"], rtol=1e-4, atol=1e-4)
    np.testing.assert_allclose(torch.cat([ea, e_p, en]).detach().cpu().numpy(), g["embed"], rtol=1e-4, atol=1e-4)
    assert abs(float(loss.detach()) - float(g["loss"])) < 1e-4
    for k, p in m.named_parameters():
        ref = g["g." + k]
        got = p.grad.cpu().numpy() if p.grad is not None else np.zeros_like(ref)
        np.testing.assert_allclose(got, ref, rtol=2e-3, atol=2e-4, err_msg=k)


# ------------------------------------------------------------------------------------------------ 5. poisoned padding
def _poison(nbytes):
    """fill the caching allocator's free memory with NaN: allocate, fill and free tensors of the step's sizes (the allocator hands
    the same blocks to the next step's torch.empty calls)"""
    ts = [torch.empty(max(n // 4, 1), dtype=torch.float32, device="cuda") for n in nbytes for _ in range(3)]
    for t in ts:
        t.fill_(float("nan"))
    torch.cuda.synchronize()
    del ts


@pytest.mark.parametrize("data,name,var", [("small", "l1_j2_f1", "base"), ("small", "l2_j1", "nomask"), ("small", "l1_j2_f2", "nocon"),
                                           ("big", "big", "base")])
def test_poisoned_padding_changes_nothing(data, name, var):
    """before every gather both capacity buffers of the stream hold NaN / -7 in every word and torch.empty hands the step memory that
    holds NaN: outputs and every gradient are finite and bit for bit the unpoisoned step's.  A padding row that leaked into a
    weight-gradient sum would put 0 * NaN there (the pooled rows behind the batch are the capacity pooling launch's to zero)"""
    from two_stage_gnn_amd import _native as nat
    m, net, objs, st = _stream(data, name, var)
    sched = U.schedule(data)
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
        st._ibuf.fill_(U.IPAT)
        st._fbuf.view(torch.int32).fill_(PAT)
        _poison(sizes)
        outs, loss, gs = _streamed_entry(m, st, crit, tgt)
        assert float(loss) > 0 and np.isfinite(float(loss)) and all(bool(torch.isfinite(o).all()) for o in outs), (k, ids.tolist())
        assert all(bool(torch.isfinite(g).all()) for g in gs.values()), (k, ids.tolist())
        assert _same_bits(loss, clean[k][1]) and all(_same_bits(a, b) for a, b in zip(outs, clean[k][0])), (k, ids.tolist())
        assert set(gs) == set(clean[k][2])
        for key, g in gs.items():
            assert _same_bits(g, clean[k][2][key]), (key, k, float((g - clean[k][2][key]).abs().max()))


# ------------------------------------------------------------------------------------------------ 6. the launch trace
def _traced(fn):
    from two_stage_gnn_amd import _native as nat
    nat.trace = []
    try:
        fn()
        return [t[0] for t in nat.trace]
    finally:
        nat.trace = None


@pytest.mark.parametrize("data,name", [("small", "l1_j2_f1"), ("small", "l2_j1"), ("big", "big")])
def test_launch_trace_of_a_streamed_step(data, name):
    """the library launches of a streamed step are those of the resident drop-in step (``embed`` of a batch from ``batch()`` + loss +
    backward) on the same objects with ``eigen_triplet_gather_f32`` in front and the capacity entry in place of the plain pooling
    forward of every pooled level (the final pooling keeps the plain one): no other kernel needed a capacity form"""
    m, net, objs, st = _stream(data, name)
    sched = U.schedule(data)
    st.load(sched)
    crit, tgt = _crit()
    trip = [objs[i] for i in sched[0]]
    for _ in range(2):                                            # (warm: allocator, library load, the resident pieces)
        m.zero_grad(set_to_none=True)
        crit(*net(*trip)[:2], tgt).backward()
    st.loss(crit, tgt)().backward()
    st.load(sched)
    m.zero_grad(set_to_none=True)
    b = net.batch(*trip)
    res = _traced(lambda: crit(*net.embed(b)[:2], tgt).backward())
    m.zero_grad(set_to_none=True)
    got = _traced(lambda: st.loss(crit, tgt)().backward())
    print("library launches of a streamed EigenGCN step (%s %s): %d\n%s" % (data, name, len(got), " ".join(got)))
    L = st.arena.L
    want, left = [], L
    for n_ in res:
        if n_ == "eigen_pool_fwd_f32" and left:
            want.append("eigen_pool_fwd_cap_f32")
            left -= 1
        else:
            want.append(n_)
    assert left == 0 and got == ["eigen_triplet_gather_f32"] + want
    assert got.count("eigen_pool_fwd_cap_f32") == L and got.count("eigen_pool_fwd_f32") == res.count("eigen_pool_fwd_f32") - L
    assert Counter(got)["eigen_pool_bwd_f32"] == Counter(res)["eigen_pool_bwd_f32"]


# ------------------------------------------------------------------------------------------------ 7. no host in the loop
def test_no_host_in_the_loop():
    """after one warm call, forward + backward of two streamed steps under sync debug mode "error" """
    m, net, objs, st = _stream("small", "l1_j2_f1")
    st.load(U.schedule("small"))
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
    assert st.position() == 3 and np.isfinite(float(loss.detach())) and float(loss.detach()) > 0
    assert all(bool(torch.isfinite(p.grad).all()) for p in m.parameters() if p.grad is not None)


# ------------------------------------------------------------------------------------------------ 8. replays
@pytest.mark.parametrize("data,name", [("small", "l1_j2_f1"), ("big", "big")])
def test_replays_walk_the_schedule_and_move_the_parameters_as_uncaptured_steps(data, name):
    """``GraphedStep(FlatTrainer(...), st.loss(...))``: T replays walk the schedule (``ids_out`` per replay, ``position() == T``) and
    move the parameters as T uncaptured streamed steps of a deep-copied model do — the same route, so rtol 1e-5 / atol 1e-6 (the
    sibling streams' bound for this comparison); a second ``load`` restarts the walk at 0"""
    from two_stage_gnn_amd import eigen_stream, eigen_triplet, message_passing as mp
    from two_stage_gnn_amd.data_parallel import FlatTrainer, GraphedStep
    sched = U.schedule(data)
    T = len(sched)
    m1, net1, objs, st1 = _stream(data, name)
    m2 = copy.deepcopy(m1)
    start = {k: v.detach().clone() for k, v in m1.state_dict().items()}
    crit, tgt = _crit()
    st2 = eigen_stream.TripletStream(eigen_triplet.tripletnet(m2, H.args_of(U.cfg(data, name))), objs)
    st2.load(sched)
    tr2 = FlatTrainer(m2, lr=1e-4, clip=2.0)
    step2 = st2.loss(crit, tgt)
    for ids in sched:
        assert float(tr2.step(step2).detach()) > 0
        assert st2.ids_out.tolist() == ids.tolist()
    st1.load(sched)
    gs = GraphedStep(FlatTrainer(m1, lr=1e-4, clip=2.0), st1.loss(crit, tgt))     # (its warm-up steps consume entries and are rolled back ...)
    assert gs.describe().startswith("one graph"), gs.describe()
    st1.load(sched)                                                             # ... so the epoch starts here: cursor := 0
    for ids in sched:
        gs.step()
        gs.synchronize()
        assert st1.ids_out.tolist() == ids.tolist() and gs.loss_value() > 0
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


# ------------------------------------------------------------------------------------------------ 9. refusals
def test_constructor_and_load_refuse(monkeypatch):
    from two_stage_gnn_amd import eigen_encoders as EE, eigen_stream, eigen_triplet, resident
    objs = U.dataset("small", "l1_j2_f1")
    args = H.args_of(U.cfg("small", "l1_j2_f1"))
    tn = lambda m: eigen_triplet.tripletnet(m, args)
    eager = "eager drop-in, tripletnet.forward\\(a, p, n\\)$"
    with pytest.raises(TypeError, match="eigen_triplet.tripletnet.*" + eager):
        eigen_stream.TripletStream(object(), objs)
    with pytest.raises(TypeError, match="eigen_triplet.tripletnet.*" + eager):
        eigen_stream.TripletStream(U.model("small", "l1_j2_f1"), objs)          # the bare encoder
    with pytest.raises(TypeError, match="GPU only.*" + eager):
        eigen_stream.TripletStream(tn(U.model("small", "l1_j2_f1", dev="cpu")), objs)
    with monkeypatch.context() as mk:
        mk.setattr(resident, "RESIDENT", False)
        with pytest.raises(TypeError, match="RESIDENT.*" + eager):
            eigen_stream.TripletStream(tn(U.model("small", "l1_j2_f1")), objs)
    for mode in ("eval", "train"):                                 # dropout > 0 is refused whatever the mode
        with pytest.raises(TypeError, match="dropout.*" + eager):
            eigen_stream.TripletStream(tn(U.model("small", "l1_j2_f1", mode=mode, dropout=0.3)), objs)
    dps, dJ, dJf = EU.DEEP["l4_j1_f1"]
    c = dict(U.cfg("small", "l1_j1"), pool_sizes=list(dps), J=dJ, Jf=dJf)
    deep = EE.WavePoolingGcnEncoder(c["nmax"], 6, 16, 16, 6, 3, num_pool_matrix=dJ, num_pool_final_matrix=dJf, pool_sizes=list(dps),
                                    pred_hidden_dims=[50], args=H.args_of(c)).cuda()
    with pytest.raises(TypeError, match="up to 3 pooling levels.*" + eager):
        eigen_stream.TripletStream(eigen_triplet.tripletnet(deep, H.args_of(c)), objs)
    with pytest.raises(ValueError, match="8 features per node, the model takes 6"):
        c8 = U.cfg("small", "l1_j2_f1")
        eigen_stream.TripletStream(tn(U.model("small", "l1_j2_f1")), [EU.GraphObj(EU.make_dict(
            EU.make_result(np.random.default_rng(1), 9, c8["pool_sizes"]), np.random.default_rng(2), EU.NMAX, c8["J"], c8["Jf"], 8))])
    with pytest.raises(ValueError, match="graph 1: the graph dict has no"):     # whatever pack_arena refuses
        eigen_stream.TripletStream(tn(U.model("small", "l1_j2_f1")), [objs[0], U.dataset("small", "l1_j1")[1]])
    m, net, objs, st = _stream("small", "l1_j2_f1", max_steps=4)
    assert len(st) == 1 and st.position() == 0
    with pytest.raises(ValueError, match="exceeds"):
        st.load(U.schedule("small"))                               # ten entries into a buffer of four
    assert st.load(U.schedule("small")[:4]) == 4
    with pytest.raises(ValueError, match="indices"):
        st.load(np.array([[0, 1, 12]]))
    # the warm-up schedule serves a step: graph 0 three times
    crit, tgt = _crit()
    m2, net2, objs2, st2 = _stream("small", "l1_j2_f1", max_steps=4)
    assert float(st2.loss(crit, tgt)()) > 0 and st2.ids_out.tolist() == [0, 0, 0]
    with pytest.raises(RuntimeError, match="load"):
        st3 = eigen_stream.TripletStream(tn(U.model("small", "l1_j2_f1")), objs)
        st3.gather()
