"""Host-side checks (no GPU) of the SAGPool / EigenGCN post-training phase: the arena and the capacity plan at ``batch=1``, the anchor
schedule and label refusals, every refusal the new entry points of csrc/posttrain_cls.hip and csrc/sag_stream.hip decide on the host
before a launch, tests/posttrain_cls_ref.py against float64 autograd, and the declarations in include/tsgnn.h and the built library."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import posttrain_cls_ref as CR
import sag_stream_util as U

EINVAL, EUNSUPPORTED = -1, -3
P = 1 << 20                                    # (pointers are only tested for NULL and alignment here)


# ------------------------------------------------------------------------------------------------ arenas and plans at batch = 1
@pytest.mark.parametrize("name", ["small6", "dd3"])
def test_sag_arena_at_batch_1_differs_in_its_capacities_only(name):
    from two_stage_gnn_amd import sag_stream as S
    datas = U.datas(U.dataset(name)[3], "cpu")
    a3, a1 = S.pack_arena(datas), S.pack_arena(datas, batch=1)
    assert a3.batch == 3 and a1.batch == 1
    assert a1.caps == (a1.largest, int(a1.records[:, 1].max())) and a3.caps == (3 * a1.caps[0], 3 * a1.caps[1])
    assert a1.largest == max(U.SIZES[name])
    for k in ("records", "buf", "feats"):
        assert np.array_equal(getattr(a1, k), getattr(a3, k)), k
    assert (a1.off, a1.words, a1.fin, a1.ld, a1.n_graphs, a1.total_nodes) == (a3.off, a3.words, a3.fin, a3.ld, a3.n_graphs, a3.total_nodes)
    with pytest.raises(ValueError, match="offsets reach"):
        S.pack_arena(datas, batch=1, limit=8)


@pytest.mark.parametrize("data,name", [("small", "l1_j2_f1"), ("small", "l2_j1"), ("big", "big")])
def test_eigen_arena_at_batch_1_differs_in_its_capacities_only(data, name):
    import eigen_stream_util as EU_
    from two_stage_gnn_amd import eigen_stream as ES
    pool_sizes, J, Jf = EU_.shape(data, name)
    objs = EU_.dataset(data, name)
    a3, a1 = ES.pack_arena(objs, len(pool_sizes), J, Jf), ES.pack_arena(objs, len(pool_sizes), J, Jf, batch=1)
    assert a3.batch == 3 and a1.batch == 1 and a1.top == a3.top
    assert a1.caps == a1.top and a3.caps == (tuple(3 * t for t in a1.top[0]), tuple(3 * t for t in a1.top[1]))
    assert np.array_equal(a1.records, a3.records) and np.array_equal(a1.buf, a3.buf)
    assert (a1.words, a1.nmax, a1.fin, a1.ldf, a1.L, a1.J, a1.Jf, a1.n_graphs) == (a3.words, a3.nmax, a3.fin, a3.ldf, a3.L, a3.J, a3.Jf, a3.n_graphs)
    stub = type("S", (), {"arena": a1})()
    assert ES.PostTrainStream._checked(stub, [a1.n_graphs - 1, 0]).tolist() == [[a1.n_graphs - 1], [0]]
    with pytest.raises(ValueError, match="indices"):
        ES.PostTrainStream._checked(stub, [a1.n_graphs])


def test_eigen_anchor_gather_refuses_on_the_host():
    """the anchor form returns the triplet form's statuses without a launch; its header has B = 1 and its capacities cover ONCE the
    arena's largest piece per level"""
    from two_stage_gnn_amd import _native as nat
    L = nat.lib()
    hw = int(L.tsgnn_eigen_assemble_header_words())

    def desc(B, R0, R1, E0=40, E1=4, nmax=19, ldf=8, J=2, Jf=1):
        d = np.zeros(hw, dtype=np.int64)
        d[0:8] = (B, B, 2, J, Jf, ldf, nmax, 1)
        d[9], d[10] = P, P
        d[12:16] = (R0, E0, R1, E1)
        for i in range(2):
            d[20 + 7 * i:27 + 7 * i] = P
        d[48:52] = P
        return d
    top_n, top_z = np.array([19, 3], dtype=np.int64), np.array([40, 4], dtype=np.int64)

    def call(fn, d, records=P, n_graphs=12, arena=P, words=4096, sched=P, cap=5, state=P, ticket=P, ids=P):
        return fn(records, n_graphs, arena, words, top_n.ctypes.data, top_z.ctypes.data, sched, cap, state, ticket, d.ctypes.data, ids, None)
    anchor, triplet = L.tsgnn_eigen_anchor_gather_f32, L.tsgnn_eigen_triplet_gather_f32
    for fn, B in ((anchor, 1), (triplet, 3)):
        good = desc(B, B * 19, B * 3, B * 40, B * 4)
        for kw in (dict(records=None), dict(ids=None), dict(state=None), dict(ticket=None), dict(n_graphs=0), dict(cap=0), dict(words=0)):
            assert call(fn, good, **kw) == EINVAL, (B, kw)
        assert call(fn, desc(B, B * 19 - 1, B * 3, B * 40, B * 4)) == EINVAL              # a row capacity below B x the largest piece
        assert call(fn, desc(B, B * 19, B * 3, B * 40 - 1, B * 4)) == EINVAL              # ... an entry capacity
        assert call(fn, desc(4 - B, B * 19, B * 3, B * 40, B * 4)) == EINVAL              # the other form's header
        for kw in (dict(records=P + 4), dict(arena=P + 8), dict(state=P + 4), dict(words=1 << 31)):
            assert call(fn, good, **kw) == EUNSUPPORTED, (B, kw)
    assert call(triplet, desc(3, 57, 9, 120, 12), cap=(1 << 31) // 3 + 1) == EUNSUPPORTED
    assert call(anchor, desc(1, 19, 3, 40, 4), cap=1 << 31) == EUNSUPPORTED


def test_capacity_plan_at_batch_1():
    from two_stage_gnn_amd import sag_stream as S
    for largest, ratio in ((31, 0.5), (420, 0.5), (31, 0.3), (1, 0.5)):
        chain = S.k_chain(largest, ratio, 3)
        p1, p3 = S.CapacityPlan(largest, ratio, 3, batch=1), S.CapacityPlan(largest, ratio, 3)
        assert p1.capacity and p1.depth == 3 and p1.batch == 1 and p3.batch == 3 and p1.gp_all is None
        assert [(L.B, L.N, L.max_seg) for L in p1.levels] == [(1, k, k) for k in chain]
        assert [(L.B, L.N, L.max_seg) for L in p3.levels] == [(3, 3 * k, k) for k in chain]


# ------------------------------------------------------------------------------------------------ schedules and labels
def test_anchor_schedules_and_sag_labels():
    from two_stage_gnn_amd import post_train as PT, sag_stream as S
    assert PT.check_anchors([2, 0, 2], 3).tolist() == [[2], [0], [2]] and PT.check_anchors(np.array([[1], [1]]), 3).shape == (2, 1)
    for bad in ([], [[0, 1]], [0.5], [3], [-1]):
        with pytest.raises(ValueError):
            PT.check_anchors(np.asarray(bad), 3)
    # both streams validate through it (an unbound call: no GPU object is needed for the check itself)
    stub = type("S", (), {"arena": type("A", (), {"n_graphs": 3})()})()
    assert S.PostTrainStream._checked(stub, [2, 1]).tolist() == [[2], [1]]
    with pytest.raises(ValueError, match="indices"):
        S.PostTrainStream._checked(stub, [3])

    class D:
        def __init__(self, y):
            if y is not None:
                self.y = y
    ok = [D(torch.tensor([1])), D(np.int64(0)), D(7)]
    assert S.label_table(ok, 8).tolist() == [1, 0, 7] and S.label_table(ok, 8).dtype == np.int32
    assert S.label_table(ok, 8, labels=[7, 7, 0]).tolist() == [7, 7, 0]
    assert S.label_table(ok, 8, labels=torch.tensor([2, 3, 4])).tolist() == [2, 3, 4]
    with pytest.raises(ValueError, match="graph 1 carries no label"):
        S.label_table([D(0), D(None)], 8)
    with pytest.raises(ValueError, match="graph 2: the label must be one integer"):
        S.label_table([D(0), D(1), D(torch.tensor([0.5]))], 8)
    with pytest.raises(ValueError, match="graph 0: the label must be one integer"):
        S.label_table([D(torch.tensor([1, 2]))], 8)
    with pytest.raises(ValueError, match="graph 2: label 8 lies outside \\[0, 8\\)"):
        S.label_table([D(0), D(1), D(8)], 8)
    with pytest.raises(ValueError, match="graph 0: label -1 lies outside"):
        S.label_table([D(-1)], 8)
    with pytest.raises(ValueError, match="2 labels for 3 graphs"):
        S.label_table(ok, 8, labels=[0, 1])


# ------------------------------------------------------------------------------------------------ the entry points' refusals
def test_supported_functions_at_the_envelope_s_edges():
    from two_stage_gnn_amd import _native as nat
    L = nat.lib()
    ok3 = L.tsgnn_posttrain_mlp3_nll_supported
    assert ok3(4, 4, 4, 2, 1) == 1 and ok3(256, 128, 64, 64, 1) == 1 and ok3(2048, 1024, 512, 512, 8) == 1 and ok3(260, 132, 68, 65, 3) == 1
    for bad in ((2052, 128, 64, 64, 1), (256, 1028, 64, 64, 1), (256, 128, 516, 64, 1), (256, 128, 64, 513, 1), (256, 128, 64, 1, 1),
                (254, 128, 64, 64, 1), (256, 126, 64, 64, 1), (256, 128, 62, 64, 1), (256, 128, 64, 64, 0), (256, 128, 64, 64, 9),
                (0, 128, 64, 64, 1)):
        assert ok3(*bad) == 0, bad
    ok2 = L.tsgnn_posttrain_mlp2_ce_supported
    assert ok2(4, 1, 2, 1) == 1 and ok2(1152, 50, 64, 1) == 1 and ok2(2048, 512, 512, 8) == 1 and ok2(36, 7, 3, 3) == 1
    for bad in ((2052, 50, 64, 1), (1150, 50, 64, 1), (1152, 513, 64, 1), (1152, 50, 513, 1), (1152, 50, 1, 1), (1152, 0, 64, 1),
                (1152, 50, 64, 0), (1152, 50, 64, 9)):
        assert ok2(*bad) == 0, bad
    assert L.tsgnn_mlp3_triplet_supported(256, 128, 64, 1) == 1 and L.tsgnn_mlp2_triplet_supported(1152, 50, 1) == 1   # (C >= 2 is the heads')


def test_head_entry_points_refuse_on_the_host():
    """TSGNN_EINVAL / TSGNN_EUNSUPPORTED of the four head launches, decided before anything is launched (there is no GPU here)"""
    from two_stage_gnn_amd import _native as nat
    L = nat.lib()

    def f3(r=P, ld=256, R=1, w1=P, w2=P, w3=P, p=0.0, state=None, used=None, D0=256, D1=128, D2=64, C=64, ids=P, labels=P, n=7,
           a1=P, loss=P):
        return L.tsgnn_posttrain_mlp3_nll_fwd_f32(r, ld, R, w1, P, p, 5, state, used, w2, P, w3, P, D0, D1, D2, C, ids, labels, n, a1, P, P,
                                                  loss, None)

    def b3(r=P, ld=256, R=1, w1=P, D0=256, D1=128, D2=64, C=64, ids=P, labels=P, n=7, a1=P, dr=None, lddr=0, dw1=P, dw3=P):
        return L.tsgnn_posttrain_mlp3_nll_bwd_f32(r, ld, R, w1, P, P, D0, D1, D2, C, 1.0, ids, labels, n, a1, P, P, None, dr, lddr, dw1, None,
                                                  P, None, dw3, None, None)
    for f in (f3, b3):
        for kw in (dict(r=None), dict(R=0), dict(R=9), dict(C=1), dict(ld=252), dict(ids=None), dict(labels=None), dict(n=0), dict(n=1 << 31),
                   dict(a1=None), dict(w1=None), dict(D1=0)):
            assert f(**kw) == EINVAL, (f.__name__, kw)
        for kw in (dict(D0=254, ld=256), dict(D0=2052, ld=2052), dict(D1=1028), dict(D2=516), dict(C=513), dict(D1=126)):
            assert f(**kw) == EUNSUPPORTED, (f.__name__, kw)
    assert f3(p=-0.1) == EINVAL and f3(p=1.0) == EINVAL and f3(p=float("nan")) == EINVAL and f3(loss=None) == EINVAL
    assert f3(p=0.5) == EINVAL and f3(p=0.5, state=P) == EINVAL and f3(p=0.5, used=P) == EINVAL        # the mask's words come together
    assert f3(r=P + 4) == EUNSUPPORTED and f3(ld=258) == EUNSUPPORTED and f3(w1=P + 4) == EUNSUPPORTED and f3(w2=P + 8) == EUNSUPPORTED
    assert f3(w3=P + 4) == EUNSUPPORTED
    assert b3(dw1=None) == EINVAL and b3(dw3=None) == EINVAL and b3(dr=P, lddr=252) == EINVAL

    def f2(r=P, ld=1152, R=1, w1=P, w2=P, D=1152, H=50, C=64, ids=P, labels=P, n=7, h=P, z=P, loss=P):
        return L.tsgnn_posttrain_mlp2_ce_fwd_f32(r, ld, R, w1, None, w2, None, D, H, C, ids, labels, n, h, z, P, loss, None)

    def b2(r=P, ld=1152, R=1, w1=P, w2=P, D=1152, H=50, C=64, ids=P, labels=P, n=7, h=P, dr=None, lddr=0, dw1=P, dw2=P):
        return L.tsgnn_posttrain_mlp2_ce_bwd_f32(r, ld, R, w1, w2, D, H, C, ids, labels, n, h, P, None, dr, lddr, dw1, None, dw2, None, None)
    for f in (f2, b2):
        for kw in (dict(r=None), dict(R=0), dict(R=9), dict(C=1), dict(ld=1148), dict(ids=None), dict(labels=None), dict(n=0), dict(h=None),
                   dict(w1=None), dict(w2=None), dict(H=0)):
            assert f(**kw) == EINVAL, (f.__name__, kw)
        for kw in (dict(D=1150, ld=1152), dict(D=2052, ld=2052), dict(H=513), dict(C=513)):
            assert f(**kw) == EUNSUPPORTED, (f.__name__, kw)
    assert f2(z=None) == EINVAL and f2(loss=None) == EINVAL
    assert f2(r=P + 4) == EUNSUPPORTED and f2(ld=1154) == EUNSUPPORTED and f2(w1=P + 4) == EUNSUPPORTED
    assert b2(dw1=None) == EINVAL and b2(dw2=None) == EINVAL and b2(dr=P, lddr=1148) == EINVAL


def test_sag_anchor_gather_refuses_on_the_host():
    """the anchor form returns the triplet form's statuses without a launch; its capacities are ONE largest graph's"""
    from two_stage_gnn_amd import _native as nat
    L = nat.lib()

    def call(fn, records=P, n_graphs=6, arena=P, off_rowptr=0, off_col=64, words=128, feats=P, ldf=8, need_rows=31, need_nnz=90, sched=P,
             sched_cap=5, state=P, ticket=P, row_cap=31, nnz_cap=90, ratio=0.5, depth=3, rowptr=P, col=P, x=P, ldx=8, dinv=P, self_w=P,
             gp=P, ids=P):
        return fn(records, n_graphs, arena, off_rowptr, off_col, words, feats, ldf, need_rows, need_nnz, sched, sched_cap, state, ticket,
                  row_cap, nnz_cap, ratio, depth, rowptr, col, x, ldx, dinv, self_w, gp, ids, None)
    for fn in (L.tsgnn_sag_anchor_gather_f32, L.tsgnn_sag_triplet_gather_f32):
        for kw in (dict(records=None), dict(ids=None), dict(state=None), dict(row_cap=30), dict(nnz_cap=89), dict(depth=0), dict(depth=8),
                   dict(ratio=0.0), dict(ratio=1.5), dict(off_col=-4), dict(words=32), dict(sched_cap=0), dict(n_graphs=0)):
            assert call(fn, **kw) == EINVAL, kw
        for kw in (dict(ldf=6, ldx=6), dict(ldx=12), dict(off_col=66), dict(x=P + 4), dict(state=P + 8), dict(row_cap=1 << 31, need_rows=0)):
            assert call(fn, **kw) == EUNSUPPORTED, kw
    # what differs: a schedule of [T, 1] may be three times as long before its words pass 2^31
    assert call(L.tsgnn_sag_triplet_gather_f32, sched_cap=(1 << 31) // 3 + 1) == EUNSUPPORTED
    assert call(L.tsgnn_sag_anchor_gather_f32, sched_cap=1 << 31) == EUNSUPPORTED


# ------------------------------------------------------------------------------------------------ the references against autograd
def _rand(gen, *s):
    return torch.randn(*s, generator=gen, dtype=torch.float64)


@pytest.mark.parametrize("shape", [(1, 4, 4, 4, 2), (3, 20, 12, 8, 5), (8, 36, 16, 12, 9)])
@pytest.mark.parametrize("masked", [False, True])
def test_mlp3_nll_ref_is_float64_autograd(shape, masked):
    R, D0, D1, D2, C = shape
    gen = torch.Generator().manual_seed(R + D0)
    p = {"w1": _rand(gen, D1, D0), "b1": _rand(gen, D1), "w2": _rand(gen, D2, D1), "b2": _rand(gen, D2), "w3": _rand(gen, C, D2),
         "b3": _rand(gen, C)}
    r = _rand(gen, R, D0)
    y = torch.randint(0, C, (R,), generator=gen)
    mask = (torch.rand(R, D1, generator=gen) < 0.5).double() if masked else None
    scale = 2.0 if masked else 1.0
    got = CR.mlp3_nll(p, r, y, 0.5, torch.float64, mask=mask, keep_scale=scale)
    q = {k: v.clone().requires_grad_(True) for k, v in p.items()}
    rr = r.clone().requires_grad_(True)
    a1 = F.relu(F.linear(rr, q["w1"], q["b1"])) * (mask * scale if masked else 1.0)
    a2 = F.relu(F.linear(a1, q["w2"], q["b2"]))
    logp = F.log_softmax(F.linear(a2, q["w3"], q["b3"]), dim=-1)
    loss = F.nll_loss(logp, y)
    loss.backward(gradient=torch.tensor(0.5, dtype=torch.float64))
    want = {"a1": a1, "a2": a2, "logp": logp, "loss": loss.reshape(1), "dr": rr.grad, "dw1": q["w1"].grad, "db1": q["b1"].grad,
            "dw2": q["w2"].grad, "db2": q["b2"].grad, "dw3": q["w3"].grad, "db3": q["b3"].grad}
    assert set(got) == set(want)
    for k, v in want.items():
        torch.testing.assert_close(got[k], v.detach(), rtol=1e-12, atol=1e-13, msg=lambda s, k=k: k + ": " + s)
    f32 = CR.mlp3_nll(p, r, y, 0.5, torch.float32, mask=mask, keep_scale=scale)
    assert all(v.dtype == torch.float32 for v in f32.values())


@pytest.mark.parametrize("shape", [(1, 4, 1, 2), (3, 36, 7, 3), (8, 24, 50, 11)])
@pytest.mark.parametrize("bias", [True, False])
def test_mlp2_ce_ref_is_float64_autograd(shape, bias):
    R, D, H, C = shape
    gen = torch.Generator().manual_seed(R + D + H)
    p = {"w1": _rand(gen, H, D), "b1": _rand(gen, H) if bias else None, "w2": _rand(gen, C, H), "b2": _rand(gen, C) if bias else None}
    r = _rand(gen, R, D)
    y = torch.randint(0, C, (R,), generator=gen)
    got = CR.mlp2_ce(p, r, y, 0.5, torch.float64)
    q = {k: (v.clone().requires_grad_(True) if v is not None else None) for k, v in p.items()}
    rr = r.clone().requires_grad_(True)
    h = F.relu(F.linear(rr, q["w1"], q["b1"]))
    z = F.linear(h, q["w2"], q["b2"])
    loss = F.cross_entropy(z, y)
    loss.backward(gradient=torch.tensor(0.5, dtype=torch.float64))
    want = {"h": h, "z": z, "p": F.softmax(z, dim=1), "loss": loss.reshape(1), "dr": rr.grad, "dw1": q["w1"].grad, "dw2": q["w2"].grad}
    if bias:
        want.update({"db1": q["b1"].grad, "db2": q["b2"].grad})
    for k, v in want.items():
        torch.testing.assert_close(got[k], v.detach(), rtol=1e-12, atol=1e-13, msg=lambda s, k=k: k + ": " + s)


# ------------------------------------------------------------------------------------------------ declarations
def test_new_entry_points_are_declared_and_exported():
    from two_stage_gnn_amd import _native as nat
    decls = nat.parse_header()
    names = ["tsgnn_sag_anchor_gather_f32", "tsgnn_eigen_anchor_gather_f32", "tsgnn_posttrain_mlp3_nll_supported", "tsgnn_posttrain_mlp3_nll_fwd_f32",
             "tsgnn_posttrain_mlp3_nll_bwd_f32", "tsgnn_posttrain_mlp2_ce_supported", "tsgnn_posttrain_mlp2_ce_fwd_f32",
             "tsgnn_posttrain_mlp2_ce_bwd_f32"]
    nat.build()
    lib = ctypes.CDLL(nat.LIB_PATH)
    for n in names:
        assert n in decls and hasattr(lib, n), n
    for fam in ("sag", "eigen"):
        a, t = decls["tsgnn_%s_anchor_gather_f32" % fam][1], decls["tsgnn_%s_triplet_gather_f32" % fam][1]
        assert [ty for ty, _ in a] == [ty for ty, _ in t] and [n for _, n in a] == [n for _, n in t]
    assert len(decls["tsgnn_posttrain_mlp3_nll_fwd_f32"][1]) == 25 and len(decls["tsgnn_posttrain_mlp2_ce_bwd_f32"][1]) == 21


# ------------------------------------------------------------------------------------------------ the EigenGCN fixture's own consistency
FIXTURE = "posttrain_eigen"


def fixture_steps(g):
    """[(prefix of the step's keys)]: the triplet step, then the post-training steps, in the order the reference's first Adam saw them"""
    return ["triplet."] + ["s%d." % s for s in range(int(g["n_steps"]))]


def replay_adam(g, dtype=np.float64):
    """the reference's first optimiser restated in numpy from the fixture's own pre-clip gradients: ``clip_grad_norm`` over all
    parameters (coefficient clip / (norm + 1e-6) where below 1), then torch's Adam with L2 weight decay added to the clipped
    gradient, betas (0.9, 0.999), eps 1e-8, moments and step count continued across the triplet step and the post-training steps
    -> [{parameter: value after the step}] per step of ``fixture_steps``"""
    lr, wd, clip = float(g["lr"]), float(g["weight_decay"]), float(g["clip"])
    names = [k[2:] for k in g if k.startswith("p.")]
    p = {k: g["p." + k].astype(dtype) for k in names}
    m = {k: np.zeros_like(p[k]) for k in names}
    v = {k: np.zeros_like(p[k]) for k in names}
    out = []
    for t, pre in enumerate(fixture_steps(g), start=1):
        gr = {k: g[pre + "g." + k].astype(dtype) for k in names}
        norm = np.sqrt(sum(float((x.astype(np.float64) ** 2).sum()) for x in gr.values()))
        coef = clip / (norm + 1e-6)
        for k in names:
            x = gr[k] * dtype(coef) if coef < 1.0 else gr[k]
            x = x + dtype(wd) * p[k]
            m[k] = dtype(0.9) * m[k] + dtype(0.1) * x
            v[k] = dtype(0.999) * v[k] + dtype(0.001) * x * x
            step = lr / (1.0 - 0.9 ** t)
            p[k] = p[k] - dtype(step) * m[k] / (np.sqrt(v[k]) / dtype(np.sqrt(1.0 - 0.999 ** t)) + dtype(1e-8))
        out.append({k: p[k].copy() for k in names})
    return out


def test_eigen_fixture_is_consistent_with_its_own_gradients():
    """the reference's parameters after every step reproduce from its own pre-clip gradients by the numpy clip + Adam (weight decay,
    continued moments); every loss is positive, every conv and pred_model weight has a non-zero gradient in every step, the clip is
    active in at least one post-training step and inactive in at least one; the file holds arrays only and is no larger than
    tests/golden/posttrain_diffpool.npz"""
    import os
    from conftest import GOLDEN, load_golden
    g = load_golden(FIXTURE)
    steps = fixture_steps(g)
    assert len(steps) == 4 and float(g["weight_decay"]) > 0
    after = replay_adam(g)
    for pre, ps in zip(steps, after):
        assert float(g[pre + "loss"]) > 0
        for k, want in ps.items():
            got = g[pre + "p." + k]
            assert got.dtype == np.float32
            np.testing.assert_allclose(got, want, rtol=2e-6, atol=5e-7, err_msg=pre + k)
            if k.endswith("weight"):
                assert np.any(g[pre + "g." + k] != 0), pre + k
    norms = [float(g["s%d.norm" % s]) for s in range(3)]
    assert min(norms) < float(g["clip"]) < max(norms)
    moved = max(float(np.abs(after[-1][k] - g["p." + k]).max()) for k in after[-1])
    assert moved > 2 * float(g["lr"])                                                  # (four steps of Adam: the test above is not vacuous)
    assert len({int(g["t%d.num_nodes" % t]) for t in range(3)}) == 3 and sorted(int(g["t%d.label" % t]) for t in range(3)) == [0, 2, 5]
    assert all(v.dtype.kind in "fiu" for v in g.values())
    size = lambda n: os.path.getsize(os.path.join(GOLDEN, n + ".npz"))
    assert size(FIXTURE) <= size("posttrain_diffpool") and size(FIXTURE) < (1 << 20)
