"""The MLP probe on the GPU: ``two_stage.MLPProbe`` (csrc/mlp_probe.hip: the whole training pass as one launch of one workgroup, the
predictions as a second launch) against the reference's loop in float64 on the CPU (tests/mlp_probe_oracle.py, where the tolerance and
the undecided rule are stated), and ``two_stage.evaluate_mlp`` end to end."""
import numpy as np
import pytest
import torch

import mlp_probe_oracle as MO

pytestmark = pytest.mark.gpu

# (seed, n, q, D, C), hidden
GRID = [((7, 16, 8, 4, 2), (64, 32)),
        ((6, 64, 16, 6, 2), (64, 32)),           # rows of 8 floats, NaN in the padding
        ((4, 37, 5, 8, 3), (64, 32)),
        ((10, 1, 4, 12, 2), (64, 32)),           # a single step
        ((1, 1051, 117, 20, 2), (64, 32)),
        ((0, 1051, 117, 64, 2), (64, 32)),
        ((5, 256, 64, 384, 2), (64, 32)),
        ((8, 256, 64, 512, 2), (64, 32)),        # the widest first layer whose moments stay in registers
        ((9, 128, 32, 1024, 4), (64, 32)),       # past it: the moments stream through the moment buffers
        ((11, 200, 40, 20, 6), (16, 8)),
        ((12, 200, 40, 36, 3), (64, 64))]


def _padded(a, fill):
    """the rows of ``a`` inside a wider buffer whose padding holds ``fill``: a view with a stride of the next multiple of 4 (+ 4)"""
    n, d = a.shape
    buf = torch.full((n, (d + 3) // 4 * 4 + (4 if d % 4 == 0 else 0)), fill, device="cuda")
    buf[:, :d] = torch.from_numpy(a).cuda()
    return buf[:, :d]


def _got(probe, Q):
    return {"losses": probe.losses_.cpu().numpy(), "logits": probe.decision_function(Q).cpu().numpy(),
            "params": [p.cpu().numpy() for p in probe._params]}


@pytest.mark.parametrize("case,hidden", GRID, ids=lambda c: "_".join(str(v) for v in c))
def test_fit_and_predict_against_the_fp64_loop(case, hidden):
    from two_stage_gnn_amd import _native as nat, two_stage as TS
    ref = MO.case(*case, hidden=hidden)
    n, C = case[1], case[4]
    nan_pad = case[3] % 4 != 0
    X = _padded(ref["X"], float("nan")) if nan_pad else torch.from_numpy(ref["X"]).cuda()
    Q = _padded(ref["Q"], float("nan")) if nan_pad else torch.from_numpy(ref["Q"]).cuda()
    keep = [t.clone() for t in ref["init"]]
    probe = TS.MLPProbe(hidden).fit(X, ref["y"], classes=np.arange(C), init=ref["init"])
    assert probe.kernel_ok() and nat.last_kernel().startswith("mlp_probe_fit_kernel")
    assert all(torch.equal(a, b) for a, b in zip(keep, ref["init"]))
    got = _got(probe, Q)
    assert nat.last_kernel().startswith("mlp_probe_predict_kernel")
    tag = "%s %s" % (case, hidden)
    MO.check_run(tag, got, ref)
    pred = probe.predict(Q)
    assert pred.is_cuda and pred.dtype == torch.int64
    MO.check_predictions(tag, pred.cpu().numpy(), ref["f64"]["logits"])
    assert (pred.cpu().numpy() == got["logits"].argmax(1)).all()
    # the same pass again: the same bits
    again = TS.MLPProbe(hidden).fit(X, ref["y"], classes=np.arange(C), init=ref["init"])
    assert torch.equal(again.losses_, probe.losses_) and torch.equal(again._flat, probe._flat)
    assert torch.equal(again._exp_avg, probe._exp_avg) and torch.equal(again._exp_avg_sq, probe._exp_avg_sq)
    assert probe._step == n


@pytest.mark.parametrize("h", [1, 37 // 2])
def test_split_fit_continues_moments_and_step_count(h):
    from two_stage_gnn_amd import two_stage as TS
    ref = MO.case(4, 37, 5, 8, 3)
    X = torch.from_numpy(ref["X"]).cuda()
    whole = TS.MLPProbe().fit(X, ref["y"], classes=np.arange(3), init=ref["init"])
    split = TS.MLPProbe().fit(X[:h], ref["y"][:h], classes=np.arange(3), init=ref["init"])
    first = split.losses_.clone()
    split.partial_fit(X[h:], ref["y"][h:])
    assert split._step == 37 and torch.equal(split._flat, whole._flat)
    assert torch.equal(split._exp_avg, whole._exp_avg) and torch.equal(split._exp_avg_sq, whole._exp_avg_sq)
    assert torch.equal(torch.cat([first, split.losses_]), whole.losses_)


@pytest.mark.parametrize("case", [(4, 37, 5, 8, 3), (8, 256, 64, 512, 2), (9, 128, 32, 1024, 4)], ids=lambda c: "D%d" % c[3])
def test_zero_columns_leave_their_weights_untouched(case):
    """five input columns exactly zero: gradient 0, Adam update 0, so those columns of W1 keep the bits of ``init``"""
    from two_stage_gnn_amd import two_stage as TS
    ref = MO.case(*case)
    D = case[3]
    cols = [0, 3, D // 2, D - 2, D - 1]
    X = torch.from_numpy(ref["X"]).cuda()
    X[:, cols] = 0.0
    probe = TS.MLPProbe().fit(X, ref["y"], classes=np.arange(case[4]), init=ref["init"])
    W1 = probe._params[0].cpu()
    assert torch.equal(W1[:, cols], ref["init"][0][:, cols])
    other = [c for c in range(D) if c not in cols]
    assert not torch.equal(W1[:, other], ref["init"][0][:, other])


def test_zero_pre_activation_takes_the_negative_slope():
    """an all-zero first row with b1 = 0: every pre-activation of layer 1 is exactly 0, where torch's LeakyReLU has the derivative
    ``negative_slope``.  After that one step W1 has not moved (x = 0) and everything equals the fp64 run.  Adam's first step is
    lr g / (|g| + eps), which hides the size of g, so the gradient that reached b1 is read from its first moment, 0.1 g: with a
    derivative of 1 at zero it would be a hundred times the fp64 value, with 0 it would vanish.  Its bound: the rule's
    10 err(cpu32), or 1e-5 of the largest fp64 entry (the rule's floor, relative to this array's own scale: g is a sum of 32
    products, whose fp32 rounding is a few 2^-24 of it)"""
    from two_stage_gnn_amd import two_stage as TS
    ref = MO.case(4, 37, 5, 8, 3)
    init = [t.clone() for t in ref["init"]]
    init[1].zero_()
    X = np.zeros((1, 8), dtype=np.float32)
    y = ref["y"][:1]
    f64 = MO.run(init, X, y, ref["Q"], torch.float64)
    f32 = MO.run(init, X, y, ref["Q"], torch.float32)
    probe = TS.MLPProbe().fit(torch.from_numpy(X).cuda(), y, classes=np.arange(3), init=init)
    got = _got(probe, torch.from_numpy(ref["Q"]).cuda())
    MO.check_run("zero pre-activation", got, {"f64": f64, "f32": f32})
    assert torch.equal(probe._params[0].cpu(), init[0])
    m_b1 = probe._exp_avg[64 * 8:64 * 8 + 64].cpu().numpy().astype(np.float64)
    want, want32 = f64["exp_avg"][1], f32["exp_avg"][1]
    err, tol = np.abs(m_b1 - want).max(), max(10 * np.abs(want32 - want).max(), 1e-5 * np.abs(want).max())
    print("first moment of b1: max |fp64| %.3g, err %.3g, bound %.3g" % (np.abs(want).max(), err, tol))
    assert np.abs(want).max() > 0 and err <= tol


def test_labels_map_through_classes_and_come_back_in_their_dtype():
    from two_stage_gnn_amd import two_stage as TS
    ref = MO.case(7, 16, 8, 4, 2)
    y = np.where(ref["y"] == 0, 3, 7).astype(np.int32)
    X, Q = torch.from_numpy(ref["X"]).cuda(), torch.from_numpy(ref["Q"]).cuda()
    probe = TS.MLPProbe().fit(X, y, init=ref["init"])
    assert probe.classes_.tolist() == [3, 7] and probe.kernel_ok()
    MO.check("labels {3, 7} losses", probe.losses_.cpu().numpy(), ref["f64"]["losses"], ref["f32"]["losses"])
    pred = probe.predict(Q)
    assert pred.is_cuda and pred.dtype == torch.int32 and set(pred.tolist()) <= {3, 7}
    host = probe.predict(ref["Q"])
    assert isinstance(host, np.ndarray) and host.dtype == np.int32 and (host == pred.cpu().numpy()).all()
    as_tensor = TS.MLPProbe().fit(X, torch.from_numpy(y.astype(np.int64)), init=ref["init"]).predict(Q)
    assert as_tensor.dtype == torch.int64 and (as_tensor.cpu().numpy() == host).all()
    assert isinstance(probe.decision_function(ref["Q"]), np.ndarray)


def test_correct_count_accumulates_and_ties_go_to_the_lower_class():
    from two_stage_gnn_amd import two_stage as TS
    ref = MO.case(1, 1051, 117, 20, 2)
    X, Q = torch.from_numpy(ref["X"]).cuda(), torch.from_numpy(ref["Q"]).cuda()
    probe = TS.MLPProbe().fit(X, ref["y"], init=ref["init"])
    pred = probe.predict(Q).cpu().numpy()
    want = int((pred == ref["yq"]).sum())
    assert probe.score(Q, ref["yq"]) == want / 117
    count = probe.correct_count(Q, ref["yq"])
    assert int(count.cpu()) == want
    probe.correct_count(Q, ref["yq"], count)
    assert int(count.cpu()) == 2 * want                                                   # the count accumulates over calls
    other = np.where(np.arange(117) % 2 == 0, ref["yq"], 9)                               # a label outside classes_ counts as wrong
    assert int(probe.correct_count(Q, other).cpu()) == int((pred == other).sum())
    # an exact tie: a last layer with equal rows 0 and 1 and a smaller row 2; lr = 0 keeps it through the pass
    init = MO.initial(3, 20, (64, 32), 3)
    init[4][1] = init[4][0]
    init[5][1] = init[5][0]
    init[4][2] = init[4][0]
    init[5][2] = init[5][0] - 1.0
    tied = TS.MLPProbe(lr=0.0).fit(X[:4], [0, 1, 2, 1], init=init)
    logits = tied.decision_function(Q)
    assert torch.equal(logits[:, 0], logits[:, 1]) and (logits[:, 2] < logits[:, 0]).all()
    assert (tied.predict(Q) == 0).all()


# ----------------------------------------------------------------------------- evaluate_mlp end to end
def _dense_sets():
    from test_gpu_two_stage import _G, _dense_model
    from util_graphs import dense_batch
    nmax, fin = 20, 6
    x, adj, sizes = dense_batch(11, 17, nmax, fin, p_edge=0.25)
    labels = [0, 1, 1, 0, 1, 0, 0, 1, 1, 0, 1, 0, 1, 0, 0, 1, 5]                        # (the last validation label: not a training label)
    graphs = [_G(adj[b].numpy(), (x[b] + 0.5 * labels[b]).numpy(), int(sizes[b]), label=labels[b]) for b in range(17)]
    return _dense_model("base", "output_dim", nmax, fin), graphs[:12], graphs[12:]


def _net_sets():
    from test_gpu_sag_triplet import NET_SEED, _D, _graph, _net
    fin = 5
    net = _net(fin, 32, 8, "gcn", False, 0.5, seed=NET_SEED)
    datas = []
    for i in range(17):
        x, ei = _graph(7000 + i, 4 + (5 * i) % 16, fin, 2.2)
        d = _D(x + 0.5 * (i % 2), ei)
        d.y = torch.tensor([i % 2])
        datas.append(d)
    return net, datas[:12], datas[12:]


@pytest.mark.parametrize("family", ["dense", "net"])
def test_evaluate_mlp_is_the_probe_on_the_embedded_rows(family):
    from two_stage_gnn_amd import two_stage as TS
    model, train, val = _dense_sets() if family == "dense" else _net_sets()
    model.train()
    had_pg = hasattr(model, "per_graph_bn")
    y_train, y_val = TS._labels(train), TS._labels(val)
    emb = TS.embed_dataset(model, train + val)
    init = MO.initial(2, int(emb.size(1)), (64, 32), 2)
    keep = [t.clone() for t in init]
    res = TS.evaluate_mlp(train, val, model, init=init)
    assert model.training and (not had_pg or model.per_graph_bn is False)
    assert all(torch.equal(a, b) for a, b in zip(keep, init))
    by_hand = TS.MLPProbe().fit(emb[:12], y_train, init=init)
    pred = by_hand.predict(emb[12:]).cpu().numpy()
    assert list(res) == ["acc"] and res["acc"] == float((pred == y_val).sum()) / 5
    # against the fp64 loop on the same rows (embed_dataset has its own tests)
    E, cls = emb.cpu().numpy(), np.searchsorted(by_hand.classes_, y_train)
    ref = {"f64": MO.run(init, E[:12], cls, E[12:], torch.float64), "f32": MO.run(init, E[:12], cls, E[12:], torch.float32)}
    MO.check_run("evaluate_mlp " + family, _got(by_hand, emb[12:]), ref)
    # a probe of the caller's and the default construction under torch's generator
    mine = TS.MLPProbe(hidden=(16, 8))
    torch.manual_seed(5)
    res2 = TS.evaluate_mlp(train, val, model, probe=mine)
    torch.manual_seed(5)
    again = TS.MLPProbe(hidden=(16, 8)).fit(emb[:12], y_train)
    assert torch.equal(mine._flat, again._flat) and res2["acc"] == again.score(emb[12:], y_val)


def test_fit_does_not_wait_for_the_device():
    """fit + the counting predict without a host synchronisation (``set_sync_debug_mode('error')`` raises at any); the one copy of
    ``score`` is the count"""
    from two_stage_gnn_amd import two_stage as TS
    ref = MO.case(0, 1051, 117, 64, 2)
    X, Q = torch.from_numpy(ref["X"]).cuda(), torch.from_numpy(ref["Q"]).cuda()
    TS.MLPProbe().fit(X, ref["y"], init=ref["init"]).correct_count(Q, ref["yq"])         # (first use: library load, allocator warm-up)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        probe = TS.MLPProbe().fit(X, ref["y"], init=ref["init"])
        count = probe.correct_count(Q, ref["yq"])
        with pytest.raises(RuntimeError):
            count.cpu()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert 0 <= int(count.cpu()) <= 117
