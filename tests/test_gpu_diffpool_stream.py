"""The DiffPool triplet stream on the GPU (two_stage_gnn_amd/diffpool_stream.py, diffpool._ContractCap, csrc/contract_cap.hip): one
streamed step per schedule entry against the eager drop-in and the CPU oracle's three B = 1 forwards, the launch trace of a step,
no host in the loop, an epoch walked by replays of one hipGraph, and the constructor's refusals.

Dataset and schedule: tests/triplet_stream_util.py.  The hinge is active in every entry: margin 10, ``map_model`` scaled down."""
import copy

import numpy as np
import pytest
import torch

import triplet_stream_util as U
from oracle import dense_ref as R

pytestmark = pytest.mark.gpu

MARGIN, HID = 10.0, 32


class _A:
    bias = True


def _model(nmax, num_pooling=1, seed=6, hid=HID):
    from two_stage_gnn_amd import dense_encoders as E
    torch.manual_seed(seed)
    m = E.SoftPoolingGcnEncoder(nmax, U.FIN, hid, hid, 2, 3, hid, assign_ratio=0.25, num_pooling=num_pooling, bn=True, linkpred=False,
                                args=_A(), assign_input_dim=U.FIN, final_dim="output_dim")
    with torch.no_grad():
        for k, p in m.named_parameters():
            if "conv" in k and k.endswith("bias"):
                p.copy_(torch.randn_like(p) * 0.3)
        m.map_model.weight.mul_(0.25)                        # distances of a few units: the margin-10 hinge is active for every entry
    return m.cuda()


def _stream(m, graphs, **kw):
    from two_stage_gnn_amd import diffpool_stream, triplet
    net = triplet.tripletnet(m)
    return net, diffpool_stream.TripletStream(net, graphs, **kw)


def _oracle_step(p_ref, graphs, ids, num_pooling):
    """the reference's step: three B = 1 forwards, distances, margin loss; -> (dp, dn, embeds, grads)"""
    for v in p_ref.values():
        v.grad = None
    emb = []
    for i in ids:
        d = graphs[i].graph
        x, adj = torch.from_numpy(d["feats"])[None], torch.from_numpy(d["adj"])[None]
        emb.append(R.diffpool_encoder(p_ref, x, adj, np.array([d["num_nodes"]]), num_pooling, assign_x=x, final_dim="output_dim")[1])
    dp = torch.nn.functional.pairwise_distance(emb[0], emb[1], 2)
    dn = torch.nn.functional.pairwise_distance(emb[0], emb[2], 2)
    torch.nn.MarginRankingLoss(margin=MARGIN)(dp, dn, torch.tensor([-1.0])).backward()
    return dp.detach(), dn.detach(), [e.detach() for e in emb], {k: v.grad for k, v in p_ref.items() if v.grad is not None}


@pytest.mark.parametrize("nmax,num_pooling", [(48, 1), (64, 2), (400, 1)])
def test_streamed_step_equals_the_drop_in_and_the_oracle(nmax, num_pooling):
    """nmax 48: K = 12; nmax 64: two pooling levels, K = 16 and 4; nmax 400: K = 100.  Every schedule entry, from equal parameters:
    the streamed step against ``net(a, p, n)`` and against the oracle's three B = 1 ``diffpool_encoder`` forwards at the bounds of
    test_triplet_step_equals_three_b1_forwards (outputs 1e-4, gradients 5e-3 max|ref| + 1e-6); the drop-in itself is held to the
    same bounds against the oracle, and the largest streamed - drop-in gradient difference is printed.  Gradients are compared from
    equal parameters, never after Adam.  For [1, 1, 1] (anchor = positive = negative: d_p - d_n is identically zero) the gradient is
    pure rounding: that one entry's gradient comparison is skipped, and it is the only one.
    Measured on an MI355X (profiles/r15/diffpool_stream.txt keeps the lines this test prints): the largest |streamed - drop-in| gradient
    entry is 7.5e-9 to 6.0e-8 per entry at max|grad| 1.5 to 2.4 (both routes run the same stacks; the contraction's two backward forms differ
    in summation order only), the largest |streamed - oracle| 5.4e-7 to 2.0e-6; for [1, 1, 1] both routes give a gradient of exactly 0."""
    from two_stage_gnn_amd.triplet import MarginRankingLoss
    graphs = U.dataset(nmax=nmax)
    m = _model(nmax, num_pooling)
    net, st = _stream(m, graphs)
    assert st.g.ghost_slots_fixed == min(nmax, 49) and int(m.assign_pred_modules[0].out_features) == nmax // 4
    st.load(U.SCHEDULE)
    crit, tgt = MarginRankingLoss(margin=MARGIN), torch.tensor([-1.0]).cuda()
    p_ref = {k: v.detach().cpu().clone().requires_grad_(True) for k, v in m.state_dict().items()}

    def grads_of():
        return {k: p.grad.detach().clone() for k, p in m.named_parameters() if p.grad is not None}

    skipped = []
    for k, ids in enumerate(U.SCHEDULE):
        m.zero_grad(set_to_none=True)
        outs = st.embed()
        crit(outs[0], outs[1], tgt).backward()
        gs = grads_of()
        assert st.ids_out.tolist() == ids.tolist()
        m.zero_grad(set_to_none=True)
        outd = net(*[graphs[i] for i in ids])
        crit(outd[0], outd[1], tgt).backward()
        gd = grads_of()
        dpo, dno, embo, go = _oracle_step(p_ref, graphs, ids, num_pooling)
        assert float(dpo - dno) + MARGIN > 0                       # the hinge is active
        for name, got in (("streamed", outs), ("drop-in", outd)):
            torch.testing.assert_close(got[0].detach().cpu(), dpo, rtol=1e-4, atol=1e-4, msg=lambda s_, n_=name: "%s d_p: %s" % (n_, s_))
            torch.testing.assert_close(got[1].detach().cpu(), dno, rtol=1e-4, atol=1e-4, msg=lambda s_, n_=name: "%s d_n: %s" % (n_, s_))
            for a, b in zip(got[2:], embo):
                torch.testing.assert_close(a.detach().cpu(), b, rtol=1e-4, atol=1e-4, msg=lambda s_, n_=name: "%s embedding: %s" % (n_, s_))
        assert set(go) == set(gs) == set(gd) and len(go) >= 12
        scale = max(float(v.abs().max()) for v in go.values())
        worst = max(float((gs[n_] - gd[n_]).abs().max()) for n_ in gd)
        worst_o = max(float((gs[n_].cpu() - go[n_]).abs().max()) for n_ in go)
        print("nmax %d entry %d %s: max|grad| %.3e, max|streamed - drop-in| %.3e, max|streamed - oracle| %.3e"
              % (nmax, k, ids.tolist(), scale, worst, worst_o))
        if len(set(ids.tolist())) == 1:
            skipped.append(ids.tolist())
            continue
        for n_, ref in go.items():
            bound = 5e-3 * float(ref.abs().max()) + 1e-6
            for name, got in (("streamed", gs), ("drop-in", gd)):
                err = float((got[n_].cpu() - ref).abs().max())
                assert err <= bound, (name, k, n_, err, float(ref.abs().max()))
    assert skipped == [[1, 1, 1]]


def test_launch_trace_of_a_streamed_step():
    """one gather launch, the row sum and the capacity backward once each, no csr_spmm, no ragged gemm"""
    from two_stage_gnn_amd import _native as nat
    from two_stage_gnn_amd.triplet import MarginRankingLoss
    graphs = U.dataset()
    m = _model(U.NMAX)
    net, st = _stream(m, graphs)
    st.load(U.SCHEDULE)
    crit, tgt = MarginRankingLoss(margin=MARGIN), torch.tensor([-1.0]).cuda()
    st.loss(crit, tgt)().backward()                              # (warm: allocator, library load)
    m.zero_grad(set_to_none=True)
    nat.trace = []
    try:
        st.loss(crit, tgt)().backward()
        trace = list(nat.trace)
    finally:
        nat.trace = None
    names = [t[0] for t in trace]
    print("library launches of a streamed DiffPool step: %d\n%s" % (len(names), " ".join(names)))
    assert names.count("triplet_gather_f32") == 1 and names[0] == "triplet_gather_f32"
    assert names.count("ell_rowsum_f32") == 1 and names.count("contract_cap_bwd_f32") == 1 and names.count("ragged_tn_direct_ro_f32") == 1
    assert not [n for n in names if n.startswith("csr_spmm") or n in ("ragged_tn_f32", "contract_rows_bwd_f32", "contract_rows_bwd_ro_f32")]
    assert not [t for t in trace if t[0] == "gemm_f32" and int(t[1][17]) != 0]                   # (..., seg_ptr, ragged, ...)
    assert names.count("dense_pg_layer_fwd_f32") == 3 and names.count("dense_pg_layer_bwd_f32") == 3
    assert "row_maps" not in names


def test_no_host_in_the_loop():
    """after one warm call, forward + backward of a streamed step under sync debug mode "error" """
    from two_stage_gnn_amd.triplet import MarginRankingLoss
    graphs = U.dataset()
    m = _model(U.NMAX)
    net, st = _stream(m, graphs)
    st.load(U.SCHEDULE)
    crit, tgt = MarginRankingLoss(margin=MARGIN), torch.tensor([-1.0]).cuda()
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


def test_replays_walk_the_schedule_and_move_the_parameters_as_uncaptured_steps():
    """``GraphedStep(FlatTrainer(...), st.loss(...))``: five replays walk the schedule (``ids_out`` per replay, ``position() == 5``)
    and move the parameters as five uncaptured streamed steps of a deep-copied model do — the same route, so rtol 1e-5 / atol 1e-6"""
    from two_stage_gnn_amd import message_passing as mp
    from two_stage_gnn_amd.data_parallel import FlatTrainer, GraphedStep
    from two_stage_gnn_amd.triplet import MarginRankingLoss
    graphs = U.dataset()
    m1 = _model(U.NMAX)
    m2 = copy.deepcopy(m1)
    start = {k: v.detach().clone() for k, v in m1.state_dict().items()}
    T, lr = len(U.SCHEDULE), 1e-3
    crit, tgt = MarginRankingLoss(margin=MARGIN), torch.tensor([-1.0]).cuda()
    net2, st2 = _stream(m2, graphs)
    st2.load(U.SCHEDULE)
    tr2 = FlatTrainer(m2, lr=lr, clip=2.0)
    step2 = st2.loss(crit, tgt)
    for ids in U.SCHEDULE:
        tr2.step(step2)
        assert st2.ids_out.tolist() == ids.tolist()
    net1, st1 = _stream(m1, graphs)
    st1.load(U.SCHEDULE)
    gs = GraphedStep(FlatTrainer(m1, lr=lr, clip=2.0), st1.loss(crit, tgt))     # (its warm-up steps consume entries and are rolled back ...)
    st1.load(U.SCHEDULE)                                                        # ... so the epoch starts here: cursor := 0
    for ids in U.SCHEDULE:
        gs.step()
        gs.synchronize()
        assert st1.ids_out.tolist() == ids.tolist()
    assert st1.position() == T == 5 and np.isfinite(gs.loss_value())
    mp.check_device_errors()
    moved = 0
    for (k, p1), (_, p2) in zip(m1.named_parameters(), m2.named_parameters()):
        torch.testing.assert_close(p1.detach(), p2.detach(), rtol=1e-5, atol=1e-6, msg=lambda s_, k=k: k + ": " + s_)
        moved += int(not torch.equal(p1.detach(), start[k]))
    assert moved >= 12


def test_constructor_and_load_refuse():
    from two_stage_gnn_amd import dense_encoders as E
    from two_stage_gnn_amd import diffpool_stream, triplet
    graphs = U.dataset()
    m = _model(U.NMAX)
    m.bn = False                                                   # (the constructor does not forward bn: encoders.py:249-250)
    with pytest.raises(TypeError, match="eager drop-in"):
        diffpool_stream.TripletStream(triplet.tripletnet(m), graphs)
    with pytest.raises(TypeError, match="eager drop-in"):          # stacks wider than the fused per-graph node takes
        diffpool_stream.TripletStream(triplet.tripletnet(_model(U.NMAX, hid=136)), graphs)
    sage = E.GcnEncoderGraph(U.FIN, HID, HID, 2, 3, bn=True, args=_A(), final_dim="output_dim").cuda()
    with pytest.raises(TypeError, match="eager drop-in"):
        diffpool_stream.TripletStream(triplet.tripletnet(sage), graphs)
    with pytest.raises(TypeError, match="eager drop-in"):          # ... and the GraphSage stream keeps refusing the DiffPool encoder
        triplet.TripletStream(triplet.tripletnet(_model(U.NMAX)), graphs)
    net, st = _stream(_model(U.NMAX), graphs, max_steps=4)
    assert len(st) == 1 and st.position() == 0
    with pytest.raises(ValueError, match="exceeds"):
        st.load(U.SCHEDULE)                                        # five entries into a buffer of four
    assert st.load(U.SCHEDULE[:4]) == 4
