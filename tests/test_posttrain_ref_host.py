"""Post-training phase, host side (no GPU): tests/posttrain_ref.py on the CPU oracle reproduces the reference's own six steps
(tests/golden/posttrain_gcn.npz, scripts/gen_golden_posttrain.py) at the tolerances of tests/test_oracle_golden.py for the encoder
fixtures (outputs rtol 1e-4 / atol 1e-5, gradients rtol 1e-3 / atol 1e-4); the label table, the anchor schedules and the
construction order of ``make_head``."""
import numpy as np
import pytest
import torch

import posttrain_ref as PR
import triplet_stream_util as U
from conftest import load_golden, params_of
from oracle import dense_ref as R

OUT_TOL = dict(rtol=1e-4, atol=1e-5)
GRAD_TOL = dict(rtol=1e-3, atol=1e-4)


def test_reference_step_reproduces_the_golden_steps():
    g = load_golden("posttrain_gcn")
    dicts = PR.golden_graphs(g)
    assert [d["num_nodes"] for d in dicts][:2] == [int(g["nmax"]), 1] and {d["label"] for d in dicts} == {0, 1}
    p = params_of(g, requires_grad=True)
    trained = [v for k, v in p.items() if not k.startswith(("pre_pred_model", "pred_model"))]      # (no gradient in this setting: Adam skips them)
    opt = torch.optim.Adam(trained, lr=float(g["lr"]))
    for s, d in enumerate(dicts):
        opt.zero_grad()
        loss, pred, out = PR.step(p, d)
        loss.backward()
        np.testing.assert_allclose(float(loss.detach()), float(g["s%d.loss" % s]), err_msg="loss %d" % s, **OUT_TOL)
        if s == 0:
            # (outputs are compared from EQUAL parameters: behind an Adam step an element whose gradient is rounding noise, 7 of
            # conv_block.0.weight here, moves by up to lr in either implementation, and a later step's `out` carries that)
            np.testing.assert_allclose(pred.detach().numpy(), g["s0.pred"], err_msg="pred", **OUT_TOL)
            np.testing.assert_allclose(out.detach().numpy(), g["s0.out"], err_msg="out", **OUT_TOL)
            # the oracle's own "output_dim" heads on the same parameters: its second output is map_model on the readout, this `out`
            x, adj = torch.as_tensor(d["feats"])[None], torch.as_tensor(d["adj"])[None]
            np.testing.assert_allclose(R.gcn_encoder(p, x, adj, bn=True, final_dim="output_dim")[1].detach().numpy(), g["s0.out"], **OUT_TOL)
            seen = 0
            for k, v in p.items():
                ref = g["s0.g." + k]
                got = v.grad.numpy() if v.grad is not None else np.zeros_like(ref)
                np.testing.assert_allclose(got, ref, err_msg=k, **GRAD_TOL)
                seen += bool(np.abs(ref).max() > 1e-3)
            assert seen >= 14                                   # 3 convs + map_model + 3 head layers, weight and bias: none vanishes
        opt.step()
    for k, v in p.items():
        np.testing.assert_allclose(v.detach().numpy(), g["final." + k], err_msg=k, **OUT_TOL)
    assert max(float(np.abs(g["final." + k] - g["p." + k]).max()) for k in p) > 3e-3       # (six Adam steps moved them)


def test_metrics_of_the_stored_predictions():
    from two_stage_gnn_amd import two_stage as TS
    g = load_golden("posttrain_gcn")
    y = np.array([d["label"] for d in PR.golden_graphs(g)])
    pred = g["eval.pred"]
    assert set(pred.tolist()) == {0, 1}
    got = TS.metrics_from_confusion(TS.confusion_matrix(y, pred, np.unique(np.concatenate([y, pred]))))
    for k in ("prec", "recall", "acc", "F1"):
        assert got[k] == pytest.approx(float(g["eval." + k]), abs=1e-12), k


class _G:
    def __init__(self, label):
        self.graph = {"label": label}


def test_label_table_validation():
    from two_stage_gnn_amd import post_train as PT
    t = PT.label_table([_G(0), _G(np.int64(1)), {"label": np.array([1])}, _G(np.int32(0))], 2)
    assert t.dtype == np.int32 and t.tolist() == [0, 1, 1, 0]
    for bad, C in ((2, 2), (-1, 2), (1.0, 2), ("1", 2), (np.array([0, 1]), 2), (3, 3)):
        with pytest.raises(ValueError, match="graph 1"):
            PT.label_table([_G(0), _G(bad)], C)
    with pytest.raises(ValueError, match="graph 0"):
        PT.label_table([{"adj": None}], 2)


def test_load_takes_anchor_vectors_and_columns():
    from two_stage_gnn_amd import post_train as PT
    from two_stage_gnn_amd import triplet_stream as TS
    for s in (np.array([0, 1, 4, 1, 1, 6, 3]), np.array([[0], [1], [4]]), [3, 2], U.SCHEDULE[:, :1]):
        out = PT.check_anchors(s, 7)
        assert out.dtype == np.int32 and out.flags["C_CONTIGUOUS"] and out.shape == (len(s), 1)
        assert np.array_equal(out.reshape(-1), np.asarray(s).reshape(-1))
    st = PT.PostTrainStream.__new__(PT.PostTrainStream)          # (load validates before it touches the device)
    st.arena, st.B = TS.pack_arena(U.dataset(), U.NMAX, batch=1), 1
    assert st.arena.caps[0] == 48
    for bad in (U.SCHEDULE, np.zeros((4, 2), dtype=np.int64), np.zeros(0, dtype=np.int64), np.zeros((0, 1), dtype=np.int64), np.array([0, -1]),
                np.array([7]), np.array([0.0, 1.0]), np.zeros((2, 1, 1), dtype=np.int64)):
        with pytest.raises(ValueError):
            st.load(bad)
    assert issubclass(PT.PostTrainStream, TS.ArenaStream) and issubclass(TS.TripletStream, TS.ArenaStream)
    assert PT.PostTrainStream.load is TS.TripletStream.load and PT.PostTrainStream.gather is TS.TripletStream.gather     # shared, not copied


def test_make_head_follows_the_reference_construction_order():
    from two_stage_gnn_amd import post_train as PT
    torch.manual_seed(123)
    head = PT.make_head(24, device=torch.device("cpu"))
    torch.manual_seed(123)
    want = [torch.nn.Linear(24, 64), torch.nn.Linear(64, 32), torch.nn.Linear(32, 2)]
    assert [type(m).__name__ for m in head] == ["Linear", "LeakyReLU", "Linear", "LeakyReLU", "Linear"]
    assert head[1].negative_slope == 0.01 and head[3].negative_slope == 0.01
    for got, ref in zip((head[0], head[2], head[4]), want):
        assert torch.equal(got.weight, ref.weight) and torch.equal(got.bias, ref.bias)
    torch.manual_seed(5)
    other = PT.make_head(10, hidden=(5, 3), n_classes=4, device=torch.device("cpu"))
    assert [tuple(m.weight.shape) for m in (other[0], other[2], other[4])] == [(5, 10), (3, 5), (4, 3)]
    layers = PT.head_layers(type("M", (), {"map_model": torch.nn.Linear(6, 10), "map2_model": other})())
    assert layers is not None and layers[4] == 0.01
    assert PT.head_layers(type("M", (), {"map_model": torch.nn.Linear(6, 10), "map2_model": torch.nn.Linear(10, 2)})()) is None
    assert PT.head_layers(type("M", (), {"map_model": torch.nn.Linear(6, 9), "map2_model": other})()) is None       # widths do not chain
    with pytest.raises(ValueError):
        PT.make_head(8, hidden=(64,), device=torch.device("cpu"))


def test_head_entry_points_validate_on_the_host():
    """the library's word on the shapes, and both launches' refusals, decided before anything is launched (no GPU here)"""
    from two_stage_gnn_amd import _native as nat
    L = nat.lib()
    ok = L.tsgnn_posttrain_head_supported
    assert ok(384, 64, 64, 32, 2, 1) == 1 and ok(2048, 512, 64, 64, 64, 8) == 1 and ok(4, 4, 1, 1, 2, 1) == 1
    for bad in ((6, 64, 64, 32, 2, 1), (2052, 64, 64, 32, 2, 1), (384, 513, 64, 32, 2, 1), (384, 64, 65, 32, 2, 1), (384, 64, 64, 65, 2, 1),
                (384, 64, 64, 32, 1, 1), (384, 64, 64, 32, 65, 1), (384, 64, 64, 32, 2, 0), (384, 64, 64, 32, 2, 9), (0, 64, 64, 32, 2, 1)):
        assert ok(*bad) == 0, bad
    P = 1 << 20                                                    # (pointers are only tested for NULL and alignment here)
    fwd = lambda r=P, R=1, Pn=384, C=2, ld=384: L.tsgnn_posttrain_head_fwd_f32(r, ld, R, Pn, P, P, 64, P, P, 64, P, P, 32, P, P, C, 0.01, P, P, 7,
                                                                                P, P, P, P, P, P, None)
    bwd = lambda r=P, R=1, Pn=384, C=2, ld=384, dw0=P: L.tsgnn_posttrain_head_bwd_f32(r, ld, R, Pn, P, 64, P, 64, P, 32, P, C, 0.01, P, P, 7, P, P, P,
                                                                                       P, None, None, 0, dw0, P, P, P, P, P, P, P, None)
    for f in (fwd, bwd):
        assert f(r=None) == -1 and f(R=0) == -1 and f(R=9) == -1 and f(C=1) == -1 and f(ld=380) == -1      # TSGNN_EINVAL
        assert f(Pn=6, ld=8) == -3 and f(Pn=2052, ld=2052) == -3                                                # TSGNN_EUNSUPPORTED
    assert fwd(r=P + 4) == -3 and fwd(ld=386) == -3 and bwd(dw0=None) == -1
