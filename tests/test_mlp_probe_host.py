"""The MLP probe without a GPU: ``two_stage.MLPProbe`` on CPU tensors (the torch composition that also serves sizes the kernel does
not take) against the fp64 loop of tests/mlp_probe_oracle.py, the default initial parameters against the reference's construction,
and the host-side argument checks of the C entry points of csrc/mlp_probe.hip."""
import numpy as np
import pytest
import torch

import mlp_probe_oracle as MO


def _got(probe, Q):
    return {"losses": probe.losses_.numpy(), "logits": probe.decision_function(Q).numpy(), "params": [p.numpy() for p in probe._params]}


@pytest.mark.parametrize("case", [(7, 16, 8, 4, 2), (4, 37, 5, 8, 3), (6, 64, 16, 6, 2)], ids=lambda c: "seed%d_n%d_q%d_D%d_C%d" % c)
def test_cpu_tensors_run_the_torch_composition_against_fp64(case):
    from two_stage_gnn_amd import two_stage as TS
    ref = MO.case(*case)
    C = case[4]
    X, Q = torch.from_numpy(ref["X"]), torch.from_numpy(ref["Q"])
    keep = [t.clone() for t in ref["init"]]
    probe = TS.MLPProbe().fit(X, ref["y"], classes=np.arange(C), init=ref["init"])
    assert not probe.kernel_ok() and probe.losses_.shape == (case[1],)
    assert all(torch.equal(a, b) for a, b in zip(keep, ref["init"]))                      # init is copied, never written
    MO.check_run("cpu %s" % (case,), _got(probe, Q), ref)
    pred = probe.predict(Q)
    assert isinstance(pred, torch.Tensor)
    MO.check_predictions("cpu %s" % (case,), pred.numpy(), ref["f64"]["logits"])
    assert probe.score(Q, ref["yq"]) == float((pred.numpy() == ref["yq"]).mean())
    # a split pass continues the moments and the step count: bit for bit the single pass
    h = case[1] // 2
    split = TS.MLPProbe().fit(X[:h], ref["y"][:h], classes=np.arange(C), init=ref["init"]).partial_fit(X[h:], ref["y"][h:])
    assert all(torch.equal(a, b) for a, b in zip(split._params, probe._params))
    assert torch.equal(split.losses_, probe.losses_[h:])
    seq = probe.module()
    with torch.no_grad():
        assert torch.equal(seq(Q), probe.decision_function(Q))


@pytest.mark.parametrize("seed", [0, 3])
def test_default_initial_parameters_are_the_reference_construction(seed):
    """after torch.manual_seed(s) the probe starts from what nn.Linear(E, 64), nn.Linear(64, 32), nn.Linear(32, 2), built on the host
    in that order after the same seed, hold"""
    from two_stage_gnn_amd import two_stage as TS
    E = 20
    want = MO.initial(seed, E, (64, 32), 2)
    X, y, _, _ = MO.KO.synthetic(1, 5, 1, E, 2, 0)
    torch.manual_seed(seed)
    probe = TS.MLPProbe(lr=0.0).fit(torch.from_numpy(X), np.arange(5) % 2)               # (lr = 0: the pass leaves the parameters alone)
    assert [tuple(p.shape) for p in probe._params] == [tuple(w.shape) for w in want]
    assert all(torch.equal(p, w) for p, w in zip(probe._params, want))


def test_labels_and_containers_on_the_cpu():
    from two_stage_gnn_amd import two_stage as TS
    ref = MO.case(7, 16, 8, 4, 2)
    y = np.where(ref["y"] == 0, 3, 7)
    probe = TS.MLPProbe().fit(torch.from_numpy(ref["X"]), y, init=ref["init"])
    assert probe.classes_.tolist() == [3, 7]
    pred = probe.predict(torch.from_numpy(ref["Q"]))
    assert set(pred.tolist()) <= {3, 7} and pred.dtype == torch.int64
    assert probe.score(torch.from_numpy(ref["Q"]), np.full(8, 5)) == 0.0                 # a label outside classes_ counts as wrong
    with pytest.raises(ValueError):
        probe.partial_fit(torch.from_numpy(ref["X"][:2]), [3, 5])
    with pytest.raises(ValueError):
        TS.MLPProbe().fit(torch.zeros(3, 4), [0, 1])
    with pytest.raises(ValueError):
        TS.MLPProbe(hidden=(16, 8)).fit(torch.from_numpy(ref["X"]), y, init=ref["init"])  # init of another shape


def test_abi_declares_the_probe_entry_points_and_refuses_bad_arguments():
    """no GPU: every refusal below is decided on the host before anything is launched"""
    from two_stage_gnn_amd import _native as nat
    decls = nat.parse_header()
    assert [n for _, n in decls["tsgnn_mlp_probe_fit_f32"][1]] == [
        "x", "ld_x", "cls", "n", "dim", "h1", "h2", "n_classes", "w1", "b1", "w2", "b2", "w3", "b3", "exp_avg", "exp_avg_sq", "step0",
        "lr", "beta1", "beta2", "eps", "negative_slope", "loss", "stream"]
    assert [n for _, n in decls["tsgnn_mlp_probe_predict_f32"][1]] == [
        "q", "ld_q", "n_query", "dim", "h1", "h2", "n_classes", "w1", "b1", "w2", "b2", "w3", "b3", "negative_slope", "logits", "pred",
        "query_class", "correct", "stream"]
    L = nat.lib()
    assert L.tsgnn_mlp_probe_supported(1024, 64, 64, 64) == 1 and L.tsgnn_mlp_probe_supported(1025, 64, 64, 64) == 0
    assert L.tsgnn_mlp_probe_supported(1, 1, 1, 2) == 1 and L.tsgnn_mlp_probe_supported(64, 64, 32, 1) == 0
    assert L.tsgnn_mlp_probe_supported(64, 65, 32, 2) == 0 and L.tsgnn_mlp_probe_supported(64, 64, 65, 2) == 0
    assert L.tsgnn_mlp_probe_supported(64, 64, 32, 65) == 0 and L.tsgnn_mlp_probe_supported(0, 64, 32, 2) == 0
    P = 1 << 20
    hyper = (1e-3, 0.9, 0.999, 1e-8, 0.01)

    def fit(x=P, ld=64, n=10, dim=64, h1=64, h2=32, C=2, m=P, v=P):
        return L.tsgnn_mlp_probe_fit_f32(x, ld, P, n, dim, h1, h2, C, P, P, P, P, P, P, m, v, 0, *hyper, None, None)

    def predict(q=P, ld=64, n=5, dim=64, h1=64, h2=32, C=2, qc=None, correct=None):
        return L.tsgnn_mlp_probe_predict_f32(q, ld, n, dim, h1, h2, C, P, P, P, P, P, P, 0.01, None, P, qc, correct, None)

    for call in (fit, predict):
        assert call(dim=0) == -1                                                  # dim < 1
        assert call(ld=32) == -1                                                  # rows shorter than dim
        assert call(ld=66) == -1                                                  # stride not a multiple of 4 floats
        assert call(C=1) == -1
        assert call(h1=65) == -1
        assert call(n=0) == -1
    assert fit(x=None) == -1 and predict(q=None) == -1
    assert fit(m=P, v=None) == -1 and fit(m=None, v=P) == -1                      # the moments come together or not at all
    assert predict(qc=P, correct=None) == -1 and predict(qc=None, correct=P) == -1
    assert fit(x=P + 4) == -3 and predict(q=P + 4) == -3                          # misaligned rows: not this kernel's layout
    assert fit(dim=1024, ld=1024, m=None, v=None) == -3                           # past 512 columns the W1 moments need the caller's buffers
