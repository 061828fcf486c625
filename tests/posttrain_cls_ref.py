"""The two classification heads of csrc/posttrain_cls.hip restated by hand, forward AND backward, without autograd, parametrised by
dtype so that one text serves as ``ref64`` (float64) and as ``cpu32`` (the yardstick of tests/fp32_yardstick.py):

  mlp3 + nll (Code/sag/network.py:48-53 + F.nll_loss):   a1 = relu(lin1(r)) * mask * keep_scale, a2 = relu(lin2(a1)),
      logp = log_softmax(lin3(a2)), loss = mean_i -logp[i, y_i]
  mlp2 + CE  (WavePoolingGcnEncoder.pred_model + F.cross_entropy):   h = relu(W1 r + b1), z = W2 h + b2, p = softmax(z),
      loss = mean_i (logsumexp(z_i) - z_i[y_i])

tests/test_posttrain_sag_eigen_host.py anchors both to float64 autograd.  TEST INFRASTRUCTURE: no project kernel."""
import torch

MLP3_KEYS = ("w1", "b1", "w2", "b2", "w3", "b3")
MLP2_KEYS = ("w1", "b1", "w2", "b2")


def _onehot(y, C, dtype):
    return torch.zeros(y.numel(), C, dtype=dtype).scatter_(1, y.long().view(-1, 1), 1.0)


def _lin(x, w, b):
    return x @ w.t() + (b if b is not None else 0.0)


def mlp3_nll(p, r, y, upstream=1.0, dtype=torch.float64, mask=None, keep_scale=1.0):
    """p: {'w1' [D1, D0], 'b1', 'w2' [D2, D1], 'b2', 'w3' [C, D2], 'b3'}, r [R, D0], y [R] class indices, mask [R, D1] of 0 / 1 or
    None -> {'a1', 'a2', 'logp', 'loss' [1], 'dr', 'dw1', 'db1', 'dw2', 'db2', 'dw3', 'db3'} for an upstream gradient on the loss"""
    q = {k: p[k].detach().to(dtype) for k in MLP3_KEYS}
    r = r.detach().to(dtype)
    R, C = r.size(0), q["w3"].size(0)
    gate = torch.ones(R, q["w1"].size(0), dtype=dtype) if mask is None else mask.to(dtype)
    gate = gate * dtype_scalar(keep_scale, dtype)
    a1 = torch.relu(_lin(r, q["w1"], q["b1"])) * gate
    a2 = torch.relu(_lin(a1, q["w2"], q["b2"]))
    z = _lin(a2, q["w3"], q["b3"])
    m = z.max(dim=1, keepdim=True).values
    logp = z - (m + (z - m).exp().sum(dim=1, keepdim=True).log())
    oh = _onehot(y, C, dtype)
    loss = -(logp * oh).sum() / R
    dz = (logp.exp() - oh) * (dtype_scalar(upstream, dtype) / R)
    dz2 = (dz @ q["w3"]) * (a2 > 0).to(dtype)
    dz1 = (dz2 @ q["w2"]) * (a1 > 0).to(dtype) * gate
    return {"a1": a1, "a2": a2, "logp": logp, "loss": loss.reshape(1), "dr": dz1 @ q["w1"],
            "dw1": dz1.t() @ r, "db1": dz1.sum(0), "dw2": dz2.t() @ a1, "db2": dz2.sum(0), "dw3": dz.t() @ a2, "db3": dz.sum(0)}


def mlp2_ce(p, r, y, upstream=1.0, dtype=torch.float64):
    """p: {'w1' [H, D], 'b1' or None, 'w2' [C, H], 'b2' or None}, r [R, D], y [R] -> {'h', 'z', 'p', 'loss' [1], 'dr', 'dw1', 'db1',
    'dw2', 'db2'}"""
    q = {k: (p[k].detach().to(dtype) if p.get(k) is not None else None) for k in MLP2_KEYS}
    r = r.detach().to(dtype)
    R, C = r.size(0), q["w2"].size(0)
    h = torch.relu(_lin(r, q["w1"], q["b1"]))
    z = _lin(h, q["w2"], q["b2"])
    m = z.max(dim=1, keepdim=True).values
    e = (z - m).exp()
    se = e.sum(dim=1, keepdim=True)
    prob = e / se
    oh = _onehot(y, C, dtype)
    loss = ((m + se.log()).sum() - (z * oh).sum()) / R
    dz = (prob - oh) * (dtype_scalar(upstream, dtype) / R)
    dh = (dz @ q["w2"]) * (h > 0).to(dtype)
    return {"h": h, "z": z, "p": prob, "loss": loss.reshape(1), "dr": dh @ q["w1"], "dw1": dh.t() @ r, "db1": dh.sum(0),
            "dw2": dz.t() @ h, "db2": dz.sum(0)}


def dtype_scalar(v, dtype):
    """a python number rounded as the kernel's float argument is when dtype is float32"""
    return float(torch.tensor(v, dtype=dtype))
