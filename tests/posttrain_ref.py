"""The 2stg+ post-training step in plain torch on the CPU (train_triplet_pre_train.py:249-256): the head as the same expression as
``:256`` on ``map_model`` and the replacement ``Sequential``, parametrised by dtype so that it serves as ``ref64`` (float64) and as
``cpu32`` (the yardstick of tests/fp32_yardstick.py), and the whole step on top of ``oracle/dense_ref.gcn_encoder_readouts``.

Parameter names are the state dict's: ``map_model.{weight,bias}`` and ``map2_model.{0,2,4}.{weight,bias}``."""
import torch
import torch.nn.functional as F

from oracle import dense_ref as R

HEAD_KEYS = ("map_model.weight", "map_model.bias", "map2_model.0.weight", "map2_model.0.bias", "map2_model.2.weight",
             "map2_model.2.bias", "map2_model.4.weight", "map2_model.4.bias")


def head(p, r, label, slope=0.01):
    """readout rows r [R, P], label [R] int64 -> (loss, pred [R, C], out [R, E]); dtype and autograd are the inputs'"""
    out = F.linear(r, p["map_model.weight"], p["map_model.bias"])
    h = F.leaky_relu(F.linear(out, p["map2_model.0.weight"], p["map2_model.0.bias"]), slope)
    h = F.leaky_relu(F.linear(h, p["map2_model.2.weight"], p["map2_model.2.bias"]), slope)
    pred = F.linear(h, p["map2_model.4.weight"], p["map2_model.4.bias"])
    return F.cross_entropy(F.softmax(pred, dim=1), label), pred, out


def head_grads(p, r, label, upstream, dtype, slope=0.01):
    """the head in ``dtype`` from float32 inputs -> {'loss', 'z', 'out', 'dr', and the eight HEAD_KEYS gradients} for an upstream
    gradient of ``upstream`` on the loss"""
    q = {k: p[k].detach().to(dtype).clone().requires_grad_(True) for k in HEAD_KEYS}
    rr = r.detach().to(dtype).clone().requires_grad_(True)
    loss, pred, out = head(q, rr, label.long(), slope)
    loss.backward(gradient=torch.tensor(upstream, dtype=dtype))
    res = {"loss": loss.detach().reshape(1), "z": pred.detach(), "out": out.detach(), "dr": rr.grad}
    res.update({k: q[k].grad for k in HEAD_KEYS})
    return res


def step(p, d, slope=0.01):
    """one graph dict (adj, feats, label) through the oracle's encoder at B = 1 and the head -> (loss, pred, out)"""
    x = torch.as_tensor(d["feats"])[None]
    adj = torch.as_tensor(d["adj"])[None]
    r = R.gcn_encoder_readouts(p, x, adj, bn=True, concat=True)
    return head(p, r, torch.tensor([int(d["label"])]), slope)


def golden_graphs(g):
    """the graph dicts of tests/golden/posttrain_gcn.npz, in the order of its steps"""
    return [{"adj": g["g%d.adj" % i], "feats": g["g%d.feats" % i], "num_nodes": int(g["g%d.num_nodes" % i]), "label": int(g["g%d.label" % i])}
            for i in range(int(g["n_graphs"]))]
