"""The 2stg+ post-training loop for --method=GAT and --method=soft-assign in plain torch on the CPU (train_triplet_pre_train.py:233-262),
on top of oracle/dense_ref.py and tests/posttrain_ref.py's head, in whatever dtype the parameters have: float64 as the reference of
tests/test_posttrain_families_host.py and of the GPU tests' yardstick (tests/fp32_yardstick.py), float32 as its ``cpu32``.

GAT: ``DGATEncoderGraph(final_dim='output_dim')`` returns the max-readout row first (encoders_GAT.py:189-198), so the loop's ``pred`` is
that row and ``out = map2_model(map_model(pred))`` never reaches the loss.  DiffPool: ``pred, out`` are the head and ``map_model`` on the
concatenated readout rows of every level (encoders.py:396-399)."""
import numpy as np
import torch
import torch.nn.functional as F

import posttrain_ref as PR
from oracle import dense_ref as R


class GraphObj:
    """stands for the networkx graph object whose ``.graph`` dict the drop-ins read"""

    def __init__(self, d):
        self.graph = {"adj": d["adj"], "feats": d["feats"], "num_nodes": d["num_nodes"], "assign_feats": d["feats"], "label": d["label"]}


def golden_objects(g):
    return [GraphObj(d) for d in PR.golden_graphs(g)]


def _inputs(p, d):
    dt = next(iter(p.values())).dtype
    return torch.as_tensor(d["feats"]).to(dt)[None], torch.as_tensor(d["adj"]).to(dt)[None]


def _mlp(p, out, slope=0.01):
    h = F.leaky_relu(F.linear(out, p["map2_model.0.weight"], p["map2_model.0.bias"]), slope)
    h = F.leaky_relu(F.linear(h, p["map2_model.2.weight"], p["map2_model.2.bias"]), slope)
    return F.linear(h, p["map2_model.4.weight"], p["map2_model.4.bias"])


def gat_step(p, d):
    """-> (loss, pred, out): pred is the readout row, the loss the doubled soft-max cross-entropy over its columns"""
    x, adj = _inputs(p, d)
    pred, mapped = R.gat_encoder(p, x, adj, final_dim="output_dim")            # (x, map_model(x))
    return F.cross_entropy(F.softmax(pred, dim=1), torch.tensor([int(d["label"])])), pred, _mlp(p, mapped)


def diffpool_step(p, d, num_pooling=1):
    x, adj = _inputs(p, d)
    r = R.diffpool_encoder(p, x, adj, [int(d["num_nodes"])], num_pooling, assign_x=x, final_dim="output_dim")[0]    # the readout rows
    return PR.head(p, r, torch.tensor([int(d["label"])]))


def run_loop(step, p0, dicts, lr, dtype):
    """the loop from the parameters ``p0`` ({name: array}) in ``dtype`` -> {'s<i>.pred' / '.out' / '.loss', 's0.g.<name>' (absent for a
    parameter the loss does not reach), 'final.<name>'} as ``dtype`` tensors"""
    p = {k: torch.as_tensor(np.asarray(v)).to(dtype).clone().requires_grad_(True) for k, v in p0.items()}
    opt = torch.optim.Adam(list(p.values()), lr=lr)                            # (a parameter without gradient is skipped, as in the reference)
    res = {}
    for s, d in enumerate(dicts):
        opt.zero_grad(set_to_none=True)
        loss, pred, out = step(p, d)
        loss.backward()
        if s == 0:
            res.update({"s0.g." + k: v.grad.detach().clone() for k, v in p.items() if v.grad is not None})
        opt.step()
        res["s%d.pred" % s], res["s%d.out" % s], res["s%d.loss" % s] = pred.detach(), out.detach(), loss.detach().reshape(1)
    res.update({"final." + k: v.detach() for k, v in p.items()})
    return res


def initial(g):
    """the float parameters of a fixture's initial state dict (``p.``)"""
    return {k[2:]: v for k, v in g.items() if k.startswith("p.") and np.issubdtype(np.asarray(v).dtype, np.floating)}


_RUNS = {}


def reference_runs(name, g):
    """(ref64, cpu32) of a fixture's loop, computed once per process and shared by the tests: leave them unchanged"""
    if name not in _RUNS:
        step = gat_step if name == "posttrain_gat" else diffpool_step
        dicts = PR.golden_graphs(g)
        _RUNS[name] = tuple(run_loop(step, initial(g), dicts, float(g["lr"]), dt) for dt in (torch.float64, torch.float32))
    return _RUNS[name]
