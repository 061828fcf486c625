#!/usr/bin/env python3
"""Golden vectors of the reference's EigenGCN post-training loop (test infrastructure; never imported by the product path).

Same rules and stubs as scripts/gen_golden_eigen_triplet.py (whose helpers it imports): the reference's Code/eigengcn is imported
read-only with ``.cuda()`` turned into the identity and SpectralClustering replaced by fixed chunk labels.  Three ``.graph`` dicts of
different sizes, labelled, are built from the reference's own ``Graphs(...).coarsening_pooling``; the reference's model and its FIRST
optimiser (train_triplet_pre_train.py:94: Adam with ``lr`` and ``weight_decay``) take

  1. one triplet step (:117-139: the reference's ``tripletnet``, margin loss, ``clip_grad_norm``, ``optimizer.step()``), so that the
     optimiser's moments and step count are no longer trivial, then
  2. three post-training steps of :192-247, one per graph as the anchor: the dead ``model.map_model = pred_model`` installed as the
     driver installs it, ``ypred = model(...)`` at B = 1 under ``model.train()`` with the pooled adjacencies passed WITHOUT a batch
     dimension as the driver passes them, ``loss = model.loss(ypred, label)``, ``clip_grad_norm(model.parameters(), clip)`` and
     ``optimizer.step()`` of the FIRST Adam.

Stored (data only, tests/golden/posttrain_eigen.npz): the graph arrays and labels, the parameters before the run, the triplet step's
pre-clip gradients and the parameters after it, and per post-training step ``ypred``, the loss, the pre-clip gradients and the
parameters after.  ``clip`` is chosen between the smallest and the largest gradient norm of a dry run, so that it is active in at
least one step and inactive in at least one.  Asserted: every loss > 0, a non-zero gradient on every conv and pred_model weight in
every step, the clip active and inactive, the dead head's parameters unmoved.

Usage:  python scripts/gen_golden_posttrain_eigen.py REFERENCE_ROOT        (rewrites tests/golden/posttrain_eigen.npz)
"""
import contextlib
import copy
import io
import os
import sys

import numpy as np
import torch
import torch.nn as nn

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gen_golden_eigen as GE  # noqa: E402
import gen_golden_eigen_triplet as GT  # noqa: E402

NAME = "posttrain_eigen"
CFG = dict(J=2, Jf=1, con_final=1, pool_sizes=[4], sizes=[17, 9, 13], nmax=18)
F_IN, HIDDEN, EMB, LAYERS, LABEL_DIM, PRED_HIDDEN = 7, 8, 4, 3, 6, [6]            # (widths that keep the file small: nine parameter sets)
LR, WEIGHT_DECAY, MARGIN = 1e-3, 1e-2, 1.5
LABELS = [0, 5, 2]                                  # the first and the last class occur


def _norm(model):
    return float(torch.sqrt(sum((p.grad.double() ** 2).sum() for p in model.parameters() if p.grad is not None)))


def _clip(model, clip):
    fn = getattr(nn.utils, "clip_grad_norm", None) or nn.utils.clip_grad_norm_
    fn(model.parameters(), clip)


def _grads(model):
    return {k: (p.grad if p.grad is not None else torch.zeros_like(p)).detach().numpy().copy() for k, p in model.named_parameters()
            if not k.startswith("map_model")}


def _params(model):
    return {k: v.detach().numpy().copy() for k, v in model.state_dict().items() if not k.startswith("map_model")}


def model_inputs(d, L, J, Jf):
    """one ``.graph`` dict -> the positional arguments of the reference's encoder at B = 1, float32.  Features, adjacency and every
    pooling matrix carry the batch dimension; the pooled adjacencies do NOT ([N, N]): that is how the driver's post-training loop hands
    them over (:192-247), and the fixture keeps it"""
    f32 = lambda key: torch.from_numpy(np.asarray(d[key], dtype=np.float32))
    pools = {lev: [f32("pool_adj_%d_%d" % (lev, j))[None] for j in range(J if lev < L else Jf)] for lev in range(L + (1 if Jf else 0))}
    return (f32("feats")[None], f32("adj")[None], [f32("adj_pool_%d" % (lev + 1)) for lev in range(L)], np.array([d["num_nodes"]]),
            [[d["num_nodes_%d" % (lev + 1)]] for lev in range(L)], pools)


def post_step(model, optimizer, obj, clip):
    """one post-training step on the anchor ``obj``: the reference's model and ``model.loss`` on the anchor's label, ``clip_grad_norm``
    over all parameters, a step of the optimiser handed in (the FIRST Adam) -> (ypred, loss, pre-clip gradients, their norm)"""
    d = obj.graph
    model.zero_grad()
    with contextlib.redirect_stdout(io.StringIO()):
        ypred = model(*model_inputs(d, len(CFG["pool_sizes"]), CFG["J"], CFG["Jf"]))
    loss = model.loss(ypred, torch.tensor([int(d["label"])], dtype=torch.long))
    loss.backward()
    grads, norm = _grads(model), _norm(model)
    _clip(model, clip)
    optimizer.step()
    return ypred.detach().numpy().copy(), float(loss.item()), grads, norm


def run(cp, enc, tn, seed, clip, out=None):
    """the whole sequence from ``seed``; -> the post-training steps' pre-clip gradient norms (and fills ``out``)"""
    rng = np.random.default_rng(seed)
    gen = torch.Generator().manual_seed(seed)
    J, Jf, N = CFG["J"], CFG["Jf"], CFG["nmax"]
    dicts, labels = [], []
    for n, y in zip(CFG["sizes"], LABELS):
        d, lab = GT.graph_dict(cp, rng, gen, n, N, CFG, F_IN)
        d["label"] = y
        dicts.append(d)
        labels.append(lab)
    objs = [GT._G(d) for d in dicts]

    class Args:
        bias = True
        con_final = CFG["con_final"]
        pool_sizes = "_".join(str(s) for s in CFG["pool_sizes"])
        num_pool_matrix = J
        num_pool_final_matrix = Jf
    with contextlib.redirect_stdout(io.StringIO()):
        m = enc.WavePoolingGcnEncoder(N, F_IN, HIDDEN, EMB, LABEL_DIM, LAYERS, num_pool_matrix=J, num_pool_final_matrix=Jf,
                                      pool_sizes=CFG["pool_sizes"], pred_hidden_dims=PRED_HIDDEN, concat=True, bn=True, mask=1, args=Args())
    with torch.no_grad():
        for p in m.parameters():
            p.copy_(torch.randn(p.shape, generator=gen) * 0.5)
    optimizer = torch.optim.Adam(filter(lambda p: p.requires_grad, m.parameters()), lr=LR, weight_decay=WEIGHT_DECAY)     # :94
    m.train()
    res = dict(J=J, Jf=Jf, con_final=CFG["con_final"], mask=1, nmax=N, num_layers=LAYERS, hidden=HIDDEN, emb=EMB, label_dim=LABEL_DIM,
               pred_hidden=np.asarray(PRED_HIDDEN, dtype=np.int64), pool_sizes=np.asarray(CFG["pool_sizes"]), same_ap=0,
               margin=np.float32(MARGIN), seed=seed, lr=np.float64(LR), weight_decay=np.float64(WEIGHT_DECAY), clip=np.float64(clip),
               n_steps=len(objs))
    for t, (d, lab) in enumerate(zip(dicts, labels)):
        for k, v in d.items():
            if k != "assign_feats":                          # (read by the reference, never used)
                res["t%d.%s" % (t, k)] = np.asarray(v)
        for i, l in enumerate(lab):
            res["t%d.labels_%d" % (t, i)] = l
    for k, v in _params(m).items():
        res["p." + k] = v
    # 1. one triplet step (:117-139)
    net = tn.tripletnet(m, Args())
    m.zero_grad()
    with contextlib.redirect_stdout(io.StringIO()):
        dist_p, dist_n, _, _, _ = net(*objs)
    loss = nn.MarginRankingLoss(margin=MARGIN)(dist_p, dist_n, torch.full_like(dist_p, -1.0))
    loss.backward()
    res["triplet.loss"] = np.float32(loss.item())
    res["triplet.norm"] = np.float64(_norm(m))
    for k, v in _grads(m).items():
        res["triplet.g." + k] = v
    _clip(m, clip)
    optimizer.step()
    for k, v in _params(m).items():
        res["triplet.p." + k] = v
    # 2. the dead head (:170-183) and three post-training steps (:192-247)
    m.map_model = nn.Sequential(nn.Linear(EMB, 64), nn.LeakyReLU(), nn.Linear(64, 32), nn.LeakyReLU(), nn.Linear(32, 2))
    dead = copy.deepcopy(m.map_model.state_dict())
    norms, ok = [], float(loss.item()) > 0
    for s, a in enumerate(objs):
        ypred, l, grads, norm = post_step(m, optimizer, a, clip)
        norms.append(norm)
        ok = ok and l > 0 and all(np.any(v != 0) for k, v in grads.items() if k.endswith("weight"))
        res["s%d.ypred" % s], res["s%d.loss" % s], res["s%d.norm" % s] = ypred, np.float32(l), np.float64(norm)
        for k, v in grads.items():
            res["s%d.g.%s" % (s, k)] = v
        for k, v in _params(m).items():
            res["s%d.p.%s" % (s, k)] = v
    assert all(torch.equal(v, m.map_model.state_dict()[k]) for k, v in dead.items()), "the dead head moved"
    assert all(p.grad is None for p in m.map_model.parameters()), "the dead head received a gradient"
    if out is not None:
        out.update(res)
    return norms, ok


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    ref_dir = os.path.join(sys.argv[1], "Code", "eigengcn")
    if not os.path.isdir(ref_dir):
        sys.exit("no Code/eigengcn under %s" % sys.argv[1])
    cp, enc = GE._import_reference(ref_dir)
    with contextlib.redirect_stdout(io.StringIO()):
        import tripletnet as tn
    for seed in range(500, 560):
        norms, ok = run(cp, enc, tn, seed, 1e9)               # dry run: no clipping, the norms of the three steps
        if not ok or max(norms) < 1.2 * min(norms) or min(norms) < 0.05 * max(norms):     # (no step with a saturated soft-max)
            continue
        clip = float("%.3g" % np.sqrt(min(norms) * max(norms)))
        out = {}
        norms, ok = run(cp, enc, tn, seed, clip, out)
        if ok and min(norms) < clip < max(norms):
            break
    else:
        raise AssertionError("no seed with positive losses, non-zero weight gradients and a clip that is active and inactive")
    assert all(float(out["s%d.loss" % s]) > 0 for s in range(3))
    path = os.path.join(GE.OUT_DIR, NAME + ".npz")
    np.savez_compressed(path, **{k: np.asarray(v) for k, v in out.items()})
    print("wrote", path, "seed %d clip %g norms %s" % (seed, clip, " ".join("%.4g" % n for n in norms)), "%.1f KB" % (os.path.getsize(path) / 1024))
    assert os.path.getsize(path) <= os.path.getsize(os.path.join(GE.OUT_DIR, "posttrain_diffpool.npz"))


if __name__ == "__main__":
    main()
