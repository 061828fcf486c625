"""The datasets, models, schedules and references the GAT triplet-stream tests share (tests/test_gat_stream_host.py,
tests/test_gpu_gat_stream.py).

Datasets (graph objects as ``gat_triplet.pack_host`` reads them):
  small3 / small8   the eleven shapes of tests/test_gpu_gat_triplet.py's ASM_GRAPHS at Nmax 12 (a full graph without a ghost row, n = 1, an
                    edge-less graph, directed graphs), fin 3 (ldf 4) and fin 8 (ldf 8); pieces start off 16 bytes in rows and in entries
  big               four graphs at Nmax 320, n = 40, 130, 250, 320, fin 8, p_edge 0.06: the largest has nnz > 2 x 2048 and nr * ldf > 2048,
                    so a piece spans several copy chunks of the gather launch and its unaligned head / tail paths run
Schedules: the largest graph in each of the three places, the largest triplet followed by the smallest (what the previous gather left
must be inert), one object three times, every graph at least once; small also holds a triplet without any edge (E = 0).
Models: hidden 8, embedding 8; "l2" = 2 layers with heads [2, 2], "l3" = 3 layers with heads [1, 2, 2]: two head counts, so two
indicators.  (``DGATEncoderGraph`` builds its last layer for an input of hidden x heads[-1] columns, as the reference does, so the layer
before it needs heads[-1] heads: heads [2, 1, 2] cannot be run, by the drop-in either.)"""
import copy

import numpy as np
import torch
import torch.nn.functional as F

import test_gat_triplet_host as H
from util_graphs import dense_batch

MARGIN = 10.0          # (distances of these models are ~1: the hinge max(0, dist_p - dist_n + margin) is active in every entry)
NMAX_SMALL = 12
ASM_GRAPHS = [(9, "directed"), (12, "sym"), (1, "sym"), (7, "empty"), (10, "sym"), (5, "sym"), (11, "sym"), (12, "directed"), (6, "sym"),
              (3, "directed"), (8, "sym")]          # tests/test_gpu_gat_triplet.py's (not imported: that module is GPU-only)
BIG_SIZES = [40, 130, 250, 320]
BIG_NMAX, BIG_P = 320, 0.06
FIN = {"small3": 3, "small8": 8, "big": 8}
SCHEDULES = {
    "small": np.array([[1, 7, 6], [2, 3, 9], [4, 4, 4], [0, 1, 5], [8, 10, 1], [3, 2, 3], [7, 2, 0], [5, 9, 10], [6, 8, 4], [1, 1, 7]],
                      dtype=np.int64),
    "big": np.array([[3, 2, 1], [0, 0, 1], [1, 3, 0], [2, 1, 3], [0, 1, 2], [3, 3, 3], [0, 2, 0], [2, 2, 1]], dtype=np.int64),
}
MODELS = {"l2": (2, [2, 2]), "l3": (3, [1, 2, 2])}
# the (dataset, model) pairs of the step tests: both ldf with the two-layer model, the three-layer model once, the big dataset
CASES = [("small3", "l2"), ("small8", "l2"), ("small8", "l3"), ("big", "l2")]

_DATA = {}


def schedule(name):
    return SCHEDULES["big" if name == "big" else "small"]


def dataset(name):
    """-> the graph objects (built once per process; treat as read-only)"""
    if name not in _DATA:
        if name == "big":
            x, adj, sz = dense_batch(31, len(BIG_SIZES), BIG_NMAX, FIN[name], sizes=BIG_SIZES, p_edge=BIG_P)
            _DATA[name] = [H.GraphObj(adj[b].numpy().astype(np.float64), x[b].numpy(), int(sz[b]), label=b % 2) for b in range(len(BIG_SIZES))]
        else:
            _DATA[name] = [H.make_obj(100 + i, n, nmax=NMAX_SMALL, fin=FIN[name], kind=kind) for i, (n, kind) in enumerate(ASM_GRAPHS)]
    return _DATA[name]


def model(name, cfg, mode="eval", dev="cuda", dropouts=None):
    """the seeded encoder of a (dataset, model) pair: equal parameters at every call"""
    from two_stage_gnn_amd import gat_encoders as G
    layers, heads = MODELS[cfg]
    torch.manual_seed(11)
    m = G.DGATEncoderGraph(FIN[name], 8, 8, 2, None, num_layers=layers, num_heads=list(heads), neg_input_slopes=[0.2] * layers,
                           dropouts=dropouts or [0.0] * layers, final_dim="output_dim")
    return m.to(dev).train(mode == "train")


def dense_of(objs, dev="cuda"):
    """(feats [B, Nmax, F], adj [B, Nmax, Nmax] as the 0 / 1 mask, sizes) of graph objects, for the module's own B = 1 calls"""
    x = torch.as_tensor(np.stack([np.asarray(o.graph["feats"], dtype=np.float32) for o in objs])).to(dev)
    adj = torch.as_tensor(np.stack([(np.asarray(o.graph["adj"]) > 0).astype(np.float32) for o in objs])).to(dev)
    return x, adj, np.array([int(o.graph["num_nodes"]) for o in objs], dtype=np.int64)


def grads(m):
    return {k: p.grad.detach().clone() for k, p in m.named_parameters() if p.grad is not None}


_REF = {}


def three_calls(name, cfg, ids):
    """the reference's arithmetic on schedule entry ``ids``: three B = 1 dense calls of a deep copy of the seeded module, torch's
    distances, torch's margin loss, backward — computed once per (dataset, model, entry): (outputs, loss, {parameter: grad}).  Eval and
    training mode agree (all dropouts are 0).  Entries that name a graph without any edge are computed like every other one (nnz = 0:
    tests/test_gpu_attn_ops.py::test_encoder_on_a_graph_without_any_edge)"""
    key = (name, cfg, tuple(int(i) for i in ids))
    if key not in _REF:
        m = copy.deepcopy(model(name, cfg))
        x, adj, sz = dense_of([dataset(name)[i] for i in key[2]])
        e = [m(x[b:b + 1], adj[b:b + 1], sz[b:b + 1])[1] for b in range(3)]
        outs = (F.pairwise_distance(e[0], e[1], 2), F.pairwise_distance(e[0], e[2], 2), e[0], e[1], e[2])
        loss = torch.nn.MarginRankingLoss(margin=MARGIN)(outs[0], outs[1], torch.full_like(outs[0], -1.0))
        loss.backward()
        _REF[key] = (tuple(o.detach() for o in outs), loss.detach(), {k: (p.grad.detach().clone() if p.grad is not None else None)
                                                                      for k, p in m.named_parameters()})
    return _REF[key]


def restate(objs):
    """records [G, 8] and the pieces, graph by graph, from ``pack_host``'s numbers and a layout written out here: nine sections, each
    rounded up to 4 words"""
    from two_stage_gnn_amd import gat_triplet as GT
    a4 = lambda v: (v + 3) // 4 * 4
    rec, bufs, words = [], [], 0
    for i, o in enumerate(objs):
        p = GT.pack_host(o)
        parts = [p["rowptr"], p["rowptr_t"], p["col"], p["col_t"], p["src_e_t"], p["inv_e_t"], p["iso_rows"], p["iso_w"].view(np.int32),
                 p["feats"].reshape(-1).view(np.int32)]
        buf = np.concatenate([np.concatenate([q, np.zeros(a4(q.size) - q.size, dtype=np.int32)]) for q in parts])
        rec.append([words, p["n"], p["nr"], p["nnz"], p["k"], p["nmax"] - p["n"], i, 0])
        bufs.append(buf)
        words += buf.size
    return np.array(rec, dtype=np.int64), bufs
