"""The datasets, models, schedules and references the EigenGCN triplet-stream tests share (tests/test_eigen_stream_host.py,
tests/test_gpu_eigen_stream.py).

Datasets (``.graph`` dicts through ``eigen_two_stage_util.make_result`` / ``make_dict`` with ``odd=False``: the stream refuses directed
edges):
  small   twelve graphs at Nmax 19, fin 6 (ldf 8), per configuration of ``eigen_two_stage_util.CONFIGS``: graph 0 is full (n = Nmax),
          graph 1 has unassigned rows, graphs 2 and 3 pool to ONE cluster (the pooled level has one node and no entry)
  big     four graphs of 40 / 130 / 250 / 320 nodes at Nmax 320, fin 8, pool_sizes [6], J 2, Jf 1: the feature section of the largest
          piece (320 x 8 words) exceeds one 2,048-word copy chunk of the gather launch
Schedules: the largest graph three times (fills every capacity exactly) followed by the three smallest (what the previous gather left
must be inert), anchor = positive, three entries that name one-cluster graphs only (a level with E = 0), the unassigned graph.
Models: 3 layers, hidden = embedding = 16 (small) / 32 (big), pred_hidden [50]; per configuration the variants "base", "nomask"
(mask = 0) and "nocon" (con_final = 0).  Margin 10 keeps the hinge active in every entry."""
import numpy as np
import torch

import eigen_two_stage_util as EU
import test_eigen_triplet_host as H

MARGIN = 10.0
SMALL_SIZES = [19, 13, 9, 10, 12, 11, 14, 17, 16, 15, 18, 9]
UNASSIGNED, ONE_CLUSTER = 1, (2, 3)
BIG_SIZES = [40, 130, 250, 320]
BIG_NMAX = 320
FIN = {"small": 6, "big": 8}
SCHEDULES = {
    "small": np.array([[0, 0, 0], [2, 11, 3], [0, 1, 5], [4, 4, 6], [2, 3, 2], [1, 6, 8], [7, 9, 10], [3, 2, 2], [10, 0, 1], [2, 2, 2]],
                      dtype=np.int64),
    "big": np.array([[3, 3, 3], [0, 0, 1], [1, 3, 0], [2, 1, 3], [0, 1, 2], [2, 2, 1]], dtype=np.int64),
}
VARIANTS = {"base": dict(mask=1, con_final=1), "nomask": dict(mask=0, con_final=1), "nocon": dict(mask=1, con_final=0)}
# (dataset, configuration, variant) of the step tests
CASES = [("small", name, var) for name in sorted(EU.CONFIGS) for var in sorted(VARIANTS)] + [("big", "big", "base")]
GATHER_CASES = [("small", name) for name in sorted(EU.CONFIGS)] + [("big", "big")]

_DATA, _REF = {}, {}


def shape(data, name):
    """(pool_sizes, J, Jf) of a configuration"""
    return ([6], 2, 1) if data == "big" else EU.CONFIGS[name]


def schedule(data):
    return SCHEDULES[data]


def dataset(data, name):
    """-> the graph objects of configuration ``name`` (built once per process; treat as read-only)"""
    key = (data, name)
    if key not in _DATA:
        pool_sizes, J, Jf = shape(data, name)
        rng = np.random.default_rng(7 + len(name) + sorted(EU.CONFIGS).index(name) if data == "small" else 5)
        sizes, nmax = (SMALL_SIZES, EU.NMAX) if data == "small" else (BIG_SIZES, BIG_NMAX)
        objs = []
        for b, n in enumerate(sizes):
            r = EU.make_result(rng, n, pool_sizes, unassigned=(data == "small" and b == UNASSIGNED),
                               one_cluster=(data == "small" and b in ONE_CLUSTER), odd=False)
            objs.append(EU.GraphObj(EU.make_dict(r, rng, nmax, J, Jf, FIN[data], label=b % 3)))
        _DATA[key] = objs
    return _DATA[key]


def cfg(data, name, var="base"):
    """the model configuration as tests/test_eigen_triplet_host.py's ``cfg`` lays it out"""
    pool_sizes, J, Jf = shape(data, name)
    h = 16 if data == "small" else 32
    return dict(VARIANTS[var], J=J, Jf=Jf, nmax=EU.NMAX if data == "small" else BIG_NMAX, num_layers=3, hidden=h, emb=h, label_dim=6,
                pred_hidden=[50], pool_sizes=list(pool_sizes), same_ap=0, margin=MARGIN)


def seeded_state(m, seed=11):
    """every parameter drawn from a CPU generator: the same numbers on any machine (tests/test_gpu_eigen_triplet.py's rule)"""
    g = torch.Generator().manual_seed(seed)
    return {k: torch.randn(v.shape, generator=g) * (1.0 / np.sqrt(max(v.shape)) if v.dim() > 1 else 0.1) for k, v in m.state_dict().items()}


def model(data, name, var="base", mode="train", dev="cuda", dropout=0.0):
    """the seeded encoder of a case: equal parameters at every call"""
    from two_stage_gnn_amd import eigen_encoders as EE
    c = cfg(data, name, var)
    m = EE.WavePoolingGcnEncoder(c["nmax"], FIN[data], c["hidden"], c["emb"], c["label_dim"], c["num_layers"], num_pool_matrix=c["J"],
                                 num_pool_final_matrix=c["Jf"], pool_sizes=c["pool_sizes"], pred_hidden_dims=c["pred_hidden"],
                                 mask=c["mask"], dropout=dropout, args=H.args_of(c))
    m.load_state_dict(seeded_state(m))
    return m.to(dev).train(mode == "train")


def grads(m):
    return {k: p.grad.detach().clone() for k, p in m.named_parameters() if p.grad is not None}


def ref_step(data, name, var, ids):
    """tests/test_eigen_triplet_host.py's ``ref_step`` (tests/eigen_ref.py three times at B = 1, torch's distances and margin loss,
    backward) on schedule entry ``ids`` from the seeded parameters, in float64 and in float32 on the CPU, computed once per (case,
    entry): {dtype: (dist_p, dist_n, [e_a, e_p, e_n], loss, {parameter: grad})}"""
    key = (data, name, var, tuple(int(i) for i in ids))
    if key not in _REF:
        c = cfg(data, name, var)
        sd = seeded_state(model(data, name, var, dev="cpu"))
        dicts = [dataset(data, name)[i].graph for i in key[3]]
        out = {}
        for dt in (torch.float64, torch.float32):
            p = {k: v.to(dt).clone().requires_grad_(True) for k, v in sd.items()}
            r = H.ref_step(p, dicts, c, dt, margin=MARGIN)
            out[dt] = r + ({k: (v.grad if v.grad is not None else torch.zeros_like(v)).detach() for k, v in p.items()},)
        _REF[key] = out
    return _REF[key]


def cancelling_scale(data, name, var, i):
    """{parameter: max |d <t, e(graph i)> / d parameter|} in float64, t the unit vector (1, .., 1) / sqrt(E): the size of ONE graph's
    part of a parameter gradient when positive and negative are the same graph.  Then dist_p = dist_n, the anchor's gradient is
    t - t = 0 and the other two parts are +t and -t through the same graph: every parameter gradient is exactly zero in exact
    arithmetic (and on the CPU, where the two parts are computed by identical calls and cancel bit for bit), so "1e-4 of the
    tensor's largest entry" allows nothing, while a batched fp32 evaluation sums the two parts row by row, in its own order, and keeps
    their rounding.  The rule is then applied to what is being summed: 1e-4 of the largest entry of one part (the reasoning of
    ``test_gpu_eigen_triplet._db2_floor``, whose tensor is exactly zero for the same reason)"""
    import eigen_ref as R
    key = ("scale", data, name, var, int(i))
    if key not in _REF:
        c = cfg(data, name, var)
        sd = seeded_state(model(data, name, var, dev="cpu"))
        p = {k: v.double().clone().requires_grad_(True) for k, v in sd.items()}
        x, adj, pooled, n0, nl, pm = H.dense_inputs(dataset(data, name)[int(i)].graph, c, torch.float64)
        e = R.wave_pooling_forward(H._ref_params(p), x, adj, pooled, n0, nl, pm, c["num_layers"], c["pool_sizes"], c["J"], c["Jf"], concat=True,
                                   mask=c["mask"], con_final=c["con_final"], n_linear=len(c["pred_hidden"]) + 1)
        (e.sum() / np.sqrt(e.numel())).backward()
        _REF[key] = {k: (float(v.grad.abs().max()) if v.grad is not None else 0.0) for k, v in p.items()}
    return _REF[key]


def pieces_of(objs, L, J, Jf):
    """[(piece buffer int32, n [L + 1], nnz [L + 1])] of graph objects, as ``eigen_two_stage_util.assemble_numpy`` reads them"""
    from two_stage_gnn_amd import eigen_triplet as ET
    out = []
    for o in objs:
        p = ET.pack_host(o.graph, L, J, Jf)
        buf, _ = ET.piece_buffer(p, ET.padded_rows_host(o.graph["feats"], p["n"][0]), J)
        out.append((buf, [int(v) for v in p["n"]], [int(c[1].size) for c in p["graphs"]]))
    return out


IPAT, FPAT = -7, np.float32(np.nan)          # what ``gather_numpy`` leaves in a word no store reaches


def gather_numpy(ar, ids):
    """csrc/eigen_stream.hip restated on the host arena: the records of ``ids`` -> every array at capacity under
    ``eigen_two_stage_util.assemble_numpy``'s names (``bptr_i`` has row_cap_{i+1} + 4 entries, ``rowptr_i`` row_cap_i + Nmax + 1, ``x``
    row_cap_0 + Nmax rows); a word the launch does not write holds IPAT / NaN.  Written from the header comment of the kernel file:
    pieces copied with their offsets, closing entries and padding filled"""
    from two_stage_gnn_amd import eigen_triplet as ET
    L, J, Jf, ldf, nmax = ar.L, ar.J, ar.Jf, ar.ldf, ar.nmax
    nlev = L + 1
    Rc, Ec = ar.caps
    rec = ar.records[np.asarray(ids)]
    n, z = rec[:, 2:2 + nlev].astype(np.int64), rec[:, 6:6 + nlev].astype(np.int64)
    row0 = np.concatenate([np.zeros((1, nlev), np.int64), np.cumsum(n, axis=0)])
    e0 = np.concatenate([np.zeros((1, nlev), np.int64), np.cumsum(z, axis=0)])
    R, E = row0[-1], e0[-1]
    out = {}
    for i in range(nlev):
        out["rowptr_%d" % i] = np.full(Rc[i] + nmax + 1, E[i], dtype=np.int32)
        out["col_%d" % i] = np.full(max(Ec[i], 1), IPAT, dtype=np.int32)
        out["val_%d" % i] = np.full(max(Ec[i], 1), FPAT, dtype=np.float32)
        out["graph_ptr_%d" % i] = row0[:, i].astype(np.int32)
        out["row_graph_%d" % i] = np.full(Rc[i], 2, dtype=np.int32)
        out["row_slot_%d" % i] = np.zeros(Rc[i], dtype=np.int32)
        out["slot_count_%d" % i] = np.array([(n[:, i] > s).sum() for s in range(nmax)], dtype=np.int32)
    for i in range(L):
        out["cluster_of_%d" % i] = np.full(Rc[i], -1, dtype=np.int32)
        out["coef_%d" % i] = np.zeros((Rc[i], J), dtype=np.float32)
        out["bptr_%d" % i] = np.full(Rc[i + 1] + 4, R[i], dtype=np.int32)
        out["members_%d" % i] = np.full(Rc[i], IPAT, dtype=np.int32)
    out["final"] = np.zeros((Rc[L], Jf), dtype=np.float32) if Jf else None
    out["x"] = np.zeros((Rc[0] + nmax, ldf), dtype=np.float32)
    for b in range(3):
        o = int(rec[b, 0])
        nb, zb = [int(v) for v in n[b]], [int(v) for v in z[b]]
        words = int(ET.piece_layout(nb, zb, J, Jf, ldf)[-1])
        u = ET.unpack_piece(ar.buf[o:o + words], nb, zb, J, Jf, ldf)
        for i, (rp, col, val) in enumerate(u["graphs"]):
            r0, c0 = row0[b, i], e0[b, i]
            out["rowptr_%d" % i][r0:r0 + nb[i]] = rp[:nb[i]] + c0
            out["col_%d" % i][c0:c0 + zb[i]] = col + r0
            out["val_%d" % i][c0:c0 + zb[i]] = val
            out["row_graph_%d" % i][r0:r0 + nb[i]] = b
            out["row_slot_%d" % i][r0:r0 + nb[i]] = np.arange(nb[i])
        for i, lv in enumerate(u["levels"]):
            r0, c0 = row0[b, i], row0[b, i + 1]
            c = lv["cluster_of"]
            out["cluster_of_%d" % i][r0:r0 + nb[i]] = np.where(c >= 0, c + c0, c)
            out["coef_%d" % i][r0:r0 + nb[i]] = lv["coef"]
            out["members_%d" % i][r0:r0 + nb[i]] = lv["members"] + r0
            out["bptr_%d" % i][c0 + b:c0 + b + nb[i + 1] + 1] = lv["bptr"][:nb[i + 1] + 1] + r0
        if Jf:
            out["final"][row0[b, L]:row0[b, L] + nb[L]] = u["final"]
        out["x"][row0[b, 0]:row0[b, 0] + nb[0]] = u["feats"]
    return out, [int(v) for v in R], [int(v) for v in E]
