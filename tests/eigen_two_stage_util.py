"""What tests/test_eigen_two_stage_host.py and tests/test_gpu_eigen_two_stage.py share: small hand-built EigenGCN graph sets (as
``eigen_pool.coarsen`` results and as the ``.graph`` dicts the reference's sampler fills) and a numpy restatement of the chunk
assembler (csrc/eigen_assemble.hip) on host piece buffers.

The coarsening is built by hand, not by ``eigen_pool.coarsen``: chunk labels, random coefficients, the pooled adjacency
Omega^T A Omega without its diagonal.  That reaches the cases ``coarsen`` rejects or never produces — a pooled graph of ONE node (no
edges), rows whose J coefficients are all zero (unassigned: ``cluster_of`` = -1) — while ``eigen_pool.collate`` and
``eigen_pool.dense_inputs`` read such a result like any other."""
import numpy as np

NMAX = 19
CONFIGS = {                      # name: (pool_sizes, J, Jf)
    "l1_j1": ([4], 1, 0),
    "l1_j2_f1": ([4], 2, 1),
    "l2_j1": ([3, 2], 1, 0),
    "l1_j2_f2": ([3], 2, 2),
}
DEEP = {"l4_j1_f1": ([2, 2, 2, 2], 1, 1)}      # more pooling levels than the assembler takes: pieces and the per-graph route only


def config(name):
    return CONFIGS[name] if name in CONFIGS else DEEP[name]


# 33 graphs: the first is full (n = Nmax), the second has unassigned rows, the third pools to ONE node; the sizes that follow make the
# destination offsets of rowptr / col / members / bptr take every residue mod 4 (asserted in the tests)
SIZES = [19, 13, 9, 9, 10, 12, 11, 14, 17, 16, 15, 18, 9, 13, 11, 10, 12, 19, 14, 9, 17, 15, 16, 11, 13, 18, 10, 12, 9, 14, 19, 17, 15]
UNASSIGNED, ONE_CLUSTER = 1, 2
ODD = (0, 1, 3, 6, 11, 20)                       # graphs with one directed edge: an odd number of entries


class GraphObj:
    def __init__(self, d):
        self.graph = d


def rand_adj(rng, n, extra=1.3):
    A = np.zeros((n, n))
    i = np.arange(n)
    if n > 1:
        A[i, (i + 1) % n] = 1
    a, b = rng.integers(0, n, int(extra * n)), rng.integers(0, n, int(extra * n))
    A[a[a != b], b[a != b]] = 1
    return np.maximum(A, A.T)


def make_result(rng, n, pool_sizes, unassigned=False, one_cluster=False, odd=False):
    """a hand-built ``eigen_pool.coarsen`` result: ``graphs`` [A_0 .. A_L], ``labels``, ``coef`` [n_i, 5], ``final`` [n_L, 4].
    ``odd``: one directed edge on top of the symmetric ones, so the graph has an odd number of entries (symmetric graphs alone
    would put every piece's ``col`` at an even offset)"""
    A = rand_adj(rng, n)
    if odd:
        a, b = np.nonzero((A == 0) & ~np.eye(n, dtype=bool))
        A[a[0], b[0]] = 1.0
    graphs, labels, coefs = [A], [], []
    for level, ps in enumerate(pool_sizes):
        m = A.shape[0]
        k = 1 if one_cluster else max(1, m // ps)
        lab = np.arange(m) * k // m
        coef = rng.standard_normal((m, 5))
        if unassigned and level == 0:
            coef[[0, m // 2, m - 1]] = 0.0                   # rows that add nothing: bucket 0 of the graph
        Om = np.zeros((m, k))
        Om[np.arange(m), lab] = 1.0
        A = Om.T @ A @ Om
        np.fill_diagonal(A, 0.0)
        graphs.append(A)
        labels.append(lab.astype(np.int64))
        coefs.append(coef)
    return {"graphs": graphs, "labels": labels, "coef": coefs, "final": rng.standard_normal((A.shape[0], 4))}


def make_dict(r, rng, nmax, J, Jf, fin, label=0):
    """the ``.graph`` dict graph_sampler.py:130-176 fills for one result (through ``eigen_pool.dense_inputs`` at B = 1)"""
    from two_stage_gnn_amd import eigen_pool as ep
    L = len(r["labels"])
    adj, pooled, n0, nl, pm = ep.dense_inputs([r], nmax, J, Jf)
    n = int(n0[0])
    feats = np.zeros((nmax, fin), dtype=np.float32)
    feats[:n] = rng.standard_normal((n, fin)).astype(np.float32)
    d = {"adj": adj[0].numpy(), "feats": feats, "num_nodes": n, "label": int(label), "assign_feats": feats.copy()}
    for i in range(L):
        d["adj_pool_%d" % (i + 1)] = pooled[i][0].numpy()
        d["num_nodes_%d" % (i + 1)] = int(nl[i][0])
        for j in range(J):
            d["pool_adj_%d_%d" % (i, j)] = pm[i][j][0].numpy()
    for j in range(Jf):
        d["pool_adj_%d_%d" % (L, j)] = pm[L][j][0].numpy()
    return d


_sets = {}


def graph_set(name, fin=6, sizes=SIZES, nmax=NMAX, classes=3):
    """(results, dicts) of configuration ``name``: built once, shared, never written"""
    key = (name, fin, tuple(sizes), nmax, classes)
    if key not in _sets:
        pool_sizes, J, Jf = config(name)
        rng = np.random.default_rng((sorted(CONFIGS) + sorted(DEEP)).index(name) + 41)
        results = [make_result(rng, n, pool_sizes, unassigned=(b == UNASSIGNED), one_cluster=(b == ONE_CLUSTER), odd=(b in ODD)) for b, n in enumerate(sizes)]
        _sets[key] = (results, [make_dict(r, rng, nmax, J, Jf, fin, label=b % classes) for b, r in enumerate(results)])
    return _sets[key]


def level_sizes(results):
    """int64 [B, L + 1]: rows of every level graph"""
    return np.array([[g.shape[0] for g in r["graphs"]] for r in results], dtype=np.int64)


def destination_residues(n, nnz):
    """the residues mod 4 of where the pieces' rowptr / col / members / bptr land in the chunk's arrays, over all levels"""
    B, nlev = n.shape
    row0 = np.concatenate([np.zeros((1, nlev), np.int64), np.cumsum(n, axis=0)])[:B]
    e0 = np.concatenate([np.zeros((1, nlev), np.int64), np.cumsum(nnz, axis=0)])[:B]
    res = {"rowptr": set((row0 % 4).reshape(-1)), "col": set((e0[nnz > 0] % 4).reshape(-1))}
    if nlev > 1:
        res["members"] = set((row0[:, :-1] % 4).reshape(-1))
        res["bptr"] = set(((row0[:, 1:] + np.arange(B)[:, None]) % 4).reshape(-1))
    return res


def assemble_numpy(pieces, nmax, J, Jf, ldf):
    """csrc/eigen_assemble.hip restated: ``pieces`` = [(buffer int32, n [L + 1], nnz [L + 1])] -> the chunk's arrays, a dict:
    per level graph i ``rowptr_i`` [R_i + Nmax + 1], ``col_i``, ``val_i``, ``graph_ptr_i``, ``row_graph_i``, ``row_slot_i``,
    ``slot_count_i``; per pooling level ``cluster_of_i``, ``coef_i``, ``bptr_i``, ``members_i``; ``final``; ``x`` [R_0 + Nmax, ldf]"""
    from two_stage_gnn_amd import eigen_triplet as ET
    B, nlev = len(pieces), len(pieces[0][1])
    L = nlev - 1
    n = np.array([p[1] for p in pieces], dtype=np.int64).reshape(B, nlev)
    z = np.array([p[2] for p in pieces], dtype=np.int64).reshape(B, nlev)
    row0 = np.concatenate([np.zeros((1, nlev), np.int64), np.cumsum(n, axis=0)])
    e0 = np.concatenate([np.zeros((1, nlev), np.int64), np.cumsum(z, axis=0)])
    R, E = row0[-1], e0[-1]
    out = {}
    for i in range(nlev):
        out["rowptr_%d" % i] = np.full(R[i] + nmax + 1, E[i], dtype=np.int32)        # (the closing entries: the last piece's fill)
        out["col_%d" % i] = np.zeros(max(E[i], 1), dtype=np.int32)
        out["val_%d" % i] = np.zeros(max(E[i], 1), dtype=np.float32)
        out["graph_ptr_%d" % i] = row0[:, i].astype(np.int32)
        out["row_graph_%d" % i] = np.zeros(R[i], dtype=np.int32)
        out["row_slot_%d" % i] = np.zeros(R[i], dtype=np.int32)
        out["slot_count_%d" % i] = np.array([(n[:, i] > s).sum() for s in range(nmax)], dtype=np.int32)
    for i in range(L):
        out["cluster_of_%d" % i] = np.zeros(R[i], dtype=np.int32)
        out["coef_%d" % i] = np.zeros((R[i], J), dtype=np.float32)
        out["bptr_%d" % i] = np.zeros(R[i + 1] + B + 1, dtype=np.int32)
        out["members_%d" % i] = np.zeros(R[i], dtype=np.int32)
    out["final"] = np.zeros((R[L], Jf), dtype=np.float32) if Jf else None
    out["x"] = np.zeros((R[0] + nmax, ldf), dtype=np.float32)
    for b, (buf, nb, zb) in enumerate(pieces):
        u = ET.unpack_piece(buf, [int(v) for v in nb], [int(v) for v in zb], J, Jf, ldf)
        last = b == B - 1
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
            k1 = nb[i + 1] + 1 + int(last)                                        # k + 1 buckets per graph; the last piece closes
            out["bptr_%d" % i][c0 + b:c0 + b + k1] = lv["bptr"][:k1] + r0
        if Jf:
            out["final"][row0[b, L]:row0[b, L] + nb[L]] = u["final"]
        out["x"][row0[b, 0]:row0[b, 0] + nb[0]] = u["feats"]
    return out


def batch_arrays(eb, x=None):
    """the arrays of an ``EigenBatch`` (tensors, host or device) under ``assemble_numpy``'s names, trimmed to their defined lengths"""
    out = {}
    gs = [eb.g0] + [lv.g for lv in eb.levels]
    for i, g in enumerate(gs):
        out["rowptr_%d" % i] = g.rowptr
        out["col_%d" % i] = g.col[:max(g.nnz, 1)]
        out["val_%d" % i] = g.val[:max(g.nnz, 1)]
        out["graph_ptr_%d" % i], out["slot_count_%d" % i] = g.graph_ptr, g.slot_count
        out["row_graph_%d" % i], out["row_slot_%d" % i] = g.row_graph[:g.n_rows], g.row_slot[:g.n_rows]
    for i, lv in enumerate(eb.levels):
        R = gs[i].n_rows
        out["cluster_of_%d" % i], out["coef_%d" % i] = lv.cluster_of[:R], lv.coef[:R]
        out["bptr_%d" % i], out["members_%d" % i] = lv.bptr, lv.members[:R]
    out["final"] = None if eb.final_coef is None else eb.final_coef[:gs[-1].n_rows]
    if x is not None:
        out["x"] = x
    return out
