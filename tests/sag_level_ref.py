"""Plain torch restatement of ONE SAGPool level tail with the GCN scorer (csrc/sagpool.hip; Code/sag/layers.py:14-25 and
network.py:33-44): score layer, top-k, gated gather, max || mean readout, filter_adj on a CSR, the next level's propagate, and the
backward of all of it written out by hand.  TEST INFRASTRUCTURE: no project kernel.

Every function takes a `dtype`: float64 is the reference, float32 on the CPU the yardstick of tests/fp32_yardstick.py.  The kernels'
discrete choices (perm, arg) are INPUTS wherever a value depends on them.

A graph is a CSR triple (rowptr, rowend, col) of int64 CPU tensors: row i = the sources j of the edges j -> i, entries
[rowptr[i], rowend[i]) of col (rowend = rowptr[1:] for a compact CSR; a pooled level's rows lie at their graph's old base with gaps
between them, so only rowptr[i] / rowend[i] of row i are ever read)."""
import numpy as np
import torch


def csr_of(ei, n):
    """edge_index [2, E] (source, target) -> compact CSR over the targets, the entries of a row in edge order"""
    order = torch.sort(ei[1], stable=True).indices
    rowptr = torch.zeros(n + 1, dtype=torch.int64)
    rowptr[1:] = torch.cumsum(torch.bincount(ei[1], minlength=n), 0)
    return rowptr, rowptr[1:].clone(), ei[0][order].clone()


def entries(csr, n):
    """(row of every entry, its source), rows ascending, entries in row order"""
    rowptr, rowend, col = csr
    lens = rowend[:n] - rowptr[:n]
    rows = torch.repeat_interleave(torch.arange(n), lens)
    first = torch.cumsum(lens, 0) - lens
    pos = rowptr[:n][rows] + (torch.arange(int(lens.sum())) - first[rows])
    return rows, col[pos]


def edges_of(csr, n):
    """the CSR as an edge_index (source, target), for oracle/pyg_ref.py"""
    rows, src = entries(csr, n)
    return torch.stack([src, rows])


def coef(csr, n, dtype):
    """gcn_norm with unit weights: d_i = #entries of row i (+ 1 unless the row holds i itself: add_remaining_self_loops; an existing self
    loop keeps weight 1), dinv = d^-1/2, self_w = dinv^2 (0 where the row already holds the loop)"""
    rows, src = entries(csr, n)
    has_self = torch.zeros(n, dtype=torch.bool)
    has_self[rows[rows == src]] = True
    d = torch.bincount(rows, minlength=n).to(dtype) + (~has_self).to(dtype)
    dinv = torch.ones(n, dtype=dtype) / torch.sqrt(d)
    return dinv, torch.where(has_self, torch.zeros(n, dtype=dtype), dinv * dinv)


def coef_f32(csr, n):
    """the float32 coefficients to the bit: dinv = 1.0f / sqrtf(d) with both operations correctly rounded, self_w = dinv * dinv rounded
    once.  Formed in float64 and rounded to float32 after each operation (innocuous for sqrt, division and a product at 53 >= 2 x 24 + 2
    bits), so the answer does not depend on how this machine's float32 vector code rounds"""
    rows, src = entries(csr, n)
    has_self = np.zeros(n, dtype=bool)
    has_self[rows[rows == src].numpy()] = True
    d = np.bincount(rows.numpy(), minlength=n).astype(np.float64) + (~has_self)
    root = np.sqrt(d).astype(np.float32)
    dinv = (1.0 / root.astype(np.float64)).astype(np.float32)
    self_w = np.where(has_self, np.float32(0), (dinv.astype(np.float64) * dinv.astype(np.float64)).astype(np.float32))
    return torch.from_numpy(dinv), torch.from_numpy(self_w.astype(np.float32))


def propagate(csr, dinv, self_w, x):
    """(A^ x)_i = dinv_i sum_{j in row i} dinv_j x_j + self_w_i x_i ; x [n] or [n, F]"""
    n = x.size(0)
    rows, src = entries(csr, n)
    u = (lambda v: v.unsqueeze(1)) if x.dim() == 2 else (lambda v: v)
    acc = torch.zeros_like(x).index_add(0, rows, u(dinv[src]) * x[src])
    return u(dinv) * acc + u(self_w) * x


def score(y, csr, w_s, b_s, dtype):
    """A^ (relu(y) w_s) + b_s   (layers.py:18: GCNConv(C -> 1) on the level's input relu(y))"""
    n = y.size(0)
    dinv, self_w = coef(csr, n, dtype)
    t = torch.relu(y.to(dtype)) @ w_s.to(dtype)
    return propagate(csr, dinv, self_w, t) + b_s.to(dtype).view(())


def pooled_gp(gp, ratio):
    """k_b = ceil(ratio n_b) in float32, as PyG's topk computes it -> graph pointer of the pooled level"""
    sizes = np.diff(np.asarray(gp)).astype(np.int64)
    k = np.minimum(np.ceil(np.float32(ratio) * sizes.astype(np.float32)).astype(np.int64), sizes)
    return np.concatenate([[0], np.cumsum(k)]).astype(np.int64)


def topk_from(sc, gp, gp_new):
    """-> perm [K] (old rows, descending score inside a graph, ties towards the smaller node), new_id [n] (position in perm, -1: dropped)"""
    gp, gp_new = np.asarray(gp), np.asarray(gp_new)
    n, B = int(gp[-1]), len(gp) - 1
    s = sc.detach().double().numpy()
    graph = np.repeat(np.arange(B), np.diff(gp))
    order = np.lexsort((np.arange(n), -s, graph))
    perm = np.concatenate([order[gp[b]: gp[b] + (gp_new[b + 1] - gp_new[b])] for b in range(B)]) if B else order[:0]
    new_id = np.full(n, -1, dtype=np.int64)
    new_id[perm] = np.arange(perm.size)
    return torch.from_numpy(perm.astype(np.int64)), torch.from_numpy(new_id)


def gather(y, sc, perm, dtype, relu_in=True):
    """relu(y)[perm] * tanh(score[perm])   (layers.py:21)"""
    v = y.to(dtype)
    v = torch.relu(v) if relu_in else v
    return v[perm] * torch.tanh(sc.to(dtype)[perm]).unsqueeze(1)


def readout(xp, gp_new):
    """-> out [B, 2F] = max || mean over each graph's rows, arg [B, F] = the FIRST row attaining the max (-0.0 == 0.0)"""
    gp_new = np.asarray(gp_new)
    B, F = len(gp_new) - 1, xp.size(1)
    out = torch.zeros(B, 2 * F, dtype=xp.dtype)
    arg = torch.zeros(B, F, dtype=torch.int64)
    for b in range(B):
        rows = xp[gp_new[b]: gp_new[b + 1]]
        mx = rows.max(0).values
        out[b, :F], out[b, F:] = mx, rows.mean(0)
        arg[b] = (rows == mx.unsqueeze(0)).int().argmax(0) + int(gp_new[b])
    return out, arg


def filtered_csr(csr, n, perm, new_id, dtype):
    """filter_adj on the CSR (layers.py:23-24): new row p = the kept neighbours of old row perm[p], relabelled, in their original order.
    -> compact CSR of the pooled level, cnt [K], and that level's (dinv, self_w)"""
    rowptr, rowend, col = csr
    K = perm.numel()
    sub = (rowptr[:n][perm], rowend[:n][perm], col)
    rows, src = entries(sub, K)
    ids = new_id[src]
    keep = ids >= 0
    cnt = torch.bincount(rows[keep], minlength=K)
    rp = torch.zeros(K + 1, dtype=torch.int64)
    rp[1:] = torch.cumsum(cnt, 0)
    out = (rp, rp[1:].clone(), ids[keep].clone())
    dinv, self_w = coef(out, K, dtype)
    return out, cnt, dinv, self_w


def backward(y, csr, w_s, sc, perm, new_id, arg, gp, gp_new, dread, dtype, dxp=None, dagg_next=None, csr_next=None, relu_in=True):
    """the level tail's backward by hand (the formulas in the comments of sag_pool_bwd, sag_du_kernel and sag_pool_graph_bwd_kernel).
    dxp [K, F]: gradient arriving at the pooled rows, or None (the last level), or formed here as A^' dagg_next from the NEXT level's
    CSR (symmetric, so its transpose is itself).  For a kept row r = perm[p] of graph b, gate = tanh(score_r):
        dtot_p = dxp_p + dread[b, F:] / k_b + [arg[b, :] == p] dread[b, :F]
        dyb_r = dtot_p gate,   dscore_r = (1 - gate^2) <dtot_p, relu(y_r)>          (0 on dropped rows)
        dt = A^ dscore,   du_r = (dyb_r + dt_r w_s) [y_r > 0]
        part[b] = [sum_{r in b} dt_r relu(y_r) | sum_{r in b} dscore_r],  dw_s = sum_b part[b, :F],  db_s = sum_b part[b, F]"""
    gp, gp_new = np.asarray(gp), np.asarray(gp_new)
    n, F, B, K = y.size(0), y.size(1), len(gp) - 1, perm.numel()
    y, w_s, sc, dread = y.to(dtype), w_s.to(dtype), sc.to(dtype), dread.to(dtype)
    v = torch.relu(y) if relu_in else y
    if dagg_next is not None:
        dn, sn = coef(csr_next, K, dtype)
        dxp = propagate(csr_next, dn, sn, dagg_next.to(dtype))
    dxp = torch.zeros(K, F, dtype=dtype) if dxp is None else dxp.to(dtype)
    kb = torch.from_numpy(np.diff(gp_new))
    gnew = torch.repeat_interleave(torch.arange(B), kb)
    p = torch.arange(K)
    dtot = dxp + dread[gnew, F:] / kb.to(dtype)[gnew].unsqueeze(1) + torch.where(arg[gnew] == p.unsqueeze(1), dread[gnew, :F],
                                                                                 torch.zeros((), dtype=dtype))
    gate = torch.tanh(sc[perm])
    dyb = torch.zeros(n, F, dtype=dtype)
    dyb[perm] = dtot * gate.unsqueeze(1)
    dscore = torch.zeros(n, dtype=dtype)
    dscore[perm] = (1 - gate * gate) * (dtot * v[perm]).sum(1)
    dinv, self_w = coef(csr, n, dtype)
    dt = propagate(csr, dinv, self_w, dscore)
    du = torch.where(y > 0, dyb + dt.unsqueeze(1) * w_s.unsqueeze(0), torch.zeros((), dtype=dtype))
    gold = torch.repeat_interleave(torch.arange(B), torch.from_numpy(np.diff(gp)))
    part = torch.zeros(B, F + 1, dtype=dtype)
    part[:, :F].index_add_(0, gold, dt.unsqueeze(1) * torch.relu(y))
    part[:, F].index_add_(0, gold, dscore)
    return {"dxp": dxp, "dtot": dtot, "dyb": dyb, "dscore": dscore, "dt": dt, "du": du, "part": part, "dws": part[:, :F].sum(0),
            "dbs": part[:, F].sum().view(1)}


def level(y, csr, gp, ratio, w_s, b_s, dtype, perm=None):
    """the whole forward of one level; perm given: the kernel's (the scores' order is then not consulted).  -> dict"""
    n = y.size(0)
    gp_new = pooled_gp(gp, ratio)
    sc = score(y, csr, w_s, b_s, dtype)
    if perm is None:
        perm, new_id = topk_from(sc, gp, gp_new)
    else:
        new_id = torch.full((n,), -1, dtype=torch.int64)
        new_id[perm] = torch.arange(perm.numel())
    xp = gather(y, sc, perm, dtype)
    out, arg = readout(xp, gp_new)
    csr_n, cnt, dinv_n, self_w_n = filtered_csr(csr, n, perm, new_id, dtype)
    return {"score": sc, "perm": perm, "new_id": new_id, "gp_new": gp_new, "xp": xp, "out": out, "arg": arg, "csr_next": csr_n,
            "cnt": cnt, "dinv_next": dinv_n, "self_w_next": self_w_n, "agg_next": propagate(csr_n, dinv_n, self_w_n, xp)}
