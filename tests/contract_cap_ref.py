"""Reference of the capacity-batch contraction kernels (csrc/contract_cap.hip): a numpy / torch restatement, in the dtype of its
inputs (float64: the reference; float32 on the CPU: the yardstick of tests/fp32_yardstick.py), of

    rowsum     AS[i] = sum_{j in N(i)} S[j] over the neighbour table and its tail, zeros on rows >= n_tot
    forward    X'[b] = S_b^T Z_b, A'[b] = S_b^T (AS)_b, the folded max readout of Z (its ghost row is row_cap + size: a zero row)
    backward   dZ_b = S_b dX'_b (+ the readout's gradient where arg names a real row), dS_b = Z_b dX'_b^T + (AS)_b (dA'_b + dA'_b^T),
               zeros on rows >= n_tot

on a capacity layout: rows [0, n_tot) real (graph b: [graph_ptr[b], graph_ptr[b + 1])), [n_tot, row_cap) padding, [row_cap,
row_cap + nmax) ghost slots.  TEST INFRASTRUCTURE: no project kernel, nothing shared with the code under test."""
import numpy as np
import torch


def layout(sizes, row_cap):
    """graph_ptr int32 [B + 2] as the gather launch writes it: prefix sums, then row_cap (the dummy graph of the padding rows)"""
    gp = np.zeros(len(sizes) + 2, dtype=np.int32)
    gp[1:len(sizes) + 1] = np.cumsum(sizes)
    gp[-1] = row_cap
    assert gp[len(sizes)] <= row_cap
    return gp


def neighbours(adjs, sizes, row_cap, nmax, ell_w):
    """dense adjacencies (adj[:n, :n] of each graph) -> (ell int32 [R, ell_w] with -1 in empty entries, tail_ptr int32 [R + 1],
    tail_col int32 [>= 4], the tail's length) in batch row ids, R = row_cap + nmax: the first ell_w neighbours of a row in the table, the rest in the tail"""
    R = row_cap + nmax
    ell = np.full((R, ell_w), -1, dtype=np.int32)
    tail_ptr = np.zeros(R + 1, dtype=np.int32)
    tail = []
    r = 0
    for a, n in zip(adjs, sizes):
        g0 = r
        for v in range(n):
            nb = [g0 + int(j) for j in np.nonzero(np.asarray(a)[v, :n])[0]]
            ell[r, :min(len(nb), ell_w)] = nb[:ell_w]
            tail_ptr[r] = len(tail)
            tail += nb[ell_w:]
            r += 1
    tail_ptr[r:] = len(tail)
    return ell, tail_ptr, np.asarray(tail + [0] * max(1, 4 - len(tail)), dtype=np.int32), len(tail)


def rowsum(ell, tail_ptr, tail_col, n_tot, S):
    out = torch.zeros_like(S)
    for r in range(n_tot):
        acc = torch.zeros(S.size(1), dtype=S.dtype)
        for j in ell[r]:
            if j >= 0:
                acc = acc + S[int(j)]
        for e in range(int(tail_ptr[r]), int(tail_ptr[r + 1])):
            acc = acc + S[int(tail_col[e])]
        out[r] = acc
    return out


def forward(S, Z, AS, gp, B, row_cap, nmax):
    """-> xo [B, K, F], ao [B, K, K], ro [B, F], arg int32 [B, F] (ties go to the smallest row; the ghost row takes part when size < nmax)"""
    K, F = S.size(1), Z.size(1)
    xo, ao = torch.zeros(B, K, F, dtype=S.dtype), torch.zeros(B, K, K, dtype=S.dtype)
    ro, arg = torch.zeros(B, F, dtype=S.dtype), torch.full((B, F), -1, dtype=torch.int32)
    for b in range(B):
        r0, r1 = int(gp[b]), int(gp[b + 1])
        xo[b] = S[r0:r1].t() @ Z[r0:r1]
        ao[b] = S[r0:r1].t() @ AS[r0:r1]
        rows = list(range(r0, r1))
        cand = Z[r0:r1]
        if r1 - r0 < nmax:
            rows.append(row_cap + (r1 - r0))
            cand = torch.cat([cand, torch.zeros(1, F, dtype=S.dtype)])
        if rows:
            val, idx = cand.max(dim=0)
            first = (cand == val[None]).to(torch.int64).argmax(dim=0)         # the smallest row among equals
            ro[b], arg[b] = val, torch.tensor(rows, dtype=torch.int32)[first]
    return xo, ao, ro, arg


def backward(S, Z, AS, dxo, dao, gp, B, dro=None, arg=None):
    """-> dZ [R, F], dS [R, K]; rows outside every graph stay zero; a readout winner outside its graph's real rows is dropped"""
    dZ, dS = torch.zeros_like(Z), torch.zeros_like(S)
    for b in range(B):
        r0, r1 = int(gp[b]), int(gp[b + 1])
        dZ[r0:r1] = S[r0:r1] @ dxo[b]
        dS[r0:r1] = Z[r0:r1] @ dxo[b].t() + AS[r0:r1] @ (dao[b] + dao[b].t())
        if dro is not None:
            for c in range(Z.size(1)):
                w = int(arg[b, c])
                if r0 <= w < r1:
                    dZ[w, c] = dZ[w, c] + dro[b, c]
    return dZ, dS


def slab_count(sizes):
    return int(sum((int(n) + 31) // 32 for n in sizes))
