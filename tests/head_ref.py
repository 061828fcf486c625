"""Reference of the graph-level head (csrc/head.hip): two chained linear maps on the concatenated readout, their backward with the
per-block squared norms of the gradients, mean softmax cross-entropy, the packed (value, row) max-readout words the head's forward
launches decode, and the max readout of a last uniform level.  TEST INFRASTRUCTURE: plain torch / numpy on the CPU, no project kernel;
float64 by default, ``dtype=torch.float32`` runs the SAME code in single precision (the yardstick of the kernels' rounding).

    vec = out W1^T + b1          W1 [E, P], W2 [C, E]  (nn.Linear.weight)
    y   = vec W2^T + b2
"""
import numpy as np
import torch


def _t(x, dtype):
    return None if x is None else x.to(dtype)


def _tree_sum(t):
    """sum over the last dimension in a fixed pairwise order: (t0 + t1) + (t2 + t3) per group of four, then halves folded onto each other"""
    n = t.size(-1)
    m = 4
    while m < n:
        m *= 2
    t = torch.cat([t, t.new_zeros(t.shape[:-1] + (m - n,))], dim=-1)
    t = (t[..., 0::4] + t[..., 1::4]) + (t[..., 2::4] + t[..., 3::4])
    while t.size(-1) > 1:
        h = t.size(-1) // 2
        t = t[..., :h] + t[..., h:]
    return t[..., 0]


def _rows_times(x, w, order):
    """x [B, K] times w [N, K] transposed -> [B, N]; order "tree": the K products of every output summed pairwise (_tree_sum) instead of in
    the library's order — in float64 the two agree to rounding, in float32 they are two samples of the rounding of one sum"""
    return x @ w.t() if order == "lib" else _tree_sum(x[:, None, :] * w[None, :, :])


def head_fwd(out, w1, b1, w2, b2, dtype=torch.float64, order="lib"):
    """-> vec [B, E], y [B, C]; b1 / b2 may be None"""
    out, w1, b1, w2, b2 = (_t(x, dtype) for x in (out, w1, b1, w2, b2))
    vec = _rows_times(out, w1, order)
    if b1 is not None:
        vec = vec + b1
    y = _rows_times(vec, w2, order)
    if b2 is not None:
        y = y + b2
    return vec, y


def head_bwd(out, vec, dy, dvec, w1, w2, has_b1=True, has_b2=True, dtype=torch.float64):
    """-> dout [B, P], dw1 [E, P], db1 [E] | None, dw2 [C, E], db2 [C] | None, normparts [ceil(E/4) + 1].
    dvec (a second cotangent, of vec itself) may be None.  normparts[jb], jb < ceil(E/4): the sum of squares of rows 4jb .. 4jb+3 of
    dw1 and of their db1 entries (has_b1); the last one: of dw2 and db2 (has_b2)."""
    out, vec, dy, dvec, w1, w2 = (_t(x, dtype) for x in (out, vec, dy, dvec, w1, w2))
    dvt = dy @ w2                                              # [B, E] gradient of vec
    if dvec is not None:
        dvt = dvec + dvt
    dout = dvt @ w1
    dw1, db1 = dvt.t() @ out, dvt.sum(0)
    dw2, db2 = dy.t() @ vec, dy.sum(0)
    E = w1.size(0)
    nj = (E + 3) // 4
    parts = torch.zeros(nj + 1, dtype=dtype)
    for jb in range(nj):
        parts[jb] = (dw1[4 * jb:4 * jb + 4] ** 2).sum() + ((db1[4 * jb:4 * jb + 4] ** 2).sum() if has_b1 else 0.0)
    parts[nj] = (dw2 ** 2).sum() + ((db2 ** 2).sum() if has_b2 else 0.0)
    return dout, dw1, (db1 if has_b1 else None), dw2, (db2 if has_b2 else None), parts


def softmax_ce(y, label, dtype=torch.float64):
    """-> loss (0-dim), dy [B, C]: mean over the rows of logsumexp(y_b) - y_b[label_b], and its gradient"""
    y = y.to(dtype)
    B = y.size(0)
    m = y.max(dim=1, keepdim=True)[0]
    logz = m + torch.log(torch.exp(y - m).sum(dim=1, keepdim=True))
    idx = label.long()[:, None]
    loss = (logz - y.gather(1, idx)).sum() / B
    onehot = torch.zeros_like(y).scatter_(1, idx, 1.0)
    return loss, (torch.exp(y - logz) - onehot) / B


# ----------------------------------------------------------------------------- packed (value, row) maxima (csrc/readout_body.h)
# word = f32_ordered(value) << 32 | (0xFFFFFFFF - row); f32_ordered maps the float order onto the unsigned order (negative: all bits
# flipped, else the sign bit set), so the LARGEST word is the largest value and, among equal values, the SMALLEST row.  0: no candidate.
_ROW_TOP = np.uint64(0xFFFFFFFF)


def _f32_ordered(val):
    u = np.ascontiguousarray(val, dtype=np.float32).view(np.uint32)
    return np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def _ordered_f32(o):
    o = np.ascontiguousarray(o, dtype=np.uint32)
    return np.where(o & np.uint32(0x80000000), o & np.uint32(0x7FFFFFFF), ~o).astype(np.uint32).view(np.float32)


def encode_packed(val, row):
    """np.uint64 words of (val float32, row int; row < 0: no candidate -> 0), elementwise"""
    row = np.asarray(row, dtype=np.int64)
    w = (_f32_ordered(val).astype(np.uint64) << np.uint64(32)) | (_ROW_TOP - row.clip(min=0).astype(np.uint64))
    return np.where(row >= 0, w, np.uint64(0))


def packed_max(x, L):
    """np.uint64 [B, F]: per (graph, column) the largest word over the candidates of slot_ref.Layout L — what the per-layer partial
    kernels accumulate with atomicMax on a zeroed buffer"""
    idx = L.idx.numpy()                                        # [B, nmax], -1: absent
    xv = x.float().numpy()
    F = xv.shape[1]
    w = encode_packed(xv[idx.clip(min=0)], np.broadcast_to(idx[:, :, None], idx.shape + (F,)))
    return w.max(axis=1) if idx.shape[1] else np.zeros((idx.shape[0], F), dtype=np.uint64)


def pack_layers(words):
    """the launches' buffer: layer l (np.uint64 [B, width_l]; every layer Fh wide but the last, Fl) at offset l * B * Fh -> int64 tensor"""
    return torch.from_numpy(np.concatenate([w.reshape(-1) for w in words]).view(np.int64).copy())


def decode_packed(packed, B, L, Fh, Fl):
    """-> out float32 [B, (L - 1) * Fh + Fl] (the concatenated readout), arg int32 [same layout as packed]; a word of 0: value 0, arg -1"""
    p = packed.numpy().view(np.uint64)
    val = _ordered_f32((p >> np.uint64(32)).astype(np.uint32))
    row = (_ROW_TOP - (p & _ROW_TOP)).astype(np.int64)
    val = np.where(p == 0, np.float32(0), val)
    arg = np.where(p == 0, -1, row).astype(np.int32)
    out = np.zeros((B, (L - 1) * Fh + Fl), dtype=np.float32)
    for l in range(L):
        w = Fh if l < L - 1 else Fl
        out[:, l * Fh:l * Fh + w] = val[l * B * Fh:l * B * Fh + B * w].reshape(B, w)
    return torch.from_numpy(out), torch.from_numpy(arg)


# ----------------------------------------------------------------------------- max readout of a uniform level (DiffPool's last one)
def ro_tail(z, B, N):
    """-> out [B, F] (z's dtype), arg int32 [B, F]: max over rows b * N .. b * N + N - 1 of z, the smallest row among equal values"""
    F = z.size(1)
    d = z[:B * N].reshape(B, N, F)
    out = d.max(dim=1)[0]
    n = torch.arange(N)[None, :, None].expand(B, N, F)
    first = torch.where(d == out[:, None, :], n, torch.full_like(n, N)).min(dim=1)[0]
    return out, (first + N * torch.arange(B)[:, None]).to(torch.int32)


def ro_tail_bwd(dseg, arg, B, N):
    """dz [B * N, F]: dseg[b, f] at row arg[b, f], 0 elsewhere (arg -1: the whole column of graph b is 0)"""
    F = dseg.size(1)
    rows = torch.arange(B * N)[:, None]
    a = arg.long().repeat_interleave(N, dim=0)                 # [B * N, F]
    return torch.where(a == rows, dseg.repeat_interleave(N, dim=0), torch.zeros(B * N, F, dtype=dseg.dtype))
