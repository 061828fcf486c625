"""Restatements of the GEMM and weight-gradient building blocks (csrc/gemm.hip, csrc/tn_rows_body.h) in plain torch on the CPU, each
parametrised by dtype.  TEST INFRASTRUCTURE: no project kernel.

float64 is the reference.  The float32 run of the SAME code is the yardstick of tests/fp32_yardstick.py, and it sums the way the kernels
do: every reduction over rows or over k is a chain in index order (a loop of rank-1 updates, a running row sum), because the kernels are
k-ordered fp32 fma chains (v_mfma_f32_32x32x2_f32) closed by fixed-order slab sums.  One BLAS call would sum in blocks: a tighter
yardstick for a reason that has nothing to do with correctness.  In float64 a single product is used."""
import torch


def _tn(a, b, dtype):
    """a [R, K], b [R, N] -> a^T b [K, N]; float32: the rows are added in index order"""
    a, b = a.to(dtype), b.to(dtype)
    if dtype == torch.float64:
        return a.t() @ b
    acc = torch.zeros(a.size(1), b.size(1), dtype=dtype)
    for r in range(a.size(0)):
        acc += a[r][:, None] * b[r][None, :]
    return acc


def _rowsum(x, dtype):
    """x [R, F] -> [F]; float32: a running sum in row order"""
    x = x.to(dtype)
    if dtype == torch.float64:
        return x.sum(0)
    acc = torch.zeros(x.size(1), dtype=dtype)
    for r in range(x.size(0)):
        acc += x[r]
    return acc


def gemm_ref(A, sam, sak, B, sbk, sbn, C, scm, scn, M, N, K, batch=1, stride_a=0, stride_b=0, stride_c=0, seg_ptr=None, ragged=0,
             max_seg=0, alpha=1.0, accumulate=0, dtype=torch.float64):
    """tsgnn_gemm_f32 with its own arguments: A, B, C are FLAT CPU tensors that begin where the pointers point (C: the contents before
    the call), strides in elements.  C[z] (+)= alpha * op(A[z]) . op(B[z]) with element (m, k) of op(A) at A[m * sam + k * sak].
    seg_ptr with ragged = 1: batch z takes k in [seg_ptr[z], seg_ptr[z + 1]) of both operands (K is ignored); ragged = 2: A and C shift
    along m by seg_ptr[z] and M is the segment's length (M is ignored).  -> the whole C buffer after the call in `dtype`: elements
    the call does not own come back as they were."""
    if (seg_ptr is None) != (ragged == 0) or ragged not in (0, 1, 2):
        raise ValueError("seg_ptr goes with ragged = 1 or 2")
    A, B, out = A.to(dtype).contiguous().view(-1), B.to(dtype).contiguous().view(-1), C.to(dtype).contiguous().view(-1).clone()
    if N == 0 or (ragged == 2 and max_seg <= 0) or (ragged != 2 and M == 0):
        return out
    alpha = torch.tensor(alpha, dtype=torch.float32).to(dtype)          # (the kernel's alpha is a float)
    for z in range(batch):
        a0, b0, c0, m, k = z * stride_a, z * stride_b, z * stride_c, M, K
        if ragged == 1:
            s0, k = int(seg_ptr[z]), int(seg_ptr[z + 1]) - int(seg_ptr[z])
            a0, b0 = a0 + s0 * sak, b0 + s0 * sbk
        elif ragged == 2:
            s0, m = int(seg_ptr[z]), int(seg_ptr[z + 1]) - int(seg_ptr[z])
            a0, c0 = a0 + s0 * sam, c0 + s0 * scm
        if m <= 0:
            continue
        at = torch.as_strided(A, (k, m), (sak, sam), a0)                # op(A)^T: rows = k
        b = torch.as_strided(B, (k, N), (sbk, sbn), b0)
        c = torch.as_strided(out, (m, N), (scm, scn), c0)
        p = alpha * _tn(at, b, dtype)
        c.copy_(c + p if accumulate else p)
    return out


def _slab_ref(z, du, rows, K_in, nslab, rps, bo, dtype):
    """-> [nslab, K_in + 1, N]: slab s = z[slab rows, :K_in]^T du[slab rows], row K_in = the column sums of du over the slab's rows and
    its share of the `bo` bias-only rows behind `rows` (tsgnn_linear_wgrad_f32 with dw = NULL)"""
    N = du.size(1)
    out = torch.zeros(nslab, K_in + 1, N, dtype=dtype)
    per = -(-bo // nslab) if bo else 0
    for s in range(nslab):
        r0, r1 = min(rows, s * rps), min(rows, (s + 1) * rps)
        out[s, :K_in] = _tn(z[r0:r1, :K_in], du[r0:r1], dtype)
        out[s, K_in] = _rowsum(du[r0:r1], dtype)
        if bo:
            e0 = rows + s * per
            out[s, K_in] += _rowsum(du[e0:max(e0, min(rows + bo, e0 + per))], dtype)
    return out


def tn_ref(z, du, rows, K_in, bias_only_rows, dtype):
    """-> (dw [K_in, N], db [N]): dw = z[:rows, :K_in]^T du[:rows], db = the column sums of du[:rows + bias_only_rows]"""
    return _tn(z[:rows, :K_in], du[:rows], dtype), _rowsum(du[:rows + bias_only_rows], dtype)


def ragged_slab_ref(s, x, slab_row_ptr, dtype):
    """-> [nslab, K + 1, N]: slab t = s[rows_t]^T x[rows_t] with rows_t = [slab_row_ptr[t], slab_row_ptr[t + 1]), row K = the column
    sums of x over them (the workspace tsgnn_ragged_tn_f32 leaves)"""
    nslab, K, N = len(slab_row_ptr) - 1, s.size(1), x.size(1)
    out = torch.zeros(nslab, K + 1, N, dtype=dtype)
    for t in range(nslab):
        r0, r1 = int(slab_row_ptr[t]), int(slab_row_ptr[t + 1])
        out[t, :K], out[t, K] = _tn(s[r0:r1], x[r0:r1], dtype), _rowsum(x[r0:r1], dtype)
    return out


def ragged_tn_ref(s, x, slab_row_ptr, seg_slab_ptr, dtype):
    """-> [nseg, K, N]: out[g] = sum over the slabs [seg_slab_ptr[g], seg_slab_ptr[g + 1]) of s[rows]^T x[rows] (slabs in order);
    a segment without slabs is zeros"""
    slabs = ragged_slab_ref(s, x, slab_row_ptr, dtype)
    K = s.size(1)
    out = torch.zeros(len(seg_slab_ptr) - 1, K, x.size(1), dtype=dtype)
    for g in range(out.size(0)):
        for t in range(int(seg_slab_ptr[g]), int(seg_slab_ptr[g + 1])):
            out[g] += slabs[t, :K]
    return out


def colsum_ref(x, rows, F, prior, accumulate, dtype):
    """-> [F]: (prior if accumulate else 0) + sum of x[r, :F] over r < rows"""
    s = _rowsum(x[:rows, :F], dtype)
    return prior[:F].to(dtype) + s if accumulate else s
