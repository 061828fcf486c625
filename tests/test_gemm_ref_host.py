"""tests/gemm_ref.py against torch (float64: einsum / bmm / per-segment loops on the materialised operands, 1e-12 relative; float32:
the index-ordered chain it promises), and the refusals, no-ops and plans of the library's GEMM / weight-gradient entry points that
return before any launch (the library loads without a GPU, tests/test_abi.py)."""
import ctypes

import numpy as np
import pytest
import torch

import gemm_ref as G

EINVAL, OK = -1, 0
F64 = torch.float64


def _close(a, b, what=""):
    scale = max(b.abs().max().item(), 1e-300) if b.numel() else 1.0
    err = (a - b).abs().max().item() if b.numel() else 0.0
    assert a.shape == b.shape and err <= 1e-12 * scale, (what, err, scale)


def _operand(gen, rows, cols, trans, pad, batch=1):
    """a [batch, rows, cols] operand op(X) stored plainly (trans = False: [rows][cols + pad]) or transposed ([cols][rows + pad]);
    -> (flat buffer, stride of the rows index, stride of the cols index, batch stride, the materialised op(X) in float64)"""
    r, c = (cols, rows) if trans else (rows, cols)
    buf = torch.randn(batch, r, c + pad, generator=gen)
    mat = buf[:, :, :c].double()
    if trans:
        return buf.view(-1), 1, c + pad, r * (c + pad), mat.transpose(1, 2)
    return buf.view(-1), c + pad, 1, r * (c + pad), mat


@pytest.mark.parametrize("ta,tb", [(0, 0), (0, 1), (1, 0), (1, 1)], ids=["NN", "NT", "TN", "TT"])
@pytest.mark.parametrize("alpha,accumulate", [(1.0, 0), (-0.5, 0), (1.0, 1), (-0.5, 1)])
def test_gemm_ref_dense_and_strided_batches(ta, tb, alpha, accumulate):
    gen = torch.Generator().manual_seed(10 * ta + tb)
    for M, N, K, batch, shared_b in [(5, 7, 3, 1, False), (4, 3, 6, 3, False), (4, 3, 6, 3, True), (3, 2, 0, 2, False)]:
        A, sam, sak, stra, a = _operand(gen, M, K, ta, 3, batch)
        B, sbk, sbn, strb, b = _operand(gen, K, N, tb, 3, 1 if shared_b else batch)
        ldc, off = N + 3, 2
        C = torch.randn(off + batch * (M + 1) * ldc, generator=gen)
        want = C.double().clone()
        blocks = want[off:off + batch * (M + 1) * ldc].view(batch, M + 1, ldc)
        prod = alpha * torch.einsum("zmk,zkn->zmn", a, b.expand(batch, K, N))
        blocks[:, :M, :N] = blocks[:, :M, :N] + prod if accumulate else prod
        got = G.gemm_ref(A, sam, sak, B, sbk, sbn, C[off:], ldc, 1, M, N, K, batch, stra, 0 if shared_b else strb, (M + 1) * ldc,
                         alpha=alpha, accumulate=accumulate, dtype=F64)
        _close(got, want[off:], "row-major C")              # (unowned elements included: they come back unchanged)
        # C transposed: element (m, n) at n * ldt + m
        ldt = M + 2
        Ct = torch.randn(batch * N * ldt, generator=gen)
        want_t = Ct.double().clone()
        bt = want_t.view(batch, N, ldt)
        bt[:, :, :M] = bt[:, :, :M] + prod.transpose(1, 2) if accumulate else prod.transpose(1, 2)
        got = G.gemm_ref(A, sam, sak, B, sbk, sbn, Ct, 1, ldt, M, N, K, batch, stra, 0 if shared_b else strb, N * ldt, alpha=alpha,
                         accumulate=accumulate, dtype=F64)
        _close(got, want_t, "transposed C")


SEGS = [0, 1, 31, 32, 33, 7]


@pytest.mark.parametrize("accumulate", [0, 1])
def test_gemm_ref_ragged(accumulate):
    gen = torch.Generator().manual_seed(5)
    ptr = np.concatenate([[0], np.cumsum(SEGS)]).astype(np.int32)
    R, Kc, F, nseg = int(ptr[-1]), 5, 6, len(SEGS)
    # ragged = 1: out[z] = S[rows_z]^T X[rows_z]   (sam = 1, sak = lds; the K argument is 0)
    S, X = torch.randn(R, Kc + 3, generator=gen), torch.randn(R, F + 1, generator=gen)
    C = torch.randn(nseg * Kc * F, generator=gen)
    want = C.double().view(nseg, Kc, F).clone()
    for z in range(nseg):
        p = S[ptr[z]:ptr[z + 1], :Kc].double().t() @ X[ptr[z]:ptr[z + 1], :F].double()
        want[z] = want[z] + p if accumulate else p
    got = G.gemm_ref(S.view(-1), 1, Kc + 3, X.view(-1), F + 1, 1, C, F, 1, Kc, F, 0, nseg, 0, 0, Kc * F, ptr, 1, max(SEGS), 1.0,
                     accumulate, F64)
    _close(got, want.view(-1), "ragged K")
    # ragged = 2: out[rows_z] (+)= X[rows_z] Y[z]  (the M argument is 0), rows behind the last segment stay
    for trans_y in (0, 1):
        Y = torch.randn(nseg, F, Kc, generator=gen) if trans_y else torch.randn(nseg, Kc, F, generator=gen)
        sbk, sbn = (1, Kc) if trans_y else (F, 1)
        Xa = torch.randn(R, Kc + 3, generator=gen)
        C = torch.randn((R + 5) * (F + 2), generator=gen)
        want = C.double().view(R + 5, F + 2).clone()
        for z in range(nseg):
            y = Y[z].double().t() if trans_y else Y[z].double()
            p = Xa[ptr[z]:ptr[z + 1], :Kc].double() @ y
            want[ptr[z]:ptr[z + 1], :F] = want[ptr[z]:ptr[z + 1], :F] + p if accumulate else p
        got = G.gemm_ref(Xa.view(-1), Kc + 3, 1, Y.view(-1), sbk, sbn, C, F + 2, 1, 0, F, Kc, nseg, 0, Kc * F, 0, ptr, 2, max(SEGS),
                         1.0, accumulate, F64)
        _close(got, want.view(-1), "ragged M trans_y=%d" % trans_y)
    # no-ops: N = 0, no segment rows
    C = torch.randn(12, generator=gen)
    assert torch.equal(G.gemm_ref(C, 1, 1, C, 1, 1, C, 1, 1, 3, 0, 2, dtype=torch.float32), C)
    assert torch.equal(G.gemm_ref(C, 1, 1, C, 1, 1, C, 1, 1, 0, 3, 2, 1, 0, 0, 0, ptr, 2, 0, dtype=torch.float32), C)
    with pytest.raises(ValueError):
        G.gemm_ref(C, 1, 1, C, 1, 1, C, 1, 1, 1, 1, 1, seg_ptr=ptr, ragged=0)
    with pytest.raises(ValueError):
        G.gemm_ref(C, 1, 1, C, 1, 1, C, 1, 1, 1, 1, 1, ragged=1)


def test_float32_runs_are_index_ordered_chains():
    """the float32 run adds row after row: bit-equal to a scalar numpy float32 chain (product rounded, then added), and a case whose
    result depends on the order comes out as the chain's"""
    gen = torch.Generator().manual_seed(3)
    a, b = torch.randn(37, 3, generator=gen), torch.randn(37, 2, generator=gen)
    want = np.zeros((3, 2), dtype=np.float32)
    an, bn = a.numpy(), b.numpy()
    for r in range(37):
        for k in range(3):
            for n in range(2):
                want[k, n] = np.float32(want[k, n] + np.float32(an[r, k] * bn[r, n]))
    assert np.array_equal(G._tn(a, b, torch.float32).numpy(), want)
    dw, db = G.tn_ref(a, b, 37, 3, 0, torch.float32)
    assert np.array_equal(dw.numpy(), want)
    s = np.zeros(2, dtype=np.float32)
    for r in range(37):
        s = (s + bn[r]).astype(np.float32)
    assert np.array_equal(db.numpy(), s) and np.array_equal(G.colsum_ref(b, 37, 2, None, 0, torch.float32).numpy(), s)
    x = torch.tensor([[2.0 ** 24], [1.0], [1.0], [-2.0 ** 24]])
    assert G._rowsum(x, torch.float32).item() == 0.0 and G._rowsum(x, F64).item() == 2.0
    got = G.gemm_ref(torch.ones(4), 0, 1, x.view(-1), 1, 1, torch.zeros(1), 1, 1, 1, 1, 4, dtype=torch.float32)
    assert got.item() == 0.0


def test_tn_slab_ragged_and_colsum_refs():
    gen = torch.Generator().manual_seed(8)
    rows, bo, K_in, N = 45, 5, 7, 8
    z, du = torch.randn(rows + bo, K_in + 2, generator=gen), torch.randn(rows + bo, N, generator=gen)
    dw, db = G.tn_ref(z, du, rows, K_in, bo, F64)
    _close(dw, z[:rows, :K_in].double().t() @ du[:rows].double(), "tn_ref dw")
    _close(db, du.double().sum(0), "tn_ref db")
    for nslab, rps in [(3, 16), (2, 24), (1, 64), (4, 16)]:       # (the last: an empty slab; 5 bias-only rows over 3, 2, 1, 4 slabs)
        sl = G._slab_ref(z, du, rows, K_in, nslab, rps, bo, F64)
        assert sl.shape == (nslab, K_in + 1, N)
        _close(sl.sum(0)[:K_in], dw, "slabs sum to dw")
        _close(sl.sum(0)[K_in], db, "bias rows sum to db")
        r1 = min(rows, rps)
        _close(sl[0, :K_in], z[:r1, :K_in].double().t() @ du[:r1].double(), "slab 0")
        f32 = G._slab_ref(z, du, rows, K_in, nslab, rps, bo, torch.float32)
        assert f32.dtype == torch.float32 and (f32.double() - sl).abs().max().item() < 1e-4
    ptr, seg = [0, 32, 45, 45, 50], [0, 2, 2, 4]
    s, x = z[:, :K_in], du
    out = G.ragged_tn_ref(s, x, ptr, seg, F64)
    assert out.shape == (3, K_in, N) and not bool(out[1].any())
    _close(out[0], s[0:45].double().t() @ x[0:45].double(), "segment 0")
    _close(out[2], s[45:50].double().t() @ x[45:50].double(), "segment 2")
    slabs = G.ragged_slab_ref(s, x, ptr, F64)
    _close(slabs[1, K_in], x[32:45].double().sum(0), "ragged slab bias row")
    assert not bool(slabs[2].any())
    prior = torch.randn(N, generator=gen)
    _close(G.colsum_ref(du, 40, 5, prior, 0, F64), du[:40, :5].double().sum(0), "colsum")
    _close(G.colsum_ref(du, 40, 5, prior, 1, F64), prior[:5].double() + du[:40, :5].double().sum(0), "colsum accumulate")
    assert not bool(G.colsum_ref(du, 0, 5, prior, 0, F64).any())


# ---------------------------------------------------------------------------------------- the library, before any launch
def _lib():
    from two_stage_gnn_amd import _native as nat
    return nat.lib()


@pytest.fixture(scope="module")
def ptrs():
    """non-NULL, 16-byte aligned host addresses: the calls below must return before anything reads them"""
    buf = np.zeros(64, dtype=np.float32)
    seg = np.zeros(8, dtype=np.int32)
    p = (buf.ctypes.data + 15) & ~15
    yield p, seg.ctypes.data
    assert not buf.any() and not seg.any()


def _gemm(L, p, M=4, N=4, K=4, batch=1, seg=None, ragged=0, max_seg=0, A=True, accumulate=0):
    return L.tsgnn_gemm_f32(p if A else None, 4, 1, p, 4, 1, p, 4, 1, M, N, K, batch, 0, 0, 0, seg, ragged, max_seg, 1.0, accumulate, None)


def test_gemm_refusals_and_noops(ptrs):
    L, (p, seg) = _lib(), ptrs
    for ragged in (0, 3, -1):
        assert _gemm(L, p, seg=seg, ragged=ragged, max_seg=4) == EINVAL            # seg_ptr with ragged not in {1, 2}
    for ragged in (1, 2):
        assert _gemm(L, p, seg=None, ragged=ragged, max_seg=4) == EINVAL           # ragged without seg_ptr
    for batch in (0, -1):
        assert _gemm(L, p, batch=batch) == EINVAL
    assert _gemm(L, p, M=-1) == EINVAL and _gemm(L, p, N=-1) == EINVAL and _gemm(L, p, K=-1) == EINVAL
    assert _gemm(L, p, N=0) == OK                                                   # no output elements: nothing to launch
    assert _gemm(L, p, M=0) == OK
    for max_seg in (0, -5):
        assert _gemm(L, p, M=0, seg=seg, ragged=2, max_seg=max_seg) == OK
    assert _gemm(L, p, N=0, A=False) == OK                                          # ... and nothing to read (empty tensors: NULL)
    # (a product with output elements and a NULL operand)
    assert L.tsgnn_gemm_f32(None, 4, 1, p, 4, 1, p, 4, 1, 4, 4, 4, 1, 0, 0, 0, None, 0, 0, 1.0, 0, None) == EINVAL
    assert L.tsgnn_gemm_f32(p, 4, 1, p, 4, 1, None, 4, 1, 4, 4, 4, 1, 0, 0, 0, None, 0, 0, 1.0, 0, None) == EINVAL


def test_splitk_plan_grid():
    L = _lib()
    ks, ws = ctypes.c_int(-7), ctypes.c_int64(-7)
    seen_split = False
    for M in (1, 64, 65, 512):
        for N in (1, 64, 65, 512):
            for K in (0, 1, 127, 128, 129, 4096, 10 ** 6):
                assert L.tsgnn_gemm_splitk_plan(M, N, K, ctypes.addressof(ks), ctypes.addressof(ws)) == OK
                s = ks.value
                assert 1 <= s <= 256, (M, N, K, s)
                if s > 1:
                    seen_split = True
                    assert 4 * s <= -(-K // 32), (M, N, K, s)                      # >= 4 chunks of 32 per split on average
                    assert ws.value == s * M * N
                else:
                    assert ws.value == 0
    assert seen_split
    assert L.tsgnn_gemm_splitk_plan(4, 4, -1, ctypes.addressof(ks), ctypes.addressof(ws)) == EINVAL
    assert L.tsgnn_gemm_splitk_plan(4, 4, 4, None, ctypes.addressof(ws)) == EINVAL
    # refusals of the product itself (before the K = 0 no-op and before any launch)
    p = ctypes.addressof(ws)
    assert L.tsgnn_gemm_splitk_f32(p, 1, 4, p, 4, 1, None, 4, 4, 0, 1, None, 0, None) == EINVAL
    assert L.tsgnn_gemm_splitk_f32(p, 1, 4, p, 4, 1, p, 0, 4, 0, 1, None, 0, None) == EINVAL
    assert L.tsgnn_gemm_splitk_f32(p, 1, 4, p, 4, 1, p, 4, 4, 0, 0, None, 0, None) == EINVAL
    assert L.tsgnn_gemm_splitk_f32(p, 1, 4, p, 4, 1, p, 4, 4, 64, 2, None, 0, None) == EINVAL     # ksplit > 1 without a workspace
    assert L.tsgnn_gemm_splitk_f32(None, 1, 4, p, 4, 1, p, 4, 4, 64, 1, None, 0, None) == EINVAL  # rows, but no operand


def test_narrow_plan_formula():
    """(K_in + 1) * N floats per chunk of 128 rows up to 65,536 rows, of 512 rows above; one chunk for no rows"""
    L = _lib()
    ws = ctypes.c_int64(-1)
    for rows in (0, 1, 127, 128, 129, 65535, 65536, 65537, 65536 + 512, 10 ** 6):
        for K_in, N in ((1, 8), (4, 130)):
            assert L.tsgnn_wgrad_narrow_plan(rows, K_in, N, ctypes.addressof(ws)) == OK
            rpc = 512 if rows > 65536 else 128
            assert ws.value == max(1, -(-rows // rpc)) * (K_in + 1) * N, (rows, K_in, N)
    for bad in ((-1, 1, 8), (5, 0, 8), (5, 1, 0)):
        assert L.tsgnn_wgrad_narrow_plan(*bad, ctypes.addressof(ws)) == EINVAL
    assert L.tsgnn_wgrad_narrow_plan(5, 1, 8, None) == EINVAL


def test_wgrad_leading_dimensions_are_checked(ptrs):
    """the slab kernel's loads stay inside the matrices only when ldz >= K_in and lddu >= N: both entry points refuse anything else
    (multiples of 4, so that the refusal is this check's)"""
    L, (p, _) = _lib(), ptrs
    for ldz, lddu in ((88, 64), (92, 60), (0, 64), (92, 0), (-4, 64)):
        assert L.tsgnn_linear_wgrad_f32(p, ldz, p, lddu, 100, 92, 64, 2, 64, 0, p, p, p, None) == EINVAL, (ldz, lddu)
        assert L.tsgnn_linear_wgrad_f32(p, ldz, p, lddu, 100, 92, 64, 2, 64, 0, p, None, None, None) == EINVAL, (ldz, lddu)
        assert L.tsgnn_linear_wgrad_f32(p, ldz, p, lddu, 0, 92, 64, 1, 16, 0, p, p, p, None) == EINVAL, (ldz, lddu)
        assert L.tsgnn_linear_wgrad_du_f32(p, ldz, p, lddu, 100, 92, 64, 2, 64, p, p, p, p, 3, 64, p, p, None) == EINVAL, (ldz, lddu)
    # the other refusals that precede the launch: no workspace, no slabs, rows without operands, an unsupported width
    assert L.tsgnn_linear_wgrad_f32(p, 92, p, 64, 100, 92, 64, 2, 64, 0, None, p, p, None) == EINVAL
    assert L.tsgnn_linear_wgrad_f32(p, 92, p, 64, 100, 92, 64, 0, 64, 0, p, p, p, None) == EINVAL
    assert L.tsgnn_linear_wgrad_f32(None, 92, p, 64, 100, 92, 64, 2, 64, 0, p, p, p, None) == EINVAL
    assert L.tsgnn_linear_wgrad_f32(p, 92, None, 64, 100, 92, 64, 2, 64, 0, p, p, p, None) == EINVAL
    assert L.tsgnn_linear_wgrad_f32(None, 92, p, 64, 0, 92, 64, 1, 16, 5, p, p, p, None) == EINVAL       # bias-only rows are rows
    assert L.tsgnn_linear_wgrad_f32(p, 132, p, 64, 100, 132, 64, 2, 64, 0, p, p, p, None) == -3
    assert L.tsgnn_linear_wgrad_f32(p, 92, p, 64, 100, 92, 62, 2, 64, 0, p, p, p, None) == -3
    assert L.tsgnn_colsum_f32(p, 4, 10, 8, p, p, 0, None) == EINVAL                                       # ld < F
    assert L.tsgnn_colsum_f32(None, 8, 10, 8, p, p, 0, None) == EINVAL
    assert L.tsgnn_colsum_f32(p, 8, 10, 8, p, None, 0, None) == EINVAL
    assert L.tsgnn_colsum_f32(p, 8, 0, 8, None, p, 0, None) == EINVAL
    assert L.tsgnn_colsum_f32(p, 8, -1, 8, p, p, 0, None) == EINVAL
