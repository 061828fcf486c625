"""The GEMM and weight-gradient building blocks (csrc/gemm.hip, csrc/tn_rows_body.h) one entry point at a time against the float64
restatements of tests/gemm_ref.py, on the smallest shapes that reach their branches.

Every case: outputs (workspaces included) live in guard_buf.Out buffers; the elements the call owns satisfy the rule of
tests/fp32_yardstick.py at K = 8 against the float64 run, with the restatement's own index-ordered float32 run as the yardstick; every
other element and every guard word is bit for bit the pattern; the call is made twice on fresh outputs and the two results are equal
bit for bit (fixed-order sums).  Inputs come from seeded CPU generators.  (The dispatcher of family h allocates its own results: there
the guarded buffers are the passenger's.)

Families: a tsgnn_gemm_f32 dense, b batched / ragged, c tsgnn_gemm_splitk_f32, d tsgnn_colsum_f32, e tsgnn_linear_wgrad_f32,
f tsgnn_linear_wgrad_du_f32, g tsgnn_ragged_tn_f32, h message_passing.linear_wgrad / linear_wgrad_oi.

gemm_tn_rows_kernel<MT,NT,NY> instantiations reached (each asserted by name or by the shape that selects it):
  e, tsgnn_linear_wgrad_f32 — <1,1,1> <1,2,1> <1,3,1> <1,4,1> <2,1,1> <2,2,1> <2,3,1> <2,4,2> <3,1,1> <3,2,1> <3,3,2> <3,4,2> <4,1,1>
     <4,2,2> <4,3,2> <4,4,2>, and the one-block forms of the >= 8-tile shapes at 513 slabs: <2,4,1> <3,3,1> <3,4,1> <4,2,1> <4,3,1> <4,4,1>;
  g, tsgnn_ragged_tn_f32 — <1,1,1> <1,2,1> <1,3,1> <1,4,1> <1,5,1> <1,6,1> <1,7,1> <1,8,2> <2,1,1> <2,2,1> <2,3,1> <2,4,2> <2,5,2> <2,6,2>
     <2,7,2> <2,8,2> <3,1,1> <3,2,1> <3,3,2> <3,4,2> <3,5,2> <4,1,1> <4,2,2> <4,3,2> <4,4,2>."""
import numpy as np
import pytest
import torch

import gemm_ref as G
from fp32_yardstick import _check
from guard_buf import PAT, Out, _owned

pytestmark = pytest.mark.gpu

F32, F64 = torch.float32, torch.float64
RATIO = {}                               # family -> the largest max|hip - ref64| / yardstick of its checks so far


def _nat():
    from two_stage_gnn_amd import _native as nat
    return nat


def _chk(fam, what, hip, ref64, ref32):
    RATIO[fam] = max(RATIO.get(fam, 0.0), _check("%s: %s" % (fam, what), hip, ref64, ref32))


def _report(fam):
    print("family %s: largest ratio so far %.3f (bound 8)" % (fam, RATIO.get(fam, 0.0)))


def _same(what, first, second):
    """two runs of a case (dicts of Out buffers / tensors): equal bit for bit"""
    for k in first:
        a, b = (first[k].bits, second[k].bits) if isinstance(first[k], Out) else (first[k], second[k])
        if a is None and b is None:
            continue
        assert torch.equal(a.view(torch.int32) if a.dtype == F32 else a, b.view(torch.int32) if b.dtype == F32 else b), \
            "%s: %s differs between two runs" % (what, k)


def _all(o):
    return torch.ones(o.rows, o.ld, dtype=torch.bool)


def _none(o):
    return torch.zeros(o.rows, o.ld, dtype=torch.bool)


def _i32(v):
    return torch.tensor(list(v), dtype=torch.int32)


# ------------------------------------------------------------------------------------------------------ a, b: tsgnn_gemm_f32
def _gemm_case(fam, what, A, sam, sak, B, sbk, sbn, crows, cld, coff, scm, scn, M, N, K, batch=1, stride_a=0, stride_b=0, stride_c=0,
               seg=None, ragged=0, max_seg=0, alpha=1.0, accumulate=0, seed=0):
    """one tsgnn_gemm_f32 call with C at flat offset coff of an Out(crows, cld); the elements it owns are those gemm_ref writes"""
    nat = _nat()
    n = crows * cld - coff
    args = (sam, sak, B.view(-1), sbk, sbn)
    tail = (scm, scn, M, N, K, batch, stride_a, stride_b, stride_c, seg, ragged, max_seg, alpha)
    blank = torch.full((n,), float("nan"))
    owned = ~torch.isnan(G.gemm_ref(A.view(-1), *args, blank, *tail, 0, F64))
    prior = blank.clone()
    if accumulate:
        prior[owned] = torch.randn(int(owned.sum()), generator=torch.Generator().manual_seed(seed + 1))
    ref64 = G.gemm_ref(A.view(-1), *args, prior, *tail, accumulate, F64)
    ref32 = G.gemm_ref(A.view(-1), *args, prior, *tail, accumulate, F32)
    Ad, Bd = A.cuda(), B.cuda()
    segd = seg.cuda() if seg is not None else None

    def run():
        O = Out(crows, cld)
        flat = O.mat.view(-1)[coff:]
        if accumulate:
            flat[owned.cuda()] = prior[owned].cuda()
        nat.call("gemm_f32", Ad, sam, sak, Bd, sbk, sbn, flat, scm, scn, M, N, K, batch, stride_a, stride_b, stride_c, segd, ragged,
                 max_seg, float(alpha), int(accumulate))
        torch.cuda.synchronize()
        return {"C": O}
    first = run()
    O = first["C"]
    hip = O.mat.view(-1)[coff:].cpu()
    _chk(fam, what, hip[owned], ref64[owned], ref32[owned])
    full = torch.zeros(crows * cld, dtype=torch.bool)
    full[coff:] = owned
    O.rest_untouched(what, full.view(crows, cld))
    _same(what, first, run())
    return hip, owned


def _stored(gen, rows, cols, trans, pad=3):
    """op(X) [rows, cols] stored plainly ([rows][cols + pad]) or transposed ([cols][rows + pad]) -> (buffer, row stride, column stride);
    never empty: the entry point takes no NULL operand for a product with output elements"""
    r, c = (cols, rows) if trans else (rows, cols)
    buf = torch.randn(max(r, 1), c + pad, generator=gen)
    return (buf, 1, c + pad) if trans else (buf, c + pad, 1)


@pytest.mark.parametrize("M,N,K", [(1, 1, 1), (64, 64, 32), (63, 65, 31), (65, 63, 33), (130, 70, 100)])
def test_a_gemm_dense(M, N, K):
    """one tile exactly, one under and one over in each of M, N and K, several tiles with a short last K chunk; NN / NT / TN / TT as
    strides (both staging maps of each operand), leading dimensions padded by 3, C a column block of a wider row-major buffer and
    transposed, alpha, accumulate onto random values; K = 0 writes zeros / leaves the prior contents"""
    gen = torch.Generator().manual_seed(M * 10000 + N * 100 + K)
    for k in (K, 0):
        for ta in (0, 1):
            for tb in (0, 1):
                A, sam, sak = _stored(gen, M, k, ta)
                B, sbk, sbn = _stored(gen, k, N, tb)
                for layout in ("rowmajor", "transposed"):
                    crows, cld = (M + 2, N + 7) if layout == "rowmajor" else (N + 2, M + 7)
                    scm, scn = (cld, 1) if layout == "rowmajor" else (1, cld)
                    for alpha in (1.0, -0.5):
                        for acc in (0, 1):
                            what = "gemm %dx%dx%d %s%s %s alpha=%g acc=%d" % (M, N, k, "NT"[ta], "NT"[tb], layout, alpha, acc)
                            hip, owned = _gemm_case("a", what, A, sam, sak, B, sbk, sbn, crows, cld, cld + 3, scm, scn, M, N, k,
                                                    alpha=alpha, accumulate=acc, seed=M + N + k)
                            assert int(owned.sum()) == M * N
                            if k == 0 and not acc:
                                assert not bool(hip[owned].any()), what
    _report("a")


SEGS = [0, 1, 31, 32, 33, 70]


@pytest.mark.parametrize("form", ["bmm", "shared_b", "ragged_k", "ragged_m"])
def test_b_gemm_batched(form):
    """strided batches as diffpool._bmm_raw and dense_stack.py launch them (M = N = 33, K = 70; distinct B per batch, and one B shared
    through stride_b = 0); K-ragged as diffpool._ragged_tn's fallback (K argument 0, sam = 1: the empty segment's block becomes zeros);
    M-ragged as diffpool._ragged_nn (M argument 0, max_seg: a segment shorter than the grid returns early, rows of no segment keep the
    pattern, Y through both trans_y stride forms)"""
    gen = torch.Generator().manual_seed(len(form))
    M = N = 33
    K, Bn = 70, 3
    ptr = _i32(np.concatenate([[0], np.cumsum(SEGS)]))
    R, nseg = int(ptr[-1]), len(SEGS)
    if form == "bmm":
        for ta in (0, 1):
            for tb in (0, 1):
                a = torch.randn(Bn, K, M, generator=gen) if ta else torch.randn(Bn, M, K, generator=gen)
                b = torch.randn(Bn, N, K, generator=gen) if tb else torch.randn(Bn, K, N, generator=gen)
                sam, sak = (1, M) if ta else (K, 1)
                sbk, sbn = (1, K) if tb else (N, 1)
                for acc in (0, 1):
                    _gemm_case("b", "bmm ta=%d tb=%d acc=%d" % (ta, tb, acc), a, sam, sak, b, sbk, sbn, Bn * M + 2, N, N, N, 1, M, N, K, Bn,
                               M * K, K * N, M * N, accumulate=acc, seed=ta + tb)
    elif form == "shared_b":
        a = torch.randn(Bn, M, K, generator=gen)                   # dense_stack.py: adj [B, K, K] . x [B, K, ldx]
        for shared in (0, 1):
            b = torch.randn(1 if shared else Bn, K, N + 3, generator=gen)
            for acc in (0, 1):
                _gemm_case("b", "stack product shared=%d acc=%d" % (shared, acc), a, K, 1, b, N + 3, 1, Bn * M + 2, N, N, N, 1, M, N, K,
                           Bn, M * K, 0 if shared else K * (N + 3), M * N, accumulate=acc, seed=shared)
    elif form == "ragged_k":
        S, X = torch.randn(R, M + 3, generator=gen), torch.randn(R, N + 3, generator=gen)
        for acc in (0, 1):
            hip, owned = _gemm_case("b", "ragged K acc=%d" % acc, S, 1, M + 3, X, N + 3, 1, nseg * M + 2, N, N, N, 1, M, N, 0, nseg, 0, 0,
                                    M * N, ptr, 1, max(SEGS), accumulate=acc, seed=4)
            assert int(owned.sum()) == nseg * M * N
            if not acc:
                assert not bool(hip[:M * N].any()), "the empty segment's block is zeros"
    else:
        Kd = 35
        X = torch.randn(R, Kd + 1, generator=gen)
        for trans_y in (0, 1):
            Y = torch.randn(nseg, N, Kd, generator=gen) if trans_y else torch.randn(nseg, Kd, N, generator=gen)
            sbk, sbn = (1, Kd) if trans_y else (N, 1)
            for acc in (0, 1):
                hip, owned = _gemm_case("b", "ragged M trans_y=%d acc=%d" % (trans_y, acc), X, Kd + 1, 1, Y, sbk, sbn, R + 6, N + 3, N + 3,
                                        N + 3, 1, 0, N, Kd, nseg, 0, Kd * N, 0, ptr, 2, max(SEGS), accumulate=acc, seed=trans_y)
                assert int(owned.sum()) == R * N                   # (5 rows behind the last segment and one before the first: no one's)
    _report("b")


# ------------------------------------------------------------------------------------------------------ c: split-K
@pytest.mark.parametrize("ksplit", [1, 2, 3, 4, 7, "plan"])
def test_c_gemm_splitk(ksplit):
    """(M, N) = (92, 128) over K = 100 rows (four chunks of 32) with ksplit passed directly: 3 and 7 leave splits with an empty K
    range, whose slabs must be zeros; accumulate.  "plan": through message_passing.gemm_tn_splitk with the device's plan, which must
    split at least one of the two shapes"""
    nat = _nat()
    if ksplit == "plan":
        from two_stage_gnn_amd import message_passing as mp
        R, split = 1000, []
        for K_in, N in ((130, 6), (10, 6)):
            gen = torch.Generator().manual_seed(K_in)
            z, du = torch.randn(R, K_in + 2, generator=gen), torch.randn(R, N, generator=gen)
            ks, need = np.zeros(1, dtype=np.int32), np.zeros(1, dtype=np.int64)
            nat.call_nostream("gemm_splitk_plan", K_in, N, R, ks.ctypes.data, need.ctypes.data)
            split.append(int(ks[0]))
            zd, dud = z.cuda(), du.cuda()

            def run():
                O = Out(K_in, N)
                mp.gemm_tn_splitk(zd, K_in, dud, out=O.mat)
                torch.cuda.synchronize()
                return {"C": O}
            first = run()
            what = "gemm_tn_splitk %dx%d R=%d ksplit=%d" % (K_in, N, R, split[-1])
            _chk("c", what, first["C"].mat, G._tn(z[:, :K_in], du, F64), G._tn(z[:, :K_in], du, F32))
            first["C"].rest_untouched(what, _all(first["C"]))
            _same(what, first, run())
        assert max(split) > 1, "the plan does not split K for either shape at R = %d: %s" % (R, split)
        _report("c")
        return
    M, N, K, ldz = 92, 128, 100, 96
    gen = torch.Generator().manual_seed(ksplit)
    z, du = torch.randn(K, ldz, generator=gen), torch.randn(K, N, generator=gen)
    prior = torch.randn(M, N, generator=gen)
    zd, dud = z.cuda(), du.cuda()
    per = -(-(-(-K // 32)) // ksplit) * 32                          # rows per split: whole chunks
    for acc in (0, 1):
        def ref(dtype):
            p = G._tn(z[:, :M], du, dtype)
            return prior.to(dtype) + p if acc else p

        def slabs(dtype):
            return torch.stack([G._tn(z[s * per:min(K, (s + 1) * per), :M], du[s * per:min(K, (s + 1) * per)], dtype) for s in range(ksplit)])

        def run():
            C, W = Out(M, N), (Out(ksplit * M, N) if ksplit > 1 else None)
            if acc:
                C.mat.copy_(prior)
            nat.call("gemm_splitk_f32", zd, 1, ldz, dud, N, 1, C.mat, M, N, K, ksplit, W.mat if W is not None else None, acc)
            torch.cuda.synchronize()
            return {"C": C, "ws": W} if W is not None else {"C": C}
        first = run()
        what = "gemm_splitk ksplit=%d acc=%d" % (ksplit, acc)
        _chk("c", what, first["C"].mat, ref(F64), ref(F32))
        first["C"].rest_untouched(what, _all(first["C"]))
        if ksplit > 1:
            W = first["ws"]
            _chk("c", what + " slabs", W.mat.view(ksplit, M, N), slabs(F64), slabs(F32))
            W.rest_untouched(what + " slabs", _all(W))
            for s in range(ksplit):
                if s * per >= K:
                    assert not bool(W.mat.view(ksplit, M, N)[s].any()), "%s: the slab of the empty split %d is not zeros" % (what, s)
        _same(what, first, run())
    _report("c")


# ------------------------------------------------------------------------------------------------------ d: column sums
def _colsum_case(rows, F, acc, gen):
    nat, ld = _nat(), F + 3
    rpc = 512 if rows > 65536 else 128
    nchunk = -(-rows // rpc)
    x = torch.randn(rows, ld, generator=gen)
    prior = torch.randn(F, generator=gen)
    xd = x.cuda()

    def run():
        O, W = Out(1, F), Out(-(-rows // 128), F)                 # the documented workspace bound, guard words right behind it
        if acc:
            O.mat[0].copy_(prior)
        nat.call("colsum_f32", xd, ld, rows, F, O.mat, W.mat, acc)
        torch.cuda.synchronize()
        return {"out": O, "ws": W}
    first = run()
    what = "colsum rows=%d F=%d acc=%d" % (rows, F, acc)
    _chk("d", what, first["out"].mat[0], G.colsum_ref(x, rows, F, prior, acc, F64), G.colsum_ref(x, rows, F, prior, acc, F32))
    first["out"].rest_untouched(what, _all(first["out"]))
    W = first["ws"]

    def parts(dtype):
        return torch.stack([G.colsum_ref(x[c * rpc:], min(rpc, rows - c * rpc), F, None, 0, dtype) for c in range(nchunk)])
    _chk("d", what + " partials", W.mat[:nchunk], parts(F64), parts(F32))
    W.rest_untouched(what + " partials", _owned(W.rows, F, 0, nchunk, 0, F))
    _same(what, first, run())


@pytest.mark.parametrize("F", [1, 63, 64, 65, 130, "long", "norows"])
def test_d_colsum(F):
    """rows at and on both sides of the 4-row lanes, the 32-row unroll and the 128-row chunk, F at and around the 64-column block, ld =
    F + 3, accumulate; 65,537 rows (512-row chunks); no rows: zeros, or the prior contents under accumulate, with NULL x and workspace"""
    if F == "norows":
        nat = _nat()
        for acc in (0, 1):
            O = Out(1, 70)
            O.mat[0] = torch.arange(70.0)
            nat.call("colsum_f32", None, 73, 0, 70, O.mat, None, acc)
            torch.cuda.synchronize()
            assert torch.equal(O.mat[0].cpu(), torch.arange(70.0) if acc else torch.zeros(70))
            O.rest_untouched("colsum of no rows", _all(O))
        return
    gen = torch.Generator().manual_seed(7)
    if F == "long":
        _colsum_case(65537, 4, 0, gen)
    else:
        for rows in (1, 3, 4, 5, 31, 32, 33, 127, 128, 129, 300):
            for acc in (0, 1):
                _colsum_case(rows, F, acc, gen)
    _report("d")


# ------------------------------------------------------------------------------------------------------ e, f: weight-gradient slabs
def _wgrad_operands(gen, rows, bo, K_in, N, nt):
    """z with ldz = ceil4(K_in) + 4; du a column block (from column 4) of a matrix of 32 nt + 8 columns"""
    ldz, lddu = (K_in + 3) // 4 * 4 + 4, 32 * nt + 8
    z, wide = torch.randn(rows + bo, ldz, generator=gen), torch.randn(rows + bo, lddu, generator=gen)
    return z, wide[:, 4:4 + N], z.cuda(), wide.cuda()[:, 4:4 + N]


def _linear_wgrad_case(K_in, N, nt, rows, rps, bo, ny, gen):
    nat = _nat()
    nslab, per = -(-rows // rps), (K_in + 1) * N
    z, du, zd, dud = _wgrad_operands(gen, rows, bo, K_in, N, nt)
    ldz, lddu = zd.stride(0), dud.stride(0)
    assert dud.data_ptr() % 16 == 0 and lddu == 32 * nt + 8
    what = "linear_wgrad %dx%d rows=%d rps=%d bo=%d" % (K_in, N, rows, rps, bo)
    kern = "gemm_tn_rows_kernel<%d,%d,%d>" % ((K_in + 31) // 32, nt, ny)

    def run_slabs():
        W = Out(nslab * (K_in + 1) + 2, N)
        nat.call("linear_wgrad_f32", zd, ldz, dud, lddu, rows, K_in, N, nslab, rps, bo, W.mat, None, None)
        assert nat.last_kernel() == kern, (nat.last_kernel(), kern)
        torch.cuda.synchronize()
        return {"ws": W}
    first = run_slabs()
    W = first["ws"]
    _chk("e", what + " slabs", W.mat[:nslab * (K_in + 1)].view(nslab, K_in + 1, N), G._slab_ref(z, du, rows, K_in, nslab, rps, bo, F64),
         G._slab_ref(z, du, rows, K_in, nslab, rps, bo, F32))
    W.rest_untouched(what + " slabs", _owned(W.rows, N, 0, nslab * (K_in + 1), 0, N))
    _same(what + " slabs", first, run_slabs())
    slab_bits = W.bits[:nslab * per].clone()

    def run_reduced(want_db):
        Ws, DW, DB = Out(nslab * (K_in + 1), N), Out(K_in, N), (Out(1, N) if want_db else None)
        nat.call("linear_wgrad_f32", zd, ldz, dud, lddu, rows, K_in, N, nslab, rps, bo, Ws.mat, DW.mat, DB.mat if want_db else None)
        torch.cuda.synchronize()
        return {"ws": Ws, "dw": DW, "db": DB} if want_db else {"ws": Ws, "dw": DW}
    dw64, db64 = G.tn_ref(z, du, rows, K_in, bo, F64)
    dw32, db32 = G.tn_ref(z, du, rows, K_in, bo, F32)
    full = run_reduced(True)
    _chk("e", what + " dw", full["dw"].mat, dw64, dw32)
    _chk("e", what + " db", full["db"].mat[0], db64, db32)
    for k in ("ws", "dw", "db"):
        full[k].rest_untouched(what + " " + k, _all(full[k]))
    assert torch.equal(full["ws"].bits[:nslab * per], slab_bits), what + ": the slabs differ between the dw = NULL and the reduced form"
    _same(what + " reduced", full, run_reduced(True))
    nodb = run_reduced(False)
    assert torch.equal(nodb["dw"].bits, full["dw"].bits) and torch.equal(nodb["ws"].bits, full["ws"].bits), what + ": db = NULL changes dw"
    _same(what + " reduced, no db", nodb, run_reduced(False))


BIG = [(4, 4, True), (3, 3, False), (2, 4, False), (4, 2, False), (3, 4, False), (4, 3, False)]      # (mt, nt, full tiles) at 513 slabs


@pytest.mark.parametrize("mt,nt", [(m, n) for m in range(1, 5) for n in range(1, 5)] + [(0, 0), (-1, -1)],
                         ids=["%dx%d" % (m, n) for m in range(1, 5) for n in range(1, 5)] + ["one_block_forms", "no_rows"])
def test_e_linear_wgrad_grid(mt, nt):
    """every (MT, NT) of gemm_tn_rows_kernel at the full-tile shape (32 mt, 32 nt) and the partial one (32 mt - 3, 32 nt - 4: a partial
    float4 of z, predicated rows and columns, the bias row's tid < N); slab lengths 16, 64 and 104 rows (one chunk, two chunks, three
    chunks and a part) with a last slab of 1, 7, 9 rows or exactly full; bias-only rows 0 and 5 (not a multiple of the slab count);
    dw = NULL (slabs), dw + db and dw alone (through the closing reduction).  Shapes of >= 8 tiles run with two blocks per slab;
    their one-block form at 513 slabs; no rows: zero gradients, zero slabs"""
    nat = _nat()
    gen = torch.Generator().manual_seed(100 * mt + nt)
    if mt == 0:
        for bmt, bnt, full in BIG:
            K_in, N = (32 * bmt, 32 * bnt) if full else (32 * bmt - (0 if (bmt, bnt) == (3, 3) else 3), 32 * bnt - 4)
            _linear_wgrad_case(K_in, N, bnt, 8200, 16, 5, 1, gen)
        _report("e")
        return
    if mt == -1:
        K_in, N = 92, 64
        for give in ("dw,db", "dw", "slabs"):
            Ws, DW, DB = Out(2 * (K_in + 1), N), Out(K_in, N), Out(1, N)
            nat.call("linear_wgrad_f32", None, 96, None, 64, 0, K_in, N, 2, 16, 0, Ws.mat, DW.mat if give != "slabs" else None,
                     DB.mat if give == "dw,db" else None)
            torch.cuda.synchronize()
            if give == "slabs":
                assert not bool(Ws.mat.any()), "no rows: the slabs are zeros"
                Ws.rest_untouched("no rows", _all(Ws))
                DW.rest_untouched("no rows", _none(DW))
            else:
                assert not bool(DW.mat.any()), "no rows: dw is zeros"
                DW.rest_untouched("no rows", _all(DW))
                Ws.rest_untouched("no rows", _none(Ws))
            assert give != "dw,db" or not bool(DB.mat.any())
            DB.rest_untouched("no rows", _all(DB) if give == "dw,db" else _none(DB))
        return
    ny = 2 if mt * nt >= 8 else 1
    plans = ([(rps, 2 * rps + r) for rps in (16, 64, 104) for r in (0, 1, 7, 9)] if (mt, nt) in ((4, 4), (2, 3), (1, 1))
             else [(64, 2 * 64 + 9)])
    for K_in, N in ((32 * mt, 32 * nt), (32 * mt - 3, 32 * nt - 4)):
        for rps, rows in plans:
            for bo in (0, 5):
                _linear_wgrad_case(K_in, N, nt, rows, rps, bo, ny, gen)
    _report("e")


@pytest.mark.parametrize("nb", [1, 37, 256])
def test_f_linear_wgrad_du(nb):
    """tsgnn_linear_wgrad_du_f32: dw / db bit-equal to tsgnn_linear_wgrad_f32's, the passenger's dws / dbs bit-equal to
    tsgnn_sag_du_reduce_f32 on the same partial rows, both within the yardstick of float64"""
    nat, K_in, N, rows, rps, F_du = _nat(), 64, 64, 150, 64, 64
    nslab = -(-rows // rps)
    gen = torch.Generator().manual_seed(nb)
    z, du, zd, dud = _wgrad_operands(gen, rows, 0, K_in, N, 2)
    part = torch.randn(nb, F_du + 4, generator=gen)
    partd = part.cuda()

    def outs():
        return {"ws": Out(nslab * (K_in + 1), N), "dw": Out(K_in, N), "db": Out(1, N), "dws": Out(1, F_du), "dbs": Out(1, 1)}

    def run():
        o = outs()
        nat.call("linear_wgrad_du_f32", zd, zd.stride(0), dud, dud.stride(0), rows, K_in, N, nslab, rps, o["ws"].mat, o["dw"].mat, o["db"].mat,
                 partd, nb, F_du, o["dws"].mat, o["dbs"].mat)
        torch.cuda.synchronize()
        return o
    first = run()
    what = "linear_wgrad_du nb=%d" % nb
    assert torch.equal(partd.cpu(), part), "the partial rows are inputs"
    plain = outs()
    nat.call("linear_wgrad_f32", zd, zd.stride(0), dud, dud.stride(0), rows, K_in, N, nslab, rps, 0, plain["ws"].mat, plain["dw"].mat,
             plain["db"].mat)
    nat.call("sag_du_reduce_f32", partd, nb, F_du, plain["dws"].mat, plain["dbs"].mat)
    torch.cuda.synchronize()
    _same(what + " against the separate launches", first, plain)
    dw64, db64 = G.tn_ref(z, du, rows, K_in, 0, F64)
    dw32, db32 = G.tn_ref(z, du, rows, K_in, 0, F32)
    _chk("f", what + " dw", first["dw"].mat, dw64, dw32)
    _chk("f", what + " db", first["db"].mat[0], db64, db32)
    s64, s32 = G.colsum_ref(part, nb, F_du + 1, None, 0, F64), G.colsum_ref(part, nb, F_du + 1, None, 0, F32)
    _chk("f", what + " dws", first["dws"].mat[0], s64[:F_du], s32[:F_du])
    _chk("f", what + " dbs", first["dbs"].mat[0], s64[F_du:], s32[F_du:])
    for k, o in first.items():
        o.rest_untouched(what + " " + k, _all(o))
    _same(what, first, run())
    _report("f")


# ------------------------------------------------------------------------------------------------------ g: ragged slabs
SLAB_ROW_PTR = [0, 32, 45, 45, 109, 110, 206]     # a full chunk, a short slab, an empty one, two chunks, one row, three chunks
SEG_SLAB_PTR = [0, 2, 2, 4, 6]                    # the second segment has no slabs: its block is zeros
RAGGED_GRID = [(m, n) for m in range(1, 5) for n in range(1, 9) if m * n <= 16]


@pytest.mark.parametrize("mt,nt", RAGGED_GRID + [(0, 0)], ids=["%dx%d" % p for p in RAGGED_GRID] + ["refusals"])
def test_g_ragged_tn_grid(mt, nt):
    """every (MT, NT) tsgnn_ragged_tn_f32 accepts (mt <= 4, nt <= 8, mt nt <= 16) at the full-tile and the partial shape: the slab
    workspace against its restatement, out per segment; shapes it does not take are refused before anything is written"""
    nat = _nat()
    nslab, nseg, rows = len(SLAB_ROW_PTR) - 1, len(SEG_SLAB_PTR) - 1, SLAB_ROW_PTR[-1]
    srp, ssp = _i32(SLAB_ROW_PTR).cuda(), _i32(SEG_SLAB_PTR).cuda()
    gen = torch.Generator().manual_seed(10 * mt + nt)
    if mt == 0:
        for K, N in ((160, 32), (128, 160), (32, 30)):
            s, x = torch.randn(rows, 164, generator=gen).cuda(), torch.randn(rows, 160, generator=gen).cuda()
            W, O = Out(nslab * (K + 1), N), Out(nseg * K, N)
            assert nat.try_call("ragged_tn_f32", s, 164, x, 160, K, N, srp, nslab, ssp, nseg, W.mat, O.mat) is False, (K, N)
            W.rest_untouched("refused %dx%d" % (K, N), _none(W))
            O.rest_untouched("refused %dx%d" % (K, N), _none(O))
        return
    for K, N in ((32 * mt, 32 * nt), (32 * mt - 3, 32 * nt - 4)):
        s, x, sd, xd = _wgrad_operands(gen, rows, 0, K, N, nt)
        s = s[:, :K]

        def run():
            W, O = Out(nslab * (K + 1) + 2, N), Out(nseg * K, N)
            nat.call("ragged_tn_f32", sd, sd.stride(0), xd, xd.stride(0), K, N, srp, nslab, ssp, nseg, W.mat, O.mat)
            torch.cuda.synchronize()
            return {"ws": W, "out": O}
        first = run()
        what = "ragged_tn %dx%d" % (K, N)
        W, O = first["ws"], first["out"]
        _chk("g", what + " slabs", W.mat[:nslab * (K + 1)].view(nslab, K + 1, N), G.ragged_slab_ref(s, x, SLAB_ROW_PTR, F64),
             G.ragged_slab_ref(s, x, SLAB_ROW_PTR, F32))
        W.rest_untouched(what + " slabs", _owned(W.rows, N, 0, nslab * (K + 1), 0, N))
        r64, r32 = G.ragged_tn_ref(s, x, SLAB_ROW_PTR, SEG_SLAB_PTR, F64), G.ragged_tn_ref(s, x, SLAB_ROW_PTR, SEG_SLAB_PTR, F32)
        hip = O.mat.view(nseg, K, N)
        for g in range(nseg):
            _chk("g", what + " segment %d" % g, hip[g], r64[g], r32[g])
        assert not bool(hip[1].any()), what + ": a segment without slabs is zeros"
        O.rest_untouched(what, _all(O))
        _same(what, first, run())
    _report("g")


# ------------------------------------------------------------------------------------------------------ h: the dispatcher
SLAB3 = ["linear_wgrad_f32"] * 3 + ["wgrad_reduce_multi_f32"]
ROUTES = {                               # route -> (K_in, N, launches with want_db, launches without)
    "slab": (92, 64, ["linear_wgrad_f32"], ["linear_wgrad_f32"]),
    "slab_du_job": (64, 64, ["linear_wgrad_du_f32"], ["linear_wgrad_du_f32"]),
    "row_blocks_260": (260, 64, SLAB3, SLAB3),
    "row_blocks_256": (256, 128, SLAB3[1:], SLAB3[1:]),
    "column_blocks": (92, 264, SLAB3 + ["colsum_f32"], SLAB3),
    "narrow": (1, 64, ["wgrad_narrow_f32"], ["wgrad_narrow_f32"]),
    "splitk": (130, 6, ["gemm_splitk_f32", "colsum_f32"], ["gemm_splitk_f32"]),
    "unaligned_du": (92, 64, ["gemm_splitk_f32", "colsum_f32"], ["gemm_splitk_f32"]),
    "oi_blocks": (92, 264, ["wgrad_blocks_oi_f32"], ["wgrad_blocks_oi_f32"]),
}


@pytest.mark.parametrize("route", list(ROUTES))
def test_h_linear_wgrad_routes(route):
    """message_passing.linear_wgrad on each of its routes (pinned by the launches in nat.trace) and linear_wgrad_oi, with and without
    db, R = 37 and 1000, against tn_ref; a du whose address is not a multiple of 16 takes the split-K fallback and is still right;
    R = 0: all-zero gradients of the right shape on every route, without raising"""
    from two_stage_gnn_amd import message_passing as mp
    nat = _nat()
    K_in, N, names_db, names_nodb = ROUTES[route]
    F_du, nb = 64, 37
    for R in (37, 1000, 0):
        gen = torch.Generator().manual_seed(R + K_in)
        z = torch.randn(R, 1 if route == "narrow" else (K_in + 3) // 4 * 4, generator=gen)
        du = torch.randn(R, N, generator=gen)
        part = torch.randn(nb, F_du + 4, generator=gen)
        zd, partd = z.cuda(), part.cuda()
        if route == "unaligned_du" and R:
            dud = torch.cat([torch.zeros(1), du.view(-1)]).cuda()[1:].view(R, N)
            assert dud.data_ptr() % 16 != 0
        else:
            dud = du.cuda()
        dw64, db64 = G.tn_ref(z, du, R, K_in, 0, F64)
        dw32, db32 = G.tn_ref(z, du, R, K_in, 0, F32)
        for want_db in (True, False):
            what = "%s R=%d db=%d" % (route, R, want_db)

            def run():
                o = {"dws": Out(1, F_du), "dbs": Out(1, 1)} if route == "slab_du_job" else {}
                prev, nat.trace = nat.trace, []
                try:
                    if route == "oi_blocks":
                        dw, db = mp.linear_wgrad_oi(zd, K_in, dud, want_db)
                        dw = dw.t()
                    elif route == "slab_du_job":
                        dw, db = mp.linear_wgrad(zd, K_in, dud, want_db, du_job=(partd, nb, F_du, o["dws"].mat, o["dbs"].mat))
                    else:
                        dw, db = mp.linear_wgrad(zd, K_in, dud, want_db)
                    names = [t[0] for t in nat.trace]
                finally:
                    nat.trace = prev
                torch.cuda.synchronize()
                if R or route != "unaligned_du":                   # (an empty du has no address: nothing to misalign)
                    assert names == (names_db if want_db else names_nodb), (what, names)
                o.update({"dw": dw.contiguous(), "db": db})
                return o
            first = run()
            dw, db = first["dw"], first["db"]
            assert dw.shape == (K_in, N) and (db is None) == (not want_db) and (db is None or db.shape == (N,)), what
            if R == 0:
                assert not bool(dw.any()) and (db is None or not bool(db.any())), what + ": gradients of no rows are zeros"
            _chk("h", what + " dw", dw, dw64, dw32)
            if want_db:
                _chk("h", what + " db", db, db64, db32)
            if route == "slab_du_job":
                s64, s32 = G.colsum_ref(part, nb, F_du + 1, None, 0, F64), G.colsum_ref(part, nb, F_du + 1, None, 0, F32)
                _chk("h", what + " dws", first["dws"].mat[0], s64[:F_du], s32[:F_du])
                _chk("h", what + " dbs", first["dbs"].mat[0], s64[F_du:], s32[F_du:])
                first["dws"].rest_untouched(what, _all(first["dws"]))
                first["dbs"].rest_untouched(what, _all(first["dbs"]))
            _same(what, first, run())
    _report("h")
