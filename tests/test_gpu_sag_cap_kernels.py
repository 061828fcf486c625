"""The capacity forms of the two per-graph SAGPool level kernels (tsgnn_sag_pool_graph_cap_f32 / tsgnn_sag_pool_graph_bwd_cap_f32,
csrc/sagpool.hip) through the C ABI, on a 3-graph batch whose output allocations have more rows than the batch fills.

Every output lives in a buffer prefilled with one NaN bit pattern (guard_buf.Out) or IPAT (IntOut), with a leading dimension wider than
the row and guard words behind it.  After a launch
  (1) everything the existing entry point writes equals the existing entry point's output BIT FOR BIT (the same kernel body on the same
      inputs; what that body computes is held against float64 by tests/test_gpu_sag_level_kernels.py);
  (2) the padding rows [gp[B], cap) of xp, agg_next (forward) and du (backward) are +0 over columns [0, F);
  (3) row padding, guard words and everything else are what was put there.
Cells: with and without agg_next / dagg_next, F = 32 and 128, 700 padding rows (more than one pass of the four padding workgroups at
either width) and none at all (gp[B] == N)."""
import numpy as np
import pytest
import torch

import sag_level_ref as R
from guard_buf import PAT, Out, _owned
from test_gpu_sag_level_kernels import Batch, IntOut, _i32, _nat, _rc, _same_bits, _strided, _vec, _weights

pytestmark = pytest.mark.gpu

SIZES = (9, 300, 40)
EINVAL = -1


def _forward(Bt, ws, bs, agg, cap_pad):
    """cap_pad None: tsgnn_sag_pool_graph_f32; else its capacity form with K + cap_pad rows in xp / agg_next.  -> the output buffers"""
    nat = _nat()
    n, F, B, gp = Bt.n, Bt.F, Bt.B, Bt.gp
    gpn = R.pooled_gp(gp, 0.5)
    K = int(gpn[-1])
    rows = K + (cap_pad or 0)
    rp, re, col, dinv, self_w = Bt.dev()
    ldy, ldo, ldout, ldagg = F + 4, F + 8, 2 * F + 4, F + 4
    O = {"score": Out(1, n), "xp": Out(rows, ldo), "out": Out(B, ldout), "dinv_new": Out(1, K), "self_w_new": Out(1, K)}
    I = {"perm": IntOut(K), "new_id": IntOut(n), "cnt": IntOut(K), "arg": IntOut(B * F), "rowptr_new": IntOut(K), "rowend_new": IntOut(K),
         "col_new": IntOut(max(int(col.numel()), 1))}
    if agg:
        O["agg_next"] = Out(rows, ldagg)
    yd, gpd, gpnd, wsd = _strided(Bt.y, ldy), _i32(gp), _i32(gpn), ws.cuda()
    nat.call("sag_pool_graph_f32" if cap_pad is None else "sag_pool_graph_cap_f32", yd, ldy, rp, re, col, dinv, self_w, wsd, bs.cuda(), gpd,
             gpnd, B, Bt.max_seg, F, _vec(O["score"], n), I["perm"].t, I["new_id"].t, O["xp"].mat, ldo, I["cnt"].t, O["out"].mat, ldout,
             I["arg"].t, 0, I["rowptr_new"].t, I["rowend_new"].t, I["col_new"].t, _vec(O["dinv_new"], K), _vec(O["self_w_new"], K),
             O["agg_next"].mat if agg else None, ldagg if agg else 0, *(() if cap_pad is None else (rows,)))
    torch.cuda.synchronize()
    return {"O": O, "I": I, "K": K, "rows": rows, "yd": yd, "ldy": ldy, "gpd": gpd, "gpnd": gpnd, "wsd": wsd}


def _backward(Bt, fw, form, cap_pad):
    """form "dagg": the next level's dagg with the forward's filtered CSR; "last": neither dxp nor dagg.  -> (du, part)"""
    nat = _nat()
    n, F, B, K = Bt.n, Bt.F, Bt.B, fw["K"]
    rows = n + (cap_pad or 0)
    rp, re, col, dinv, self_w = Bt.dev()
    g = torch.Generator().manual_seed(3)
    dread, dagg = torch.randn(B, 2 * F, generator=g), torch.randn(K, F, generator=g)
    lddr, lddagg, lddu = 2 * F + 4, F + 8, F + 4
    du, part = Out(rows, lddu), Out(B, F + 4)
    O, I = fw["O"], fw["I"]
    nx = (_strided(dagg, lddagg), lddagg, I["rowptr_new"].t, I["rowend_new"].t, I["col_new"].t, _vec(O["dinv_new"], K),
          _vec(O["self_w_new"], K)) if form == "dagg" else (None, 0, None, None, None, None, None)
    nat.call("sag_pool_graph_bwd_f32" if cap_pad is None else "sag_pool_graph_bwd_cap_f32", fw["yd"], fw["ldy"], _vec(O["score"], n),
             I["new_id"].t, fw["gpd"], fw["gpnd"], I["arg"].t, None, 0, _strided(dread, lddr), lddr, rp, re, col, dinv, self_w, fw["wsd"], B,
             Bt.max_seg, F, du.mat, lddu, part.mat, None, None, *nx, *(() if cap_pad is None else (rows,)))
    torch.cuda.synchronize()
    return du, part


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


@pytest.mark.parametrize("cap_pad", [700, 0])
@pytest.mark.parametrize("agg", [True, False])
@pytest.mark.parametrize("F", [32, 128])
def test_capacity_forms_equal_the_existing_entry_points_and_zero_the_padding_rows(F, agg, cap_pad):
    Bt, (ws, bs) = Batch.make(11, SIZES, F), _weights(F, F)
    n, B = Bt.n, Bt.B
    ref = _forward(Bt, ws, bs, agg, None)
    got = _forward(Bt, ws, bs, agg, cap_pad)
    K, rows = got["K"], got["rows"]
    assert rows == K + cap_pad and K < n
    for k in ("score", "out", "dinv_new", "self_w_new"):
        assert torch.equal(got["O"][k].bits, ref["O"][k].bits), k            # (body, row padding and guard words alike)
    for k in got["I"]:
        assert torch.equal(got["I"][k].buf, ref["I"][k].buf), k
    for k in ("xp", "agg_next") if agg else ("xp",):
        o, r = got["O"][k], ref["O"][k]
        assert _same_bits(o.mat[:K, :F], r.mat[:K, :F].cpu()), k
        assert bool((_bits(o.mat[K:, :F]) == 0).all()), "%s: padding rows are not +0" % k
        o.rest_untouched(k, _owned(rows, o.ld, 0, rows, 0, F))
        r.rest_untouched(k + " (existing entry point)", _owned(K, r.ld, 0, K, 0, F))
    for form in ("dagg", "last") if agg else ("last",):
        du0, part0 = _backward(Bt, ref, form, None)
        du1, part1 = _backward(Bt, got, form, cap_pad)
        assert torch.equal(part1.bits, part0.bits), form
        assert _same_bits(du1.mat[:n, :F], du0.mat[:n, :F].cpu()), form
        assert bool((_bits(du1.mat[n:, :F]) == 0).all()), "du (%s): padding rows are not +0" % form
        du1.rest_untouched("du " + form, _owned(n + cap_pad, du1.ld, 0, n + cap_pad, 0, F))
        assert not bool(du1.mat[:n, :F].isnan().any())


def test_capacity_forms_refuse_a_negative_capacity_without_a_launch():
    F = 32
    Bt, (ws, bs) = Batch.make(11, SIZES, F), _weights(F, F)
    fw = _forward(Bt, ws, bs, False, None)
    n, B, K = Bt.n, Bt.B, fw["K"]
    rp, re, col, dinv, self_w = Bt.dev()
    O, I = fw["O"], fw["I"]
    xp = Out(K, F)
    rc = _rc("sag_pool_graph_cap_f32", fw["yd"], fw["ldy"], rp, re, col, dinv, self_w, fw["wsd"], bs.cuda(), fw["gpd"], fw["gpnd"], B,
             Bt.max_seg, F, _vec(O["score"], n), I["perm"].t, I["new_id"].t, xp.mat, F, I["cnt"].t, O["out"].mat, O["out"].ld, I["arg"].t, 0,
             None, None, None, None, None, None, 0, -1)
    assert rc == EINVAL
    du, part = Out(n, F), Out(B, F + 4)
    rc = _rc("sag_pool_graph_bwd_cap_f32", fw["yd"], fw["ldy"], _vec(O["score"], n), I["new_id"].t, fw["gpd"], fw["gpnd"], I["arg"].t, None,
             0, O["out"].mat, O["out"].ld, rp, re, col, dinv, self_w, fw["wsd"], B, Bt.max_seg, F, du.mat, F, part.mat, None, None, None, 0,
             None, None, None, None, None, -1)
    assert rc == EINVAL
    torch.cuda.synchronize()
    assert all(bool((o.bits == PAT).all()) for o in (xp, du, part))
