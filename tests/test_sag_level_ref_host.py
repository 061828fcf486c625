"""tests/sag_level_ref.py anchored (no GPU): its forward in float64 to oracle/pyg_ref.py (gcn_conv, topk, filter_adj, sag_pool,
global_max_pool, global_mean_pool), its hand-written backward to float64 autograd of the forward restatement with perm / arg frozen; both
on a mixed batch with one-node graphs, isolated nodes, self loops, ratio 0.5 and 1.0, and a chained second level fed by the first
level's filtered CSR.  And the argument checks of the SAGPool level entry points of csrc/sagpool.hip, answered before any launch."""
import ctypes

import numpy as np
import pytest
import torch

import sag_level_ref as R
from oracle import pyg_ref as P

D = torch.float64
SIZES = [1, 7, 1, 12, 30, 2, 45]


def _batch(seed):
    """symmetric edges inside each graph, nodes 8 and 20 without any edge, a self loop on every seventh node"""
    g = torch.Generator().manual_seed(seed)
    src, dst, off = [], [], 0
    for nb in SIZES:
        if nb > 1:
            a, b = torch.randint(0, nb, (3 * nb,), generator=g) + off, torch.randint(0, nb, (3 * nb,), generator=g) + off
            src += [a, b]; dst += [b, a]
        off += nb
    src, dst = torch.cat(src), torch.cat(dst)
    n = off
    keep = (src != dst) & ~torch.isin(src, torch.tensor([8, 20])) & ~torch.isin(dst, torch.tensor([8, 20]))
    code = torch.unique(src[keep] * n + dst[keep])
    loops = torch.arange(3, n, 7)
    loops = loops[(loops != 8) & (loops != 20)]
    ei = torch.cat([torch.stack([code // n, code % n]), torch.stack([loops, loops])], 1)
    gp = np.concatenate([[0], np.cumsum(SIZES)])
    batch = torch.repeat_interleave(torch.arange(len(SIZES)), torch.tensor(SIZES))
    return ei, n, gp, batch


def _rows(csr, n):
    rp, re, col = csr
    return [col[rp[i]: re[i]].tolist() for i in range(n)]


@pytest.mark.parametrize("ratio", [0.5, 1.0])
def test_forward_is_pyg_ref_in_float64(ratio):
    ei, n, gp, batch = _batch(1)
    F, B = 12, len(SIZES)
    g = torch.Generator().manual_seed(2)
    w_s, b_s = torch.randn(F, generator=g, dtype=D), torch.randn(1, generator=g, dtype=D)
    y = torch.randn(n, F, generator=g, dtype=D)
    csr = R.csr_of(ei, n)
    assert torch.equal(R.edges_of(csr, n), ei[:, torch.sort(ei[1], stable=True).indices])
    for lvl in range(2):                                     # level 1: fed by level 0's filtered CSR and pooled rows
        L = R.level(y, csr, gp, ratio, w_s, b_s, D)
        x = torch.relu(y)
        s_ref = P.gcn_conv(x, ei, w_s.view(-1, 1), b_s).view(-1)
        torch.testing.assert_close(L["score"], s_ref, rtol=1e-12, atol=1e-12)
        dinv, self_w = R.coef(csr, n, D)
        torch.testing.assert_close(R.propagate(csr, dinv, self_w, x), P.gcn_conv(x, ei, torch.eye(F, dtype=D)), rtol=1e-12, atol=1e-12)
        perm_ref = P.topk(s_ref, ratio, batch)
        assert torch.equal(L["perm"], perm_ref)
        assert torch.equal(L["new_id"][perm_ref], torch.arange(perm_ref.numel())) and int((L["new_id"] >= 0).sum()) == perm_ref.numel()
        xr, ei_r, batch_r, _ = P.sag_pool(x, ei, batch, ratio, w_s.view(-1, 1), b_s)
        torch.testing.assert_close(L["xp"], xr, rtol=1e-12, atol=1e-12)
        torch.testing.assert_close(L["out"], torch.cat([P.global_max_pool(xr, batch_r, B), P.global_mean_pool(xr, batch_r, B)], 1),
                                   rtol=1e-12, atol=1e-12)
        K = perm_ref.numel()
        assert torch.equal(ei_r, P.filter_adj(ei, perm_ref, n))
        assert _rows(L["csr_next"], K) == _rows(R.csr_of(ei_r, K), K)                      # kept entries, relabelled, original order
        assert torch.equal(L["cnt"], torch.bincount(ei_r[1], minlength=K))
        torch.testing.assert_close(L["agg_next"], P.gcn_conv(xr, ei_r, torch.eye(F, dtype=D)), rtol=1e-12, atol=1e-12)
        for b in range(B):                                   # arg: a row of the graph that holds the max
            assert torch.equal(L["xp"][L["arg"][b], torch.arange(F)], L["out"][b, :F])
            assert bool(((L["arg"][b] >= L["gp_new"][b]) & (L["arg"][b] < L["gp_new"][b + 1])).all())
        y, csr, ei, gp, batch, n = L["xp"] - 0.05, L["csr_next"], ei_r, L["gp_new"], batch_r, K
    assert n == sum(int(np.ceil(np.float32(ratio) * np.float32(int(np.ceil(np.float32(ratio) * np.float32(s)))))) for s in SIZES)


def test_topk_ties_and_readout_ties():
    gp, gpn = np.array([0, 4, 5, 9]), np.array([0, 2, 3, 5])
    sc = torch.tensor([1.0, 2.0, 2.0, 1.0, 0.0, -0.0, 0.0, 3.0, 0.0])
    perm, nid = R.topk_from(sc, gp, gpn)
    assert perm.tolist() == [1, 2, 4, 7, 5] and nid.tolist() == [-1, 0, 1, -1, 2, 4, -1, 3, -1]
    out, arg = R.readout(torch.tensor([[0.0, 1.0], [-0.0, 1.0], [5.0, 5.0], [-0.0, -1.0], [0.0, -1.0]]), gpn)
    assert arg.tolist() == [[0, 0], [2, 2], [3, 3]] and out[0].tolist() == [0.0, 1.0, 0.0, 1.0]


@pytest.mark.parametrize("form", ["dxp", "last", "dagg"])
@pytest.mark.parametrize("ratio", [0.5, 1.0])
def test_backward_is_float64_autograd_with_frozen_choices(ratio, form):
    ei, n, gp, _ = _batch(3)
    F, B = 8, len(SIZES)
    g = torch.Generator().manual_seed(4)
    w_s, b_s = torch.randn(F, generator=g, dtype=D), torch.randn(1, generator=g, dtype=D)
    y = torch.randn(n, F, generator=g, dtype=D)
    csr = R.csr_of(ei, n)
    for lvl in range(2):
        L = R.level(y, csr, gp, ratio, w_s, b_s, D)
        perm, arg, gpn, K = L["perm"], L["arg"], L["gp_new"], L["perm"].numel()
        dread = torch.randn(B, 2 * F, generator=g, dtype=D)
        dxp = torch.randn(K, F, generator=g, dtype=D)
        kw = {"dxp": dxp} if form == "dxp" else {"dagg_next": dxp, "csr_next": L["csr_next"]} if form == "dagg" else {}
        got = R.backward(y, csr, w_s, L["score"], perm, L["new_id"], arg, gp, gpn, dread, D, **kw)
        yv, wv, bv = y.clone().requires_grad_(True), w_s.clone().requires_grad_(True), b_s.clone().requires_grad_(True)
        xq = R.gather(yv, R.score(yv, csr, wv, bv, D), perm, D)
        kb = torch.from_numpy(np.diff(gpn))
        mean = torch.zeros(B, F, dtype=D).index_add(0, torch.repeat_interleave(torch.arange(B), kb), xq) / kb.to(D).unsqueeze(1)
        loss = (xq.gather(0, arg) * dread[:, :F]).sum() + (mean * dread[:, F:]).sum()
        if form == "dxp":
            loss = loss + (xq * dxp).sum()
        elif form == "dagg":
            loss = loss + (R.propagate(L["csr_next"], L["dinv_next"], L["self_w_next"], xq) * dxp).sum()
        gy, gw, gb = torch.autograd.grad(loss, [yv, wv, bv])
        torch.testing.assert_close(got["du"], gy, rtol=1e-11, atol=1e-12)
        torch.testing.assert_close(got["dws"], gw, rtol=1e-11, atol=1e-12)
        torch.testing.assert_close(got["dbs"], gb, rtol=1e-11, atol=1e-12)
        dropped = L["new_id"] < 0
        assert float(got["dscore"][dropped].abs().sum()) == 0.0 and float(got["dyb"][dropped].abs().sum()) == 0.0
        torch.testing.assert_close(got["du"][dropped], torch.where(y[dropped] > 0, got["dt"][dropped].unsqueeze(1) * w_s, torch.zeros((), dtype=D)))
        y, csr, gp = L["xp"] - 0.05, L["csr_next"], gpn


# ------------------------------------------------------------------------------------------------ argument checks, before any launch
EINVAL, EUNSUPPORTED = -1, -3


def _lib():
    from two_stage_gnn_amd import _native as nat
    return nat.lib()


def _graph_bwd(L, F=32, ldy=32, lddxp=32, lddr=64, lddu=32, col=True, dxp=True, max_seg=40):
    one = ctypes.c_void_p(16)
    return L.tsgnn_sag_pool_graph_bwd_f32(one, ldy, one, one, one, one, one, one if dxp else None, lddxp, one, lddr, one, None,
                                          one if col else None, one, one, one, 3, max_seg, F, one, lddu, one, None, None, None, 0, None,
                                          None, None, None, None, None)


def test_graph_bwd_refuses_short_rows_and_a_null_col():
    L = _lib()
    assert _graph_bwd(L, ldy=28) == EINVAL and _graph_bwd(L, lddu=28) == EINVAL and _graph_bwd(L, lddr=60) == EINVAL
    assert _graph_bwd(L, lddxp=28) == EINVAL
    assert _graph_bwd(L, col=False) == EINVAL
    assert _graph_bwd(L, F=6, ldy=8, lddxp=8, lddu=8) == EUNSUPPORTED and _graph_bwd(L, F=260, ldy=260, lddxp=260, lddr=520, lddu=260) == EUNSUPPORTED
    assert _graph_bwd(L, max_seg=L.tsgnn_sag_pool_graph_max_nodes() + 1) == EUNSUPPORTED
    assert _graph_bwd(L, max_seg=0) == 0 and _graph_bwd(L, max_seg=0, dxp=False, lddxp=0) == 0          # nothing to do: no launch either


def test_pool_bwd_and_du_refuse_short_rows():
    L, one = _lib(), ctypes.c_void_p(16)
    bwd = lambda F=32, ldy=32, lddxp=32, lddr=64, lddy=32, dxp=one, N=0: L.tsgnn_sag_pool_bwd_f32(
        one, ldy, one, one, one, one, one, dxp, lddxp, one, lddr, N, F, 1, one, lddy, one, None)
    assert bwd(ldy=28) == EINVAL and bwd(lddy=28) == EINVAL and bwd(lddr=60) == EINVAL and bwd(lddxp=28) == EINVAL
    assert bwd(dxp=None, lddxp=0) == 0 and bwd() == 0                                                   # N = 0: accepted, no launch
    assert bwd(F=6, ldy=8, lddxp=8, lddy=8) == EUNSUPPORTED and bwd(F=260, ldy=260, lddxp=260, lddr=520, lddy=260) == EUNSUPPORTED
    du = lambda F=32, ldy=32, lddy=32: L.tsgnn_sag_du_f32(one, None, one, one, one, one, one, ldy, one, one, lddy, 5, F, one, one, one, None)
    assert du(ldy=28) == EINVAL and du(lddy=28) == EINVAL
    assert du(F=6, ldy=8, lddy=8) == EUNSUPPORTED and du(F=260, ldy=260, lddy=260) == EUNSUPPORTED


def test_forward_gather_and_readout_argument_checks():
    L, one = _lib(), ctypes.c_void_p(16)
    fwd = lambda F=32, ldy=32, ldo=32, ldout=64, max_seg=40, agg=None, ldagg=0, colnew=None: L.tsgnn_sag_pool_graph_f32(
        one, ldy, one, None, one, one, one, one, one, one, one, 3, max_seg, F, one, one, one, one, ldo, one, one, ldout, one, 0,
        colnew, colnew, colnew, colnew, colnew, agg, ldagg, None)
    assert fwd(ldy=28) == EINVAL and fwd(ldo=28) == EINVAL and fwd(ldout=60) == EINVAL
    assert fwd(agg=one, ldagg=32) == EINVAL and fwd(agg=one, ldagg=28, colnew=one) == EINVAL             # agg_next needs the filter outputs
    assert fwd(F=6, ldy=8, ldo=8) == EUNSUPPORTED and fwd(F=260, ldy=260, ldo=260, ldout=520) == EUNSUPPORTED
    assert fwd(max_seg=L.tsgnn_sag_pool_graph_max_nodes() + 1) == EUNSUPPORTED and fwd(max_seg=0) == 0
    ga = lambda F=32, ldy=32, ldo=32, y=one, xp=one, K=0: L.tsgnn_sag_pool_gather_f32(y, ldy, one, one, one, one, one, K, F, 1, xp, ldo, one, None)
    assert ga(ldy=28) == EINVAL and ga(ldo=28) == EINVAL and ga(y=None) == EINVAL and ga(xp=None) == EINVAL
    assert ga(F=6, ldy=8, ldo=8) == EUNSUPPORTED and ga(F=260, ldy=260, ldo=260) == EUNSUPPORTED and ga(ldy=34) == EUNSUPPORTED
    assert ga() == 0 and ga(y=None, xp=None, ldy=0, ldo=0) == 0                                          # K = 0, both forms
    ro = lambda F=32, ld=32, ldo=64, B=3: L.tsgnn_sag_readout_f32(one, ld, one, B, F, 0, one, ldo, one, None)
    assert ro(ld=28) == EINVAL and ro(ldo=60) == EINVAL and ro(B=0) == EINVAL and ro(F=0) == EINVAL
    assert L.tsgnn_sag_du_reduce_f32(one, 0, 32, one, one, None) == EINVAL and L.tsgnn_sag_du_reduce_f32(one, 4, 6, one, one, None) == EINVAL
