"""The four launches of the two small triplet tails — csrc/triplet.hip (tsgnn_triplet_embed_fwd_f32 / _bwd_f32: one Linear on the three
readout rows + both pairwise distances) and csrc/mlp2_triplet.hip (tsgnn_mlp2_triplet_fwd_f32 / _bwd_f32: Linear-ReLU-Linear) — one
by one against torch in float64, at the scheme of tests/fp32_yardstick.py: max|hip - ref64| <= 8 * max(max|cpu32 - ref64|,
2^-23 max|ref64|), the yardstick being the SAME torch code in fp32 on the CPU.  (The mlp3 tail has its own in test_gpu_sag_triplet.py.)

The cells go through the C ABI, as tests/test_gpu_posttrain_cls.py does: only there can r and w be strided views and every output sit
in a guarded buffer (tests/guard_buf.py: every word one NaN pattern, guard words behind it); the autograd wrappers around the same
launches, triplet._TripletTail and eigen_triplet._Mlp2TripletTail, make their inputs contiguous and allocate their own outputs, and
are run in the anchor-equals-positive tests.  Shapes: the smallest that reach each path — D in {4 (fewer float4 than lanes), 36 (a
partial 32-column backward slice), 260 (a second lane pass, nine workgroups)}, E and H in {1 (fewer than the rows a wave requests
together), 5 / 50 (no multiple of 8), 130 (a second pass of the 16 waves)}, every value with both extremes of the others.  Each cell
runs with three sets of embeddings that reach the loss directly — (), (1,), (0, 1, 2): NULL and non-NULL upstream pointers — the two
distances always do."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from fp32_yardstick import EPS32, K_DEFAULT, _check, _yardstick
from guard_buf import Out

pytestmark = pytest.mark.gpu

EPS = 1e-6                                       # F.pairwise_distance's default (resident.EPS)
EMBED_CELLS = [(4, 1), (4, 5), (4, 130), (36, 1), (36, 130), (260, 1), (260, 5), (260, 130)]                  # (D, E)
MLP2_CELLS = [(4, 1, 1), (4, 130, 130), (260, 1, 130), (260, 130, 1), (36, 1, 130), (36, 130, 1), (4, 50, 130), (260, 50, 1),
              (4, 130, 5), (260, 1, 5)]                                                                        # (D, H, E)
WIDE_LDR = {(260, 5), (260, 50, 1)}              # r: a view at row stride D + 8, NaN in the padding
WIDE_LDW = {(36, 130)}                           # triplet_embed only: w a view at row stride D + 4
SUBSETS = [(), (1,), (0, 1, 2)]


def _tail_loss(dp, dn, es, used):
    loss = torch.nn.MarginRankingLoss(margin=1.5)(dp, dn, torch.full_like(dp, -1.0)) + 0.3 * dn.sum()
    coef = (0.05, -0.07, 0.11)
    for i in used:
        loss = loss + coef[i] * es[i].norm(2) + 0.01 * es[i].sum()
    return loss


def _tail_ref(r, w, dtype, used):
    """torch: Linear (ReLU Linear)* on three rows + both pairwise distances; the loss touches the distances and the embeddings in
    `used`.  w = [W1, b1(, W2, b2)] -> {name: tensor}, the names being the launches' outputs"""
    r = r.to(dtype).clone().requires_grad_(True)
    w = [t.to(dtype).clone().requires_grad_(True) for t in w]
    o = {}
    e = F.linear(r, w[0], w[1])
    if len(w) == 4:
        o["h"] = F.relu(e).detach()
        e = F.linear(F.relu(e), w[2], w[3])
    dp, dn = F.pairwise_distance(e[0:1], e[1:2], 2, EPS), F.pairwise_distance(e[0:1], e[2:3], 2, EPS)
    g = torch.autograd.grad(_tail_loss(dp, dn, [e[0:1], e[1:2], e[2:3]], used), [r] + w + [e])
    o.update(de=g[-1], embed=e.detach(), dist=torch.cat([dp, dn]).detach().view(1, 2), dr=g[0], dw1=g[1], db1=g[2].view(1, -1))
    if len(w) == 4:
        o.update(dw2=g[3], db2=g[4].view(1, -1))
    return o


def _upstream(o, used):
    """the loss's gradient on the launch's own distances and embeddings: (g_dp, g_dn, g_ea, g_ep, g_en), None where it has none"""
    d = o["dist"].mat.detach().clone().view(2).requires_grad_(True)
    e = o["embed"].mat.detach().clone().requires_grad_(True)
    es = [e[0:1], e[1:2], e[2:3]]
    loss = _tail_loss(d[0:1], d[1:2], es, used)
    gd, ge = torch.autograd.grad(loss, [d, e], allow_unused=True)
    return [gd[0:1].contiguous(), gd[1:2].contiguous()] + [ge[i].contiguous() if i in used else None for i in range(3)]


def _strided(t, ld, wide):
    """t [n, k] on the device, as a view at row stride ld (NaN in the padding) where wide"""
    if not wide:
        return t.cuda().contiguous(), t.size(1)
    buf = torch.full((t.size(0), ld), float("nan"), dtype=torch.float32, device="cuda")
    buf[:, :t.size(1)] = t.cuda()
    return buf, ld


def _inputs(cell, seed):
    gen = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=gen)
    r = rn(3, cell[0])
    w = []
    for k, n in zip(cell[:-1], cell[1:]):
        w += [rn(n, k) / k ** 0.5, 0.3 * rn(n)]
    return r, w


def _run_embed(cell, r, w, used):
    from two_stage_gnn_amd import _native as nat
    D, E = cell
    rp, ldr = _strided(r, D + 8, cell in WIDE_LDR)
    wp, ldw = _strided(w[0], D + 4, cell in WIDE_LDW)
    b = w[1].cuda()
    o = {k: Out(*s) for k, s in {"embed": (3, E), "dist": (1, 2), "dr": (3, D), "dw1": (E, D), "db1": (1, E)}.items()}
    nat.call("triplet_embed_fwd_f32", rp, ldr, wp, ldw, b, D, E, EPS, o["embed"].mat, o["dist"].mat)
    assert nat.last_kernel() == "triplet_embed_fwd_kernel"
    g = _upstream(o, used)
    nat.call("triplet_embed_bwd_f32", rp, ldr, wp, ldw, D, E, EPS, o["embed"].mat, o["dist"].mat, *g, o["dr"].mat, D, o["dw1"].mat, D,
             o["db1"].mat)
    assert nat.last_kernel() == "triplet_embed_bwd_kernel"
    return o


def _run_mlp2(cell, r, w, used):
    from two_stage_gnn_amd import _native as nat
    D, H, E = cell
    assert nat.lib().tsgnn_mlp2_triplet_supported(D, H, E) == 1
    rp, ldr = _strided(r, D + 8, cell in WIDE_LDR)
    w1, b1, w2, b2 = [t.cuda().contiguous() for t in w]
    o = {k: Out(*s) for k, s in {"h": (3, H), "embed": (3, E), "dist": (1, 2), "dr": (3, D), "dw1": (H, D), "db1": (1, H),
                                 "dw2": (E, H), "db2": (1, E)}.items()}
    nat.call("mlp2_triplet_fwd_f32", rp, ldr, w1, b1, w2, b2, D, H, E, EPS, o["h"].mat, o["embed"].mat, o["dist"].mat)
    assert nat.last_kernel() == "mlp2_triplet_fwd_kernel"
    g = _upstream(o, used)
    nat.call("mlp2_triplet_bwd_f32", rp, ldr, w1, w2, o["h"].mat, o["embed"].mat, o["dist"].mat, EPS, *g, D, H, E, o["dr"].mat, D,
             o["dw1"].mat, o["db1"].mat, o["dw2"].mat, o["db2"].mat)
    assert nat.last_kernel() == "mlp2_triplet_bwd_kernel"
    return o


def _check_out(what, k, hip, ref64, cpu32):
    """output k against the dicts of _tail_ref: fp32_yardstick._check, but for the last layer's bias gradient"""
    if k != ("db2" if "db2" in ref64 else "db1"):
        return _check("%s %s" % (what, k), hip, ref64[k], cpu32[k])
    _check_row_sum("%s %s" % (what, k), hip, ref64[k], cpu32[k], ref64["de"])


def _check_row_sum(what, hip, ref64, cpu32, terms64):
    """fp32_yardstick._check for the last layer's bias gradient, the column sum of the three rows of de.  The rows cancel — to exactly
    0 where no embedding reaches the loss directly: de = (tp + tn, -tp, -tn) — and fp32 rounds a sum at the scale of its TERMS.  Where
    the yardstick is below 2^-23 max|de| (0 in cells where fp64 and the fp32 reference both return 0: no finite K exists there) that
    floor takes its place; every other cell is _check as it is.  K stays K_DEFAULT either way"""
    floor = EPS32 * terms64.abs().max().item()
    if _yardstick(ref64, cpu32) >= floor:
        return _check(what, hip, ref64, cpu32)
    hip = hip.detach().cpu()
    assert hip.shape == ref64.shape, (what, hip.shape, ref64.shape)
    assert not torch.isnan(hip).any().item(), "%s: an element was never written" % what
    ratio = (hip.double() - ref64).abs().max().item() / floor
    print("%s: max|hip - ref64| / (2^-23 max|de|, the yardstick's floor here) = %.3f" % (what, ratio))
    assert ratio <= K_DEFAULT, "%s: %.3f x the floored fp32 yardstick (bound %g)" % (what, ratio, K_DEFAULT)


def _compare(what, o, r, w, used):
    """every output written, nothing behind it touched, and within the yardstick of float64"""
    torch.cuda.synchronize()
    ref64, cpu32 = _tail_ref(r, w, torch.float64, used), _tail_ref(r, w, torch.float32, used)
    assert set(o) | {"de"} == set(ref64)
    for k, b in o.items():
        b.rest_untouched("%s %s" % (what, k), torch.ones(b.rows, b.ld, dtype=torch.bool))
        _check_out(what, k, b.mat, ref64, cpu32)
    return ref64


@pytest.mark.parametrize("used", SUBSETS, ids=lambda u: "used" + "".join(map(str, u)))
@pytest.mark.parametrize("cell", EMBED_CELLS, ids=lambda s: "D%d_E%d" % s)
def test_triplet_embed_against_fp64(cell, used):
    r, w = _inputs(cell, 11 * EMBED_CELLS.index(cell))
    _compare("embed %s %s" % (cell, used), _run_embed(cell, r, w, used), r, w, used)


@pytest.mark.parametrize("used", SUBSETS, ids=lambda u: "used" + "".join(map(str, u)))
@pytest.mark.parametrize("cell", MLP2_CELLS, ids=lambda s: "D%d_H%d_E%d" % s)
def test_mlp2_triplet_against_fp64(cell, used):
    r, w = _inputs(cell, 13 * MLP2_CELLS.index(cell) + 1)
    _compare("mlp2 %s %s" % (cell, used), _run_mlp2(cell, r, w, used), r, w, used)


@pytest.mark.parametrize("cell", [(36, 130), (36, 50, 130)], ids=["embed", "mlp2"])
def test_anchor_equals_positive_gives_torchs_finite_values(cell):
    """a is p: dist_p = ||eps|| exactly, and its gradient is torch's finite one, not NaN — through the C ABI and through the autograd
    wrapper of the same two launches"""
    from two_stage_gnn_amd import eigen_triplet as ET, triplet as T3
    E = cell[-1]
    r, w = _inputs(cell, 4)
    r[1] = r[0]
    used = (0,)
    o = (_run_embed if len(cell) == 2 else _run_mlp2)(cell, r, w, used)
    ref64 = _compare("a is p %s" % (cell,), o, r, w, used)
    for k, b in o.items():
        assert bool(torch.isfinite(b.mat).all()), k
    assert torch.equal(o["embed"].mat[0], o["embed"].mat[1])
    assert abs(float(o["dist"].mat[0, 0]) - 1e-6 * np.sqrt(E)) <= 1e-11 and abs(float(ref64["dist"][0, 0]) - 1e-6 * np.sqrt(E)) <= 1e-11
    rg = r.cuda().requires_grad_(True)
    wg = [t.cuda().requires_grad_(True) for t in w]
    dp, dn, ea, ep, en = (T3._TripletTail if len(cell) == 2 else ET._Mlp2TripletTail).apply(rg, *wg)
    g = torch.autograd.grad(_tail_loss(dp, dn, [ea, ep, en], used), [rg] + wg)
    assert torch.equal(torch.cat([dp, dn]), o["dist"].mat.view(2)) and torch.equal(torch.cat([ea, ep, en]), o["embed"].mat)
    cpu32 = _tail_ref(r, w, torch.float32, used)
    for k, t in zip(["dr", "dw1", "db1", "dw2", "db2"], g):
        assert bool(torch.isfinite(t).all()), k
        _check_out("a is p %s autograd" % (cell,), k, t.view(ref64[k].shape), ref64, cpu32)
