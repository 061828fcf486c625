"""The GCN-scorer SAGPool level kernels (csrc/sagpool.hip, topk_segments of csrc/pooling.hip) one by one through their C entry points
against tests/sag_level_ref.py in float64.

Every float output lives in a buffer prefilled with one NaN bit pattern (guard_buf.Out), with a leading dimension wider than the row where
the entry point takes one and guard words behind it; integer outputs are prefilled with IPAT (IntOut).  After a launch
  (1) score, xp, out, agg_next, du, part, dws, dbs (and the composed path's dyb, dscore, propagate outputs) are held to the rule of
      tests/fp32_yardstick.py at K = 8: the yardstick is sag_level_ref's own float32 run on the CPU, never the kernel;
  (2) perm / new_id equal topk_from() of the kernel's OWN fp32 scores, arg the first row attaining the max in the kernel's OWN xp, cnt and
      the filtered CSR equal filter_adj of the kernel's perm entry for entry, packed from each graph's old segment base, and dinv_new /
      self_w_new equal 1 / sqrtf(d) computed in float32 bit for bit;
  (3) everything else (row padding, guard words, col_new outside every new row) is bit for bit what was put there.
In the tie-free cells the float64 reference's gap between the last kept and the first dropped score exceeds 64 x the score yardstick in
EVERY graph with k < n (a condition on the seeds, asserted), and the kernel's perm is then the float64 reference's as far as that condition
decides it: see _perm_is_the_references().  Two adjacent nodes with the same closed neighbourhood tie by structure under the GCN
normalisation; the tie-free batches hold none (_without_twins), the tie cells (every score equal; rings with constant rows) are made of them.

Worst  max|hip - ref64| / yardstick  per kernel over this module (bound 8; each test prints its own), measured on an MI355X (256 CUs):
    sag_pool_graph        1.10   (chained, F 256, level 0, out)        sag_pool_graph_bwd    4.98   (grid batch, F 256, dxp given: dbs)
    sag_pool_bwd          1.76   (F 256, relu_in 0, dxp NULL: dscore)  sag_du                2.91   (F 36, explicit row ends: dbs)
    sag_du_reduce         3.16   (nb 257, F 100: dbs)                  sag_pool_gather       0.82   sag_readout           0.20
    gcn_propagate_re      1.33 float4 / 1.03 generic / 1.30 narrow     gcn_propagate_affine  1.27
dbs is ONE float per launch, so its ratio is one sample of a rounding error; every tensor of more than one element stayed below 3.
No kernel failed a cell.  The bit-for-bit coefficients are compared with sag_level_ref.coef_f32 and not with torch's float32
1 / sqrt: that one is not correctly rounded on every CPU (it differed from the kernels' v_sqrt + IEEE division in a few elements).
"""
import numpy as np
import pytest
import torch

import sag_level_ref as R
from fp32_yardstick import _check, _yardstick
from guard_buf import GUARD, PAT, Out, _owned
from test_gpu_pyg import tie_free

pytestmark = pytest.mark.gpu

EINVAL, EUNSUPPORTED = -1, -3
IPAT = -7
D, S32 = torch.float64, torch.float32
GRID_SIZES = (1, 2, 5, 8, 9, 64, 255, 257, 1024, 1025)
GRID_F = (4, 32, 36, 64, 100, 128, 132, 256)


def _nat():
    from two_stage_gnn_amd import _native as nat
    return nat


def _rc(name, *args):
    """the entry point's return code (call() raises on anything but 0)"""
    nat = _nat()
    return getattr(nat.lib(), "tsgnn_" + name)(*[nat._arg(a) for a in args], nat.stream_handle())


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _strided(t, ld):
    """an INPUT [rows, ld] on the device: t in the first columns, NaN in the padding"""
    b = torch.full((t.size(0), ld), float("nan"), dtype=torch.float32)
    b[:, :t.size(1)] = t
    return b.cuda()


def _i32(t):
    return torch.as_tensor(np.asarray(t)).to(torch.int32).cuda()


class IntOut:
    """n int32 on the device, every word IPAT, GUARD words behind"""

    def __init__(self, n):
        self.n = n
        self.buf = torch.full((n + GUARD,), IPAT, dtype=torch.int32, device="cuda")
        self.t = self.buf[:n]

    def get(self, what):
        torch.cuda.synchronize()
        b = self.buf.cpu()
        assert bool((b[self.n:] == IPAT).all()), "%s: guard words overwritten" % what
        return b[:self.n].long()

    def untouched(self):
        torch.cuda.synchronize()
        return bool((self.buf == IPAT).all().item())


class Worst:
    """the worst ratio per kernel a test saw; printed at its end"""

    def __init__(self):
        self.w = {}

    def check(self, kernel, what, hip, r64, r32):
        r = _check("%s %s" % (kernel, what), hip, r64, r32, K=8)
        if r >= self.w.get(kernel, (-1.0, ""))[0]:
            self.w[kernel] = (r, what)
        return r

    def report(self):
        for k, (r, what) in sorted(self.w.items()):
            print("WORST %s: %.3f (%s)" % (k, r, what))


def _vec(O, n):
    """a 1-D output that lives in Out(1, n)"""
    return O.mat[0, :n]


def _same_bits(hip, want):
    a, b = hip.detach().cpu().contiguous().view(torch.int32), want.contiguous().view(torch.int32)
    if not torch.equal(a, b):
        bad = (a != b).nonzero().view(-1)
        print("bit mismatch at %d of %d elements, first %s: %r != %r" % (bad.numel(), a.numel(), bad[:4].tolist(),
                                                                        hip.detach().cpu()[bad[:4]].tolist(), want[bad[:4]].tolist()))
    return torch.equal(a, b)


def _full(O, what):
    O.rest_untouched(what, torch.ones(O.rows, O.ld, dtype=torch.bool))


# ============================================================================= batches
def _edges(seed, sizes, deg=3, special=True, hub=74, loops=True):
    """symmetric edge list of a batch.  Graphs of >= 32 + hub nodes (special): node 0 isolated, node 1 one neighbour, node 2 eight, node 3
    nine, node 4 (the hub) hub + 1 of them, more than a 64-lane group; random pairs among the other nodes.  Self loops on every node whose
    index inside its graph is 5 mod 7 (about one in seven)."""
    g = torch.Generator().manual_seed(seed)
    src, dst, off = [torch.zeros(0, dtype=torch.int64)], [torch.zeros(0, dtype=torch.int64)], 0
    for nb in sizes:
        sp = special and nb >= 32 + hub
        lo = 5 if sp else 0
        if nb - lo > 1:
            src.append(torch.randint(lo, nb, (deg * nb,), generator=g) + off)
            dst.append(torch.randint(lo, nb, (deg * nb,), generator=g) + off)
        if sp:
            a = [1] + [2] * 8 + [3] * 9 + [4] * (hub + 1)
            b = [10] + list(range(11, 19)) + list(range(20, 29)) + list(range(30, 31 + hub))
            src.append(torch.tensor(a) + off); dst.append(torch.tensor(b) + off)
        off += nb
    src, dst = torch.cat(src), torch.cat(dst)
    keep = src != dst
    src, dst = torch.cat([src[keep], dst[keep]]), torch.cat([dst[keep], src[keep]])
    n = off
    code = torch.unique(src * n + dst)
    ei = _without_twins(torch.stack([code // n, code % n]), n)
    if loops:
        local = torch.cat([torch.arange(nb) for nb in sizes])
        lp = (local % 7 == 5).nonzero().view(-1)
        ei = torch.cat([ei, torch.stack([lp, lp])], 1)
    return ei, n


def _without_twins(ei, n):
    """two ADJACENT nodes with the same closed neighbourhood have the same GCN score whatever the features (the two nodes of a 2-node
    graph, a triangle, an edge that is a component of its own): an exact tie by structure, which the tie-free cells must not contain (the
    ring and all-zero batches are the tie cells).  Removes the edge between such twins, until there are none."""
    while True:
        nb = [{i} for i in range(n)]
        for s, d in zip(ei[0].tolist(), ei[1].tolist()):
            nb[d].add(s)
        groups = {}
        for i in range(n):
            if len(nb[i]) > 1:
                groups.setdefault(frozenset(nb[i]), []).append(i)
        twins = torch.full((n,), -1, dtype=torch.int64)
        for q, g in enumerate(groups.values()):
            if len(g) > 1:
                twins[torch.tensor(g)] = q
        drop = (twins[ei[0]] >= 0) & (twins[ei[0]] == twins[ei[1]])
        if not bool(drop.any()):
            return ei
        ei = ei[:, ~drop]


class Batch:
    """one level's inputs: the CPU reference's view (y, csr, gp) and the device's (rowptr / rowend / col, dinv / self_w in float32)"""

    def __init__(self, y, csr, gp, dev_rowptr=None, dev_rowend=None, dev_col=None, dinv=None, self_w=None):
        self.y, self.csr, self.gp = y, csr, np.asarray(gp, dtype=np.int64)
        self.n, self.F, self.B = y.size(0), y.size(1), len(gp) - 1
        self.max_seg = int(np.diff(self.gp).max())
        self._dev = (dev_rowptr, dev_rowend, dev_col, dinv, self_w)

    @classmethod
    def make(cls, seed, sizes, F, y=None, **kw):
        ei, n = _edges(seed, sizes, **kw)
        y = tie_free(seed + 1000 * F, n, F) if y is None else y
        return cls(y, R.csr_of(ei, n), np.concatenate([[0], np.cumsum(sizes)]))

    def dev(self):
        """(rowptr, rowend, col, dinv, self_w) on the device, and the host copy of rowptr"""
        rp, re, col, dinv, self_w = self._dev
        if rp is None:
            d32, s32 = R.coef_f32(self.csr, self.n)                     # 1.0f / sqrtf(d) to the bit: what tsgnn_gcn_coef_f32 gives
            rp, re, col, dinv, self_w = _i32(self.csr[0]), None, _i32(self.csr[2]), d32.cuda(), s32.cuda()
            self._dev = (rp, re, col, dinv, self_w)
        return self._dev


def _gap_margin(sc64, sc32, gp, gpn):
    """min over the graphs with k < n of (last kept - first dropped score) / the score yardstick, in the float64 reference"""
    yard = _yardstick(sc64, sc32)
    worst = float("inf")
    for b in range(len(gp) - 1):
        n, k = gp[b + 1] - gp[b], gpn[b + 1] - gpn[b]
        if k < n:
            s = torch.sort(sc64[gp[b]: gp[b + 1]], descending=True).values
            worst = min(worst, float(s[k - 1] - s[k]) / yard)
    return worst


def _perm_is_the_references(tag, perm_k, nid_k, sc64, yard, gp, gpn):
    """what the gap condition lets the float64 reference decide.  The gap at the cut fixes the kept SET of every graph: it must be the
    reference's.  The ORDER inside the kept rows is fixed only between scores that are themselves more than 64 yardsticks apart (4,096
    scores of one graph lie closer than float32 resolves, whatever the seed): the kernel's order may not invert such a pair, and where
    every neighbouring pair of the reference's order is that far apart the two perms are equal."""
    ref_perm, ref_nid = R.topk_from(sc64, gp, gpn)
    assert torch.equal(nid_k >= 0, ref_nid >= 0), tag + ": the kept rows differ from the float64 reference's"
    same = torch.from_numpy(np.repeat(np.arange(len(gpn) - 1), np.diff(gpn)))
    same = same[1:] == same[:-1]
    s = sc64[perm_k]
    assert bool(((s[:-1] - s[1:] > -64.0 * yard) | ~same).all()), tag + ": perm inverts two scores the float64 reference tells apart"
    r = sc64[ref_perm]
    if bool(((r[:-1] - r[1:] > 64.0 * yard) | ~same).all()):
        assert torch.equal(perm_k, ref_perm), tag + ": perm differs from the float64 reference's"


def _weights(seed, F):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(F, generator=g) / np.sqrt(F), torch.randn(1, generator=g)


# ============================================================================= the forward launch and its checks
def _forward(Bt, ws, bs, ratio, W, tag, filt=True, agg=True, pad=4, tie_free_cell=True, twice=False):
    """sag_pool_graph_f32 on Bt, every output checked.  -> the launch's outputs (device) and the reference's level (float64)"""
    nat = _nat()
    n, F, B, gp = Bt.n, Bt.F, Bt.B, Bt.gp
    gpn = R.pooled_gp(gp, ratio)
    K = int(gpn[-1])
    rp, re, col, dinv, self_w = Bt.dev()
    rp_host = rp.cpu().long().numpy()
    yd, gpd, gpnd = _strided(Bt.y, F + pad), _i32(gp), _i32(gpn)
    wsd, bsd = ws.cuda(), bs.cuda()
    ldo, ldout, ldagg = F + 8, 2 * F + 4, F + 4
    O = {"score": Out(1, n), "xp": Out(K, ldo), "out": Out(B, ldout)}
    I = {"perm": IntOut(K), "new_id": IntOut(n), "cnt": IntOut(K), "arg": IntOut(B * F)}
    if filt:
        O.update({"dinv_new": Out(1, K), "self_w_new": Out(1, K)})
        I.update({"rowptr_new": IntOut(K), "rowend_new": IntOut(K), "col_new": IntOut(max(int(col.numel()), 1))})
        if agg:
            O["agg_next"] = Out(K, ldagg)
    f = lambda k: _vec(O[k], O[k].ld) if k in O else None
    i = lambda k: I[k].t if k in I else None

    def launch(accumulate):
        nat.call("sag_pool_graph_f32", yd, F + pad, rp, re, col, dinv, self_w, wsd, bsd, gpd, gpnd, B, Bt.max_seg, F, f("score"), i("perm"),
                 i("new_id"), O["xp"].mat, ldo, i("cnt"), O["out"].mat, ldout, i("arg"), accumulate, i("rowptr_new"), i("rowend_new"),
                 i("col_new"), f("dinv_new"), f("self_w_new"), O["agg_next"].mat if "agg_next" in O else None, ldagg if "agg_next" in O else 0)
    launch(0)
    # ---- reference
    sc64, sc32 = R.score(Bt.y, Bt.csr, ws, bs, D), R.score(Bt.y, Bt.csr, ws, bs, S32)
    W.check("sag_pool_graph", tag + " score", _vec(O["score"], n), sc64, sc32)
    _full(O["score"], tag + " score")
    sck = _vec(O["score"], n).cpu()
    perm_k, nid_k = I["perm"].get(tag + " perm"), I["new_id"].get(tag + " new_id")
    perm_own, nid_own = R.topk_from(sck, gp, gpn)
    assert torch.equal(perm_k, perm_own), tag + ": perm is not the top-k of the kernel's own scores"
    assert torch.equal(nid_k, nid_own), tag + ": new_id"
    if tie_free_cell:
        margin = _gap_margin(sc64, sc32, gp, gpn)
        print("%s: score gap at the cut / yardstick >= %.1f" % (tag, margin))
        assert margin > 64.0, "%s: the seed leaves a gap of %.1f yardsticks at the cut; choose another seed" % (tag, margin)
        _perm_is_the_references(tag, perm_k, nid_k, sc64, _yardstick(sc64, sc32), gp, gpn)
    L64, L32 = R.level(Bt.y, Bt.csr, gp, ratio, ws, bs, D, perm=perm_k), R.level(Bt.y, Bt.csr, gp, ratio, ws, bs, S32, perm=perm_k)
    W.check("sag_pool_graph", tag + " xp", O["xp"].mat[:, :F], L64["xp"], L32["xp"])
    O["xp"].rest_untouched(tag + " xp", _owned(K, ldo, 0, K, 0, F))
    W.check("sag_pool_graph", tag + " out", O["out"].mat[:, :2 * F], L64["out"], L32["out"])
    O["out"].rest_untouched(tag + " out", _owned(B, ldout, 0, B, 0, 2 * F))
    arg_k = I["arg"].get(tag + " arg").view(B, F)
    assert torch.equal(arg_k, R.readout(O["xp"].mat[:, :F].cpu(), gpn)[1]), tag + ": arg is not the first row attaining the max"
    cnt_k = I["cnt"].get(tag + " cnt")
    assert torch.equal(cnt_k, L64["cnt"]), tag + ": cnt"
    if filt:
        rpn, ren, coln = I["rowptr_new"].get(tag), I["rowend_new"].get(tag), I["col_new"].get(tag)
        # rows packed from each graph's old segment base, in perm order: inside the old segment, none overlapping another
        kb = np.diff(gpn)
        first = torch.from_numpy(np.repeat(gpn[:-1], kb))
        ex = torch.cumsum(cnt_k, 0) - cnt_k
        want_rp = torch.from_numpy(rp_host[np.repeat(gp[:-1], kb)]) + ex - ex[first]
        assert torch.equal(rpn, want_rp) and torch.equal(ren, want_rp + cnt_k), tag + ": new rows are not packed from the old segment base"
        rows, src = R.entries((rpn, ren, coln), K)
        assert torch.equal(src, L64["csr_next"][2]), tag + ": col_new"
        covered = torch.zeros(coln.numel(), dtype=torch.bool)
        pos = torch.repeat_interleave(rpn, cnt_k) + (torch.arange(int(cnt_k.sum())) - torch.repeat_interleave(ex, cnt_k))
        covered[pos] = True
        assert int(covered.sum()) == int(cnt_k.sum()) and bool((coln[~covered] == IPAT).all()), tag + ": col_new written outside the new rows"
        dn32, sn32 = R.coef_f32(L64["csr_next"], K)
        for k, want in (("dinv_new", dn32), ("self_w_new", sn32)):
            assert _same_bits(_vec(O[k], K), want), tag + ": " + k
            _full(O[k], tag + " " + k)
        if agg:
            W.check("sag_pool_graph", tag + " agg_next", O["agg_next"].mat[:, :F], L64["agg_next"], L32["agg_next"])
            O["agg_next"].rest_untouched(tag + " agg_next", _owned(K, ldagg, 0, K, 0, F))
    if twice:                                               # accumulate = 1 on the same out: twice the readout
        launch(1)
        W.check("sag_pool_graph", tag + " out (accumulate)", O["out"].mat[:, :2 * F], 2 * L64["out"], L32["out"] + L32["out"])
        O["out"].rest_untouched(tag + " out (accumulate)", _owned(B, ldout, 0, B, 0, 2 * F))
        assert torch.equal(I["perm"].get(tag), perm_k) and torch.equal(I["arg"].get(tag).view(B, F), arg_k)
    return {"O": O, "I": I, "L64": L64, "perm": perm_k, "new_id": nid_k, "arg": arg_k, "gpn": gpn, "K": K, "yd": yd, "ldy": F + pad,
            "gpd": gpd, "gpnd": gpnd, "wsd": wsd, "sc64": sc64, "sc32": sc32}


def _next_batch(Bt, fw, seed):
    """the second level's inputs: level 0's pooled rows (shifted so that the relu cuts some), the KERNEL's filtered CSR with explicit row
    ends at the old bases and its coefficients on the device; the reference's compact filtered CSR beside them"""
    O, I, K = fw["O"], fw["I"], fw["K"]
    y1 = (fw["L64"]["xp"].float() + 0.25 * tie_free(seed, K, Bt.F)).contiguous()
    return Batch(y1, fw["L64"]["csr_next"], fw["gpn"], I["rowptr_new"].t, I["rowend_new"].t, I["col_new"].t, _vec(O["dinv_new"], K),
                 _vec(O["self_w_new"], K))


# ============================================================================= the backward launch and its checks
def _backward(Bt, fw, ws, W, tag, form="dxp", own_reduce=True, nxt=None, seed=1):
    """sag_pool_graph_bwd_f32 with perm / arg / score from the forward launch fw.  form: dxp | last | dagg (nxt = the forward outputs that
    hold the next level's CSR: fw itself).  own_reduce: dws / dbs given; else NULL and tsgnn_sag_du_reduce_f32 sums the partial rows"""
    nat = _nat()
    n, F, B, gp, gpn, K = Bt.n, Bt.F, Bt.B, Bt.gp, fw["gpn"], fw["K"]
    rp, re, col, dinv, self_w = Bt.dev()
    g = torch.Generator().manual_seed(seed)
    dread = torch.randn(B, 2 * F, generator=g)
    dx = torch.randn(K, F, generator=g)
    lddr, lddxp, lddu = 2 * F + 4, F + 8, F + 4
    du, part, dws, dbs = Out(n, lddu), Out(B, F + 4), Out(1, F), Out(1, 1)
    dxd = _strided(dx, lddxp) if form != "last" else None
    O, I = fw["O"], fw["I"]
    nx = (dxd, lddxp, I["rowptr_new"].t, I["rowend_new"].t, I["col_new"].t, _vec(O["dinv_new"], K), _vec(O["self_w_new"], K)) \
        if form == "dagg" else (None, 0, None, None, None, None, None)
    nat.call("sag_pool_graph_bwd_f32", fw["yd"], fw["ldy"], _vec(O["score"], n), I["new_id"].t, fw["gpd"], fw["gpnd"], I["arg"].t,
             dxd if form == "dxp" else None, lddxp if form == "dxp" else 0, _strided(dread, lddr), lddr, rp, re, col, dinv, self_w, fw["wsd"],
             B, Bt.max_seg, F, du.mat, lddu, part.mat, _vec(dws, F) if own_reduce else None, _vec(dbs, 1) if own_reduce else None, *nx)
    kw = {"dxp": dx} if form == "dxp" else {"dagg_next": dx, "csr_next": fw["L64"]["csr_next"]} if form == "dagg" else {}
    r64 = R.backward(Bt.y, Bt.csr, ws, fw["sc64"], fw["perm"], fw["new_id"], fw["arg"], gp, gpn, dread, D, **kw)
    r32 = R.backward(Bt.y, Bt.csr, ws, fw["sc32"], fw["perm"], fw["new_id"], fw["arg"], gp, gpn, dread, S32, **kw)
    W.check("sag_pool_graph_bwd", tag + " du", du.mat[:, :F], r64["du"], r32["du"])
    du.rest_untouched(tag + " du", _owned(n, lddu, 0, n, 0, F))
    dropped = fw["new_id"] < 0                              # dropped rows: du = dt w_s [y > 0] (the prefill is NaN: a stale read shows)
    if bool(dropped.any()):
        z = torch.zeros((), dtype=D)
        W.check("sag_pool_graph_bwd", tag + " du (dropped rows)", du.mat[:, :F][dropped.cuda()],
                torch.where(Bt.y[dropped] > 0, r64["dt"][dropped].unsqueeze(1) * ws.double(), z), r32["du"][dropped])
    p64, p32 = r64["part"].clone(), r32["part"].clone()
    if own_reduce and B > 256:                              # the two-stage reduction leaves each 64-row chunk's sum in the chunk's first row
        for q in range(0, B, 64):
            p64[q], p32[q] = r64["part"][q: q + 64].sum(0), r32["part"][q: q + 64].sum(0)
    W.check("sag_pool_graph_bwd", tag + " part", part.mat[:, :F + 1], p64, p32)
    part.rest_untouched(tag + " part", _owned(B, F + 4, 0, B, 0, F + 1))
    if not own_reduce:
        assert _vec(dws, F).isnan().all() and _vec(dbs, 1).isnan().all()
        nat.call("sag_du_reduce_f32", part.mat, B, F, _vec(dws, F), _vec(dbs, 1))
    W.check("sag_pool_graph_bwd" if own_reduce else "sag_du_reduce", tag + " dws", _vec(dws, F), r64["dws"], r32["dws"])
    W.check("sag_pool_graph_bwd" if own_reduce else "sag_du_reduce", tag + " dbs", _vec(dbs, 1), r64["dbs"], r32["dbs"])
    _full(dws, tag + " dws"); _full(dbs, tag + " dbs")
    part.rest_untouched(tag + " part after the reduction", _owned(B, F + 4, 0, B, 0, F + 1))
    return r64


# seeds chosen on the CPU so that the float64 reference alone satisfies the gap condition of every cell that uses them
GRID_SEED = {4: 14, 32: 11, 36: 12, 64: 11, 100: 11, 128: 11, 132: 11, 256: 12}


def _grid_batch(F):
    return Batch.make(GRID_SEED[F], GRID_SIZES, F)


def test_grid_batch_has_the_rows_the_kernels_branch_on():
    Bt = _grid_batch(4)
    lens = (Bt.csr[1] - Bt.csr[0][:-1]).tolist()
    assert {0, 1, 8, 9} <= set(lens) and max(lens) >= 70
    rows, src = R.entries(Bt.csr, Bt.n)
    assert 0.1 < float((rows == src).sum()) / Bt.n < 0.2


# ============================================================================= forward + backward over the width grid
@pytest.mark.parametrize("F", GRID_F)
def test_width_grid_ratio_half(F):
    """ratio 0.5, filter outputs and agg_next, accumulate 0 then 1; backward with dxp given and the kernel's own reduction, then the last
    level's form (dxp NULL) with dws / dbs NULL and the partial rows summed by sag_du_reduce"""
    W = Worst()
    Bt, (ws, bs) = _grid_batch(F), _weights(F, F)
    fw = _forward(Bt, ws, bs, 0.5, W, "grid F%d r0.5" % F, twice=True, pad=8 if F % 8 else 4)
    _backward(Bt, fw, ws, W, "grid F%d dxp" % F, form="dxp", own_reduce=True)
    _backward(Bt, fw, ws, W, "grid F%d last" % F, form="last", own_reduce=False)
    W.report()


@pytest.mark.parametrize("F,ratio", [(36, 1.0), (256, 1.0), (36, 0.01), (256, 0.01)])
def test_width_grid_other_ratios(F, ratio):
    """ratio 1.0 (nothing dropped: the filter is a relabelling) and 0.01 (k = 1 up to 100 nodes), forward and backward"""
    W = Worst()
    Bt, (ws, bs) = _grid_batch(F), _weights(F + 1, F)
    fw = _forward(Bt, ws, bs, ratio, W, "grid F%d r%g" % (F, ratio))
    if ratio == 0.01:
        assert (np.diff(fw["gpn"])[:6] == 1).all()
    _backward(Bt, fw, ws, W, "grid F%d r%g dxp" % (F, ratio), form="dxp", own_reduce=True)
    W.report()


@pytest.mark.parametrize("F,filt", [(4, False), (128, False), (64, True), (100, True)])
def test_width_grid_without_filter_or_agg_next(F, filt):
    """all filter outputs NULL (what the last level passes), and the filter without agg_next"""
    W = Worst()
    Bt, (ws, bs) = _grid_batch(F), _weights(F + 2, F)
    fw = _forward(Bt, ws, bs, 0.5, W, "grid F%d filt%d" % (F, filt), filt=filt, agg=False)
    _backward(Bt, fw, ws, W, "grid F%d filt%d last" % (F, filt), form="last", own_reduce=True)
    W.report()


# ============================================================================= exact ties
@pytest.mark.parametrize("F", [32, 256])
def test_every_score_equal(F):
    """every y <= 0 (with exact +0.0 and -0.0 among them): all scores equal b_s, perm = the first k nodes of each graph; every xp is +-0, so
    every readout column ties: arg = the graph's first kept row"""
    W = Worst()
    sizes = (1, 2, 9, 40, 257, 1025)
    n = sum(sizes)
    y = -tie_free(5, n, F).abs()
    y[::3, ::2] = 0.0
    y[1::3, 1::2] = -0.0
    Bt, (ws, bs) = Batch.make(21, sizes, F, y=y), _weights(F + 3, F)
    assert float(bs) != 0.0
    fw = _forward(Bt, ws, bs, 0.5, W, "zeros F%d" % F, tie_free_cell=False)
    sck = _vec(fw["O"]["score"], n).cpu()
    assert bool((sck == bs).all())
    gp, gpn = Bt.gp, fw["gpn"]
    first_k = torch.cat([torch.arange(gp[b], gp[b] + gpn[b + 1] - gpn[b]) for b in range(Bt.B)])
    assert torch.equal(fw["perm"], first_k)
    assert torch.equal(fw["arg"], torch.from_numpy(gpn[:-1]).view(-1, 1).expand(Bt.B, F))
    assert float(fw["O"]["xp"].mat[:, :F].abs().max()) == 0.0
    _backward(Bt, fw, ws, W, "zeros F%d dxp" % F, form="dxp", own_reduce=True)
    W.report()


@pytest.mark.parametrize("F", [36, 128])
def test_ring_graphs_with_constant_rows(F):
    """rings with one feature row per graph: equal degrees give bit-equal scores inside a graph (the IMDB-B situation); perm = first k"""
    W = Worst()
    sizes = (3, 8, 17, 40, 300, 1030)
    src, off = [], 0
    for nb in sizes:
        a = torch.arange(nb)
        src.append(torch.stack([a + off, (a + 1) % nb + off])); off += nb
    e = torch.cat(src, 1)
    ei = torch.cat([e, e.flip(0)], 1)
    n = off
    rows = tie_free(7, len(sizes), F)
    y = torch.repeat_interleave(rows, torch.tensor(sizes), 0).contiguous()
    gp = np.concatenate([[0], np.cumsum(sizes)])
    Bt, (ws, bs) = Batch(y, R.csr_of(ei, n), gp), _weights(F + 4, F)
    fw = _forward(Bt, ws, bs, 0.5, W, "rings F%d" % F, tie_free_cell=False)
    sck, gpn = _vec(fw["O"]["score"], n).cpu(), fw["gpn"]
    for b in range(Bt.B):
        assert bool((sck[gp[b]: gp[b + 1]] == sck[gp[b]]).all()), b
    assert torch.equal(fw["perm"], torch.cat([torch.arange(gp[b], gp[b] + gpn[b + 1] - gpn[b]) for b in range(Bt.B)]))
    _backward(Bt, fw, ws, W, "rings F%d dagg" % F, form="dagg", own_reduce=True)
    W.report()


# ============================================================================= 256-thread workgroups, two-stage reductions
SMALL_SEED = {32: 31, 256: 31}


@pytest.mark.parametrize("extra", [1, 0])
@pytest.mark.parametrize("F", [32, 256])
def test_small_graphs_on_either_side_of_the_workgroup_threshold(F, extra):
    """B = 2 x CUs + 1 graphs of 1..40 nodes run 256-thread workgroups, the same graphs without the last one 1,024-thread ones; more than
    256 partial rows: the kernel's own reduction takes two stages"""
    W = Worst()
    B = 2 * _cus() + extra
    sizes = (torch.randint(1, 41, (2 * _cus() + 1,), generator=torch.Generator().manual_seed(3)).tolist())[:B]
    Bt, (ws, bs) = Batch.make(SMALL_SEED[F], sizes, F), _weights(F + 5, F)
    assert Bt.max_seg <= 256 and B > 256
    tag = "B%d F%d" % (B, F)
    fw = _forward(Bt, ws, bs, 0.5, W, tag)
    _backward(Bt, fw, ws, W, tag + " dagg", form="dagg", own_reduce=True)
    _backward(Bt, fw, ws, W, tag + " dxp", form="dxp", own_reduce=False)
    W.report()


def test_two_stage_reduction_with_wide_workgroups():
    """B = 257 < 2 x CUs: 1,024-thread workgroups, 257 partial rows"""
    W = Worst()
    assert 257 <= 2 * _cus()
    sizes = torch.randint(1, 30, (257,), generator=torch.Generator().manual_seed(4)).tolist()
    Bt, (ws, bs) = Batch.make(41, sizes, 64), _weights(9, 64)
    fw = _forward(Bt, ws, bs, 0.5, W, "B257 F64")
    _backward(Bt, fw, ws, W, "B257 F64 dxp", form="dxp", own_reduce=True)
    W.report()


# ============================================================================= the size limit
def test_largest_graph_and_one_node_more():
    """one graph of tsgnn_sag_pool_graph_max_nodes() nodes beside a 3-node graph at F = 256: ~152 KiB of dynamic LDS; one node more is
    unsupported and writes nothing"""
    W = Worst()
    nat = _nat()
    mx, F = int(nat.lib().tsgnn_sag_pool_graph_max_nodes()), 256
    Bt, (ws, bs) = Batch.make(51, (mx, 3), F), _weights(10, F)
    fw = _forward(Bt, ws, bs, 0.5, W, "max_nodes F256", filt=False)
    _backward(Bt, fw, ws, W, "max_nodes F256 last", form="last", own_reduce=True)
    n, B, K = Bt.n, 2, fw["K"]
    rp, re, col, dinv, self_w = Bt.dev()
    sc, xp, out = Out(1, n), Out(K, F), Out(B, 2 * F)
    perm, nid, cnt, arg = IntOut(K), IntOut(n), IntOut(K), IntOut(B * F)
    rc = _rc("sag_pool_graph_f32", fw["yd"], fw["ldy"], rp, re, col, dinv, self_w, fw["wsd"], bs.cuda(), fw["gpd"], fw["gpnd"], B, mx + 1, F,
             _vec(sc, n), perm.t, nid.t, xp.mat, F, cnt.t, out.mat, 2 * F, arg.t, 0, None, None, None, None, None, None, 0)
    assert rc == EUNSUPPORTED
    torch.cuda.synchronize()
    assert all(bool((o.bits == PAT).all()) for o in (sc, xp, out)) and all(o.untouched() for o in (perm, nid, cnt, arg))
    du, part = Out(n, F), Out(B, F + 4)
    rc = _rc("sag_pool_graph_bwd_f32", fw["yd"], fw["ldy"], _vec(fw["O"]["score"], n), fw["I"]["new_id"].t, fw["gpd"], fw["gpnd"],
             fw["I"]["arg"].t, None, 0, out.mat, 2 * F, rp, re, col, dinv, self_w, fw["wsd"], B, mx + 1, F, du.mat, F, part.mat, None, None,
             None, 0, None, None, None, None, None)
    assert rc == EUNSUPPORTED
    torch.cuda.synchronize()
    assert bool((du.bits == PAT).all()) and bool((part.bits == PAT).all())
    W.report()


# ============================================================================= chained levels
CHAIN_SEED = {32: (62, 38), 100: (61, 106), 256: (61, 300)}     # (batch, score weights): with F = 256 the hub must be KEPT


@pytest.mark.parametrize("F", [32, 100, 256])
def test_chained_levels(F):
    """level 0's filtered CSR (explicit row ends, rows in score order at the old bases with gaps, dinv_new / self_w_new as coefficients)
    feeds a second call, checked against the reference's second level; level 0's backward receives dagg_next with that CSR.  The next level
    holds rows of more than 64 kept neighbours (F = 256: G = 64) and of 9 (F = 32: G = 8)"""
    W = Worst()
    Bt = Batch.make(CHAIN_SEED[F][0], (1, 2, 7, 40, 300, 1025), F, deg=5, hub=180)
    ws, bs = _weights(CHAIN_SEED[F][1], F)
    fw0 = _forward(Bt, ws, bs, 0.5, W, "chain F%d level 0" % F)
    cnt = fw0["L64"]["cnt"]
    assert int(cnt.max()) > 64 and bool((cnt == 9).any()) and bool((cnt == 0).any())
    B1 = _next_batch(Bt, fw0, 62)
    assert B1.dev()[1] is not None
    ws1, bs1 = _weights(F + 7, F)
    fw1 = _forward(B1, ws1, bs1, 0.5, W, "chain F%d level 1" % F, twice=True)
    _backward(B1, fw1, ws1, W, "chain F%d level 1 dagg" % F, form="dagg", own_reduce=True)
    _backward(Bt, fw0, ws, W, "chain F%d level 0 dagg" % F, form="dagg", own_reduce=True)
    _backward(Bt, fw0, ws, W, "chain F%d level 0 dagg, reduce apart" % F, form="dagg", own_reduce=False, seed=2)
    W.report()


# ============================================================================= the composed-path kernels
COMP_SIZES = (1, 7, 40, 300)


def _comp_level(F, ratio=0.5, seed=71, hub=74):
    """a small level in the reference (float64 and float32) with the reference's own discrete choices"""
    Bt, (ws, bs) = Batch.make(seed, COMP_SIZES, F, hub=hub), _weights(F + 8, F)
    L64 = R.level(Bt.y, Bt.csr, Bt.gp, ratio, ws, bs, D)
    L32 = R.level(Bt.y, Bt.csr, Bt.gp, ratio, ws, bs, S32, perm=L64["perm"])
    return Bt, ws, bs, L64, L32


@pytest.mark.parametrize("F", [4, 36, 100, 256])
def test_sag_pool_bwd(F):
    W = Worst()
    nat = _nat()
    Bt, ws, bs, L64, _ = _comp_level(F)
    n, B, gpn, K = Bt.n, Bt.B, L64["gp_new"], L64["perm"].numel()
    g = torch.Generator().manual_seed(F)
    dread, dx = torch.randn(B, 2 * F, generator=g), torch.randn(K, F, generator=g)
    sc = L64["score"].float()
    row_graph_new = np.repeat(np.arange(B), np.diff(gpn))
    for relu_in in (1, 0):
        for given in (True, False):
            dyb, ds = Out(n, F + 4), Out(1, n)
            nat.call("sag_pool_bwd_f32", _strided(Bt.y, F + 8), F + 8, sc.cuda(), _i32(L64["new_id"]), _i32(row_graph_new), _i32(gpn),
                     _i32(L64["arg"].reshape(-1)), _strided(dx, F + 4) if given else None, F + 4 if given else 0, _strided(dread, 2 * F + 8),
                     2 * F + 8, n, F, relu_in, dyb.mat, F + 4, _vec(ds, n))
            kw = dict(dxp=dx if given else None, relu_in=bool(relu_in))
            r64 = R.backward(Bt.y, Bt.csr, ws, sc, L64["perm"], L64["new_id"], L64["arg"], Bt.gp, gpn, dread, D, **kw)
            r32 = R.backward(Bt.y, Bt.csr, ws, sc, L64["perm"], L64["new_id"], L64["arg"], Bt.gp, gpn, dread, S32, **kw)
            tag = "F%d relu%d dxp%d" % (F, relu_in, given)
            W.check("sag_pool_bwd", tag + " dyb", dyb.mat[:, :F], r64["dyb"], r32["dyb"])
            W.check("sag_pool_bwd", tag + " dscore", _vec(ds, n), r64["dscore"], r32["dscore"])
            dyb.rest_untouched(tag, _owned(n, F + 4, 0, n, 0, F)); _full(ds, tag)
            dropped = (L64["new_id"] < 0).cuda()
            assert float(dyb.mat[:, :F][dropped].abs().sum()) == 0.0 and float(_vec(ds, n)[dropped].abs().sum()) == 0.0
    W.report()


def _du_case(W, tag, Bt, F, rowend):
    nat = _nat()
    n = Bt.n
    g = torch.Generator().manual_seed(n + F)
    ws, dscore, dyb0 = torch.randn(F, generator=g), torch.randn(n, generator=g), torch.randn(n, F, generator=g)
    csr = Bt.csr
    if rowend:                                              # explicit ends: every third row loses its last entry
        re = csr[1].clone()
        cut = (torch.arange(n) % 3 == 0) & (re > csr[0][:-1])
        re[cut] -= 1
        csr = (csr[0], re, csr[2])
    d32, s32 = R.coef_f32(csr, n)
    nb = int(nat.lib().tsgnn_sag_du_blocks(n, F))
    G = 8 if F <= 32 else 16 if F <= 64 else 32 if F <= 128 else 64
    assert nb == min(256, -(-n // (256 // G)))
    dyb, part, dws, dbs = Out(n, F + 8), Out(nb, F + 4), Out(1, F), Out(1, 1)
    dyb.mat[:, :F] = dyb0.cuda()
    nat.call("sag_du_f32", _i32(csr[0]), _i32(csr[1]) if rowend else None, _i32(csr[2]), d32.cuda(), s32.cuda(), dscore.cuda(),
             _strided(Bt.y, F + 4), F + 4, ws.cuda(), dyb.mat, F + 8, n, F, part.mat, _vec(dws, F), _vec(dbs, 1))
    ref = {}
    for dt_ in (D, S32):
        dinv, self_w = R.coef(csr, n, dt_)
        dt = R.propagate(csr, dinv, self_w, dscore.to(dt_))
        y = Bt.y.to(dt_)
        ref[dt_] = (torch.where(y > 0, dyb0.to(dt_) + dt.unsqueeze(1) * ws.to(dt_), torch.zeros((), dtype=dt_)),
                    (dt.unsqueeze(1) * torch.relu(y)).sum(0), dscore.to(dt_).sum().view(1))
    W.check("sag_du", tag + " du", dyb.mat[:, :F], ref[D][0], ref[S32][0])
    W.check("sag_du", tag + " dws", _vec(dws, F), ref[D][1], ref[S32][1])
    W.check("sag_du", tag + " dbs", _vec(dbs, 1), ref[D][2], ref[S32][2])
    dyb.rest_untouched(tag, _owned(n, F + 8, 0, n, 0, F)); _full(dws, tag); _full(dbs, tag)
    part.rest_untouched(tag + " part", _owned(nb, F + 4, 0, nb, 0, F + 1))


@pytest.mark.parametrize("F", [4, 36, 100, 256])
def test_sag_du(F):
    W = Worst()
    Bt = Batch.make(72, COMP_SIZES, F)
    for rowend in (False, True):
        _du_case(W, "F%d rowend%d" % (F, rowend), Bt, F, rowend)
    W.report()


@pytest.mark.parametrize("F,N", [(4, 8193), (256, 1025)])
def test_sag_du_grid_stride(F, N):
    """one row more than 256 blocks hold (8,193 at G = 8, 1,025 at G = 64): the grid-stride loop under the 256-block cap"""
    W = Worst()
    sizes = [3] * (N // 3) + ([N % 3] if N % 3 else [])
    Bt = Batch.make(73, sizes, F)
    assert Bt.n == N
    assert Bt.n > 256 * (256 // (8 if F == 4 else 64))
    _du_case(W, "F%d N%d" % (F, Bt.n), Bt, F, False)
    W.report()


@pytest.mark.parametrize("nb", [1, 63, 64, 65, 256, 257, 600])
def test_sag_du_reduce(nb):
    W = Worst()
    nat = _nat()
    for F in (4, 100):
        g = torch.Generator().manual_seed(nb + F)
        p = torch.randn(nb, F + 4, generator=g)
        pd, dws, dbs = p.cuda(), Out(1, F), Out(1, 1)
        nat.call("sag_du_reduce_f32", pd, nb, F, _vec(dws, F), _vec(dbs, 1))
        tag = "nb%d F%d" % (nb, F)
        W.check("sag_du_reduce", tag + " dws", _vec(dws, F), p[:, :F].double().sum(0), p[:, :F].sum(0))
        W.check("sag_du_reduce", tag + " dbs", _vec(dbs, 1), p[:, F].double().sum().view(1), p[:, F].sum().view(1))
        _full(dws, tag); _full(dbs, tag)
        after = pd.cpu()
        same = after == p
        assert bool(same[:, F + 1:].all())                  # the three unused columns
        if nb <= 256:
            assert bool(same.all())
        else:                                               # stage one leaves each 64-row chunk's sum in the chunk's first row
            assert bool(same[torch.arange(nb) % 64 != 0].all())
    W.report()


@pytest.mark.parametrize("F", [4, 36, 100, 256])
def test_sag_pool_gather_both_forms(F):
    W = Worst()
    nat = _nat()
    Bt, ws, bs, L64, L32 = _comp_level(F)
    K, n = L64["perm"].numel(), Bt.n
    rp, _, col, _, _ = Bt.dev()
    sc = L64["score"].float()
    for relu_in in (1, 0):
        xp, cnt = Out(K, F + 4), IntOut(K)
        nat.call("sag_pool_gather_f32", _strided(Bt.y, F + 8), F + 8, sc.cuda(), _i32(L64["perm"]), _i32(L64["new_id"]), rp, col, K, F, relu_in,
                 xp.mat, F + 4, cnt.t)
        W.check("sag_pool_gather", "F%d relu%d" % (F, relu_in), xp.mat[:, :F], R.gather(Bt.y, sc, L64["perm"], D, bool(relu_in)),
                R.gather(Bt.y, sc, L64["perm"], S32, bool(relu_in)))
        xp.rest_untouched("gather", _owned(K, F + 4, 0, K, 0, F))
        assert torch.equal(cnt.get("cnt"), L64["cnt"])
    cnt = IntOut(K)                                         # the count-only form (y = xp = NULL)
    nat.call("sag_pool_gather_f32", None, 0, sc.cuda(), _i32(L64["perm"]), _i32(L64["new_id"]), rp, col, K, F, 0, None, 0, cnt.t)
    assert torch.equal(cnt.get("cnt"), L64["cnt"])
    W.report()


@pytest.mark.parametrize("F", [7, 64, 100])
def test_sag_readout(F):
    W = Worst()
    nat = _nat()
    gpn = np.array([0, 1, 4, 9, 150, 151, 410])
    K, B = int(gpn[-1]), len(gpn) - 1
    xp = tie_free(F, K, F)
    xp[9, :3] = 10.0
    xp[10:30, :3] = xp[9, :3]                               # exact ties of the max: the first row wins
    xp[4:9, 1] = 0.0; xp[6, 1] = -0.0
    out64, arg = R.readout(xp.double(), gpn)
    out32, _ = R.readout(xp, gpn)
    out, ai = Out(B, 2 * F + 4), IntOut(B * F)
    xd = _strided(xp, F + 3)
    for acc in (0, 1):
        nat.call("sag_readout_f32", xd, F + 3, _i32(gpn), B, F, acc, out.mat, 2 * F + 4, ai.t)
        W.check("sag_readout", "F%d accumulate%d" % (F, acc), out.mat[:, :2 * F], (1 + acc) * out64, (1 + acc) * out32)
        out.rest_untouched("readout", _owned(B, 2 * F + 4, 0, B, 0, 2 * F))
        assert torch.equal(ai.get("arg").view(B, F), arg)
    W.report()


@pytest.mark.parametrize("coefs", [True, False])
def test_csr_filter_fill(coefs):
    nat = _nat()
    Bt, ws, bs, L64, _ = _comp_level(36, seed=74, hub=180)
    K = L64["perm"].numel()
    rp, _, col, _, _ = Bt.dev()
    rpn, coln = _i32(L64["csr_next"][0]), IntOut(int(col.numel()))
    dn, sn = Out(1, K), Out(1, K)
    nat.call("csr_filter_fill", rp, col, _i32(L64["perm"]), _i32(L64["new_id"]), K, rpn, coln.t, _vec(dn, K) if coefs else None,
             _vec(sn, K) if coefs else None)
    got = coln.get("col_new")
    E = int(L64["csr_next"][0][-1])
    assert int(L64["cnt"].max()) > 64                       # a row longer than the wave that fills it
    assert torch.equal(got[:E], L64["csr_next"][2]) and bool((got[E:] == IPAT).all())
    torch.cuda.synchronize()
    if coefs:
        d32, s32 = R.coef_f32(L64["csr_next"], K)
        assert _same_bits(_vec(dn, K), d32) and _same_bits(_vec(sn, K), s32)
        _full(dn, "dinv_new"); _full(sn, "self_w_new")
    else:
        assert bool((dn.bits == PAT).all()) and bool((sn.bits == PAT).all())


@pytest.mark.parametrize("n", [0, 1, 4095, 4096, 4097])
def test_scan_short(n):
    nat = _nat()
    c = torch.randint(0, 9, (n,), dtype=torch.int32, generator=torch.Generator().manual_seed(n))
    o = IntOut(n + 1)
    nat.call("scan_short_i32", c.cuda() if n else None, n, o.t)
    assert np.array_equal(o.get("scan").numpy(), np.concatenate([[0], np.cumsum(c.numpy())]))


def test_topk_segments_ties_and_a_long_segment():
    nat = _nat()
    sizes = (1, 6, 5000, 40, 257)
    gp = np.concatenate([[0], np.cumsum(sizes)])
    n = int(gp[-1])
    assert 5000 <= int(nat.lib().tsgnn_topk_max_segment())
    sc = tie_free(81, n)
    sc[1:7] = 0.5                                           # a graph of equal scores
    sc[7:5007] = torch.round(sc[7:5007] * 8) / 8 + 0.0      # ~ 60 distinct values among 5,000 nodes: long runs of exact ties (no -0.0)
    sc[5007:5047:2] = 0.0; sc[5008:5047:2] = -0.0
    for ratio in (0.5, 1.0, 0.01):
        gpn = R.pooled_gp(gp, ratio)
        K = int(gpn[-1])
        perm, nid = IntOut(K), IntOut(n)
        nat.call("topk_segments_f32", sc.cuda(), _i32(gp), _i32(gpn), len(sizes), max(sizes), perm.t, nid.t)
        p, q = perm.get("perm"), nid.get("new_id")
        want_p, want_q = R.topk_from(sc, gp, gpn)
        # +0.0 and -0.0 are different keys for the kernel (it orders the bit patterns): leave the graph that mixes them to its own rule
        cut = int(gpn[3])
        assert torch.equal(p[:cut], want_p[:cut]) and torch.equal(p[gpn[4]:], want_p[gpn[4]:])
        assert torch.equal(q[:gp[3]], want_q[:gp[3]]) and torch.equal(q[gp[4]:], want_q[gp[4]:])
        seg = p[gpn[3]: gpn[4]]
        assert bool(((seg >= gp[3]) & (seg < gp[4])).all()) and seg.unique().numel() == seg.numel()
        s = sc[seg]
        assert bool((s[:-1] >= s[1:]).all())


def test_gcn_coef():
    nat = _nat()
    Bt = _grid_batch(4)
    rp, _, col, _, _ = Bt.dev()
    dn, sn = Out(1, Bt.n), Out(1, Bt.n)
    nat.call("gcn_coef_f32", rp, col, Bt.n, _vec(dn, Bt.n), _vec(sn, Bt.n))
    torch.cuda.synchronize()
    d32, s32 = R.coef_f32(Bt.csr, Bt.n)
    assert _same_bits(_vec(dn, Bt.n), d32) and _same_bits(_vec(sn, Bt.n), s32)
    assert int((s32 == 0).sum()) > 0 and float(d32.max()) == 1.0             # rows that hold their own loop; isolated nodes
    _full(dn, "dinv"); _full(sn, "self_w")


def _prop_refs(csr, n, x, relu, bias, w, b0):
    out = {}
    for dt_ in (D, S32):
        dinv, self_w = R.coef(csr, n, dt_)
        xs = torch.relu(x.to(dt_)) if relu else x.to(dt_)
        y = R.propagate(csr, dinv, self_w, xs)
        if bias is not None:
            y = y + bias.to(dt_)
        out[dt_] = (y, y @ w.to(dt_) + b0.to(dt_) if w is not None else None)
    return out


@pytest.mark.parametrize("rowend", [False, True])
@pytest.mark.parametrize("feat,ld", [(36, 40), (100, 100), (70, 71), (3, 5), (8, 9), (1, 1)])
def test_gcn_propagate_small_batch_kernels(feat, ld, rowend):
    """the float4 kernel (36, 100 columns), the generic one (70 columns on an odd leading dimension: two column passes) and its narrow
    branch (<= 8 columns, lanes over the entries): plain, relu + bias, and score mode"""
    W = Worst()
    nat = _nat()
    Bt = Batch.make(91, COMP_SIZES, feat)
    n, csr = Bt.n, Bt.csr
    if rowend:
        re = csr[1].clone()
        cut = (torch.arange(n) % 3 == 1) & (re > csr[0][:-1])
        re[cut] -= 1
        csr = (csr[0], re, csr[2])
    assert int((csr[1] - csr[0][:-1]).max()) >= 70
    d32, s32 = R.coef_f32(csr, n)
    g = torch.Generator().manual_seed(feat)
    bias, w, b0 = torch.randn(feat, generator=g), torch.randn(feat, generator=g), torch.randn(1, generator=g)
    rpd, red, cold = _i32(csr[0]), _i32(csr[1]) if rowend else None, _i32(csr[2])
    xd = _strided(Bt.y, ld)
    name = "gcn_propagate vec4" if feat % 4 == 0 and ld % 4 == 0 else "gcn_propagate generic" if feat > 8 else "gcn_propagate narrow"
    for mode in ("plain", "relu_bias", "score"):
        relu = mode != "plain"
        ldy = ld + 4
        y, t = Out(n, ldy), Out(1, n)
        want_y = mode != "score"
        nat.call("gcn_propagate_re_f32", rpd, red, cold, d32.cuda(), s32.cuda(), xd, ld, int(relu), bias.cuda() if relu else None,
                 w.cuda() if mode == "score" else None, b0.cuda() if mode == "score" else None, y.mat if want_y else None, ldy if want_y else 0,
                 _vec(t, n) if mode == "score" else None, n, feat)
        r = _prop_refs(csr, n, Bt.y, relu, bias if relu else None, w if mode == "score" else None, b0)
        tag = "feat%d ld%d rowend%d %s" % (feat, ld, rowend, mode)
        if want_y:
            W.check(name, tag + " y", y.mat[:, :feat], r[D][0], r[S32][0])
            y.rest_untouched(tag, _owned(n, ldy, 0, n, 0, feat))
            torch.cuda.synchronize()
            assert bool((t.bits == PAT).all())
        else:
            W.check(name, tag + " t", _vec(t, n), r[D][1], r[S32][1])
            _full(t, tag)
            assert bool((y.bits == PAT).all())
    W.report()


@pytest.mark.parametrize("rowend", [False, True])
@pytest.mark.parametrize("feat", [1, 3, 8])
def test_gcn_propagate_affine(feat, rowend):
    """agg = A^ x and y = agg w + bias in one launch (the narrow input of level 0)"""
    W = Worst()
    nat = _nat()
    Bt = Batch.make(92, COMP_SIZES, feat)
    n, csr, n_out = Bt.n, Bt.csr, 70
    if rowend:
        re = csr[1].clone()
        cut = (torch.arange(n) % 3 == 2) & (re > csr[0][:-1])
        re[cut] -= 1
        csr = (csr[0], re, csr[2])
    d32, s32 = R.coef_f32(csr, n)
    g = torch.Generator().manual_seed(feat + 50)
    w, bias = torch.randn(feat, n_out, generator=g), torch.randn(n_out, generator=g)
    for with_bias in (True, False):
        agg, y = Out(n, feat + 3), Out(n, n_out + 2)
        nat.call("gcn_propagate_affine_f32", _i32(csr[0]), _i32(csr[1]) if rowend else None, _i32(csr[2]), d32.cuda(), s32.cuda(),
                 _strided(Bt.y, feat + 1), feat + 1, agg.mat, feat + 3, n, feat, _strided(w, n_out + 1), n_out + 1,
                 bias.cuda() if with_bias else None, y.mat, n_out + 2, n_out)
        tag = "feat%d rowend%d bias%d" % (feat, rowend, with_bias)
        refs = {}
        for dt_ in (D, S32):
            a = _prop_refs(csr, n, Bt.y, False, None, None, None)[dt_][0]
            refs[dt_] = (a, a @ w.to(dt_) + (bias.to(dt_) if with_bias else 0))
        W.check("gcn_propagate_affine", tag + " agg", agg.mat[:, :feat], refs[D][0], refs[S32][0])
        W.check("gcn_propagate_affine", tag + " y", y.mat[:, :n_out], refs[D][1], refs[S32][1])
        agg.rest_untouched(tag, _owned(n, feat + 3, 0, n, 0, feat)); y.rest_untouched(tag, _owned(n, n_out + 2, 0, n, 0, n_out))
    W.report()
