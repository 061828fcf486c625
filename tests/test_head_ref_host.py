"""tests/head_ref.py — the reference test_gpu_head_kernels.py holds csrc/head.hip to — against float64 autograd, torch.max and
slot_ref.readout_max, so that it cannot be wrong in the same way as the kernels.  No GPU."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F_

import head_ref as H
import slot_ref as S
from guard_buf import _du_ref

D = torch.float64


def _operands(B, P, E, C, seed):
    gen = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=gen, dtype=D)
    return r(B, P), r(E, P), r(E), r(C, E), r(C), torch.randint(0, C, (B,), generator=gen), r(B, E)


@pytest.mark.parametrize("with_dvec", [True, False], ids=["dvec", "nodvec"])
@pytest.mark.parametrize("bias", [True, False], ids=["bias", "nobias"])
@pytest.mark.parametrize("B,P,E,C", [(1, 4, 1, 1), (3, 8, 5, 2), (9, 12, 10, 6)])
def test_head_against_autograd(B, P, E, C, bias, with_dvec):
    """head_fwd / softmax_ce / head_bwd == Linear -> Linear -> F.cross_entropy under float64 autograd; dvec is the cotangent of a
    second use of vec (loss + sum(vec * dvec))"""
    out, w1, b1, w2, b2, label, dvec = _operands(B, P, E, C, B * 100 + P)
    leaves = [t.clone().requires_grad_(True) for t in (out, w1, b1, w2, b2)]
    o, a1, c1, a2, c2 = leaves
    vec = F_.linear(o, a1, c1 if bias else None)
    y = F_.linear(vec, a2, c2 if bias else None)
    loss = F_.cross_entropy(y, label)
    total = loss + ((vec * dvec).sum() if with_dvec else 0.0)
    g = torch.autograd.grad(total, [o, a1, a2] + ([c1, c2] if bias else []))
    vec_r, y_r = H.head_fwd(out, w1, b1 if bias else None, w2, b2 if bias else None)
    assert torch.allclose(vec_r, vec.detach(), rtol=1e-12, atol=1e-12) and torch.allclose(y_r, y.detach(), rtol=1e-12, atol=1e-12)
    loss_r, dy = H.softmax_ce(y_r, label)
    assert abs(loss_r.item() - loss.item()) <= 1e-12 * max(1.0, abs(loss.item()))
    yl = y.detach().clone().requires_grad_(True)
    assert torch.allclose(dy, torch.autograd.grad(F_.cross_entropy(yl, label), yl)[0], rtol=1e-12, atol=1e-14)
    dout, dw1, db1, dw2, db2, parts = H.head_bwd(out, vec_r, dy, dvec if with_dvec else None, w1, w2, has_b1=bias, has_b2=bias)
    got = [dout, dw1, dw2] + ([db1, db2] if bias else [])
    assert (db1 is None) == (not bias) and (db2 is None) == (not bias)
    for a, b in zip(got, g):
        assert torch.allclose(a, b, rtol=1e-11, atol=1e-12)
    # normparts: ceil(E / 4) + 1 blocks that sum to |all gradients|^2; block jb = rows 4jb .. 4jb+3 of dw1 (+ db1), the last = dw2 (+ db2)
    assert parts.shape == ((E + 3) // 4 + 1,)
    tot = sum((t ** 2).sum() for t in got[1:])
    assert abs(parts.sum().item() - tot.item()) <= 1e-12 * tot.item()
    assert abs(parts[-1].item() - ((dw2 ** 2).sum() + ((db2 ** 2).sum() if bias else 0.0)).item()) <= 1e-12 * tot.item()
    j = (E + 3) // 4 - 1
    last = (dw1[4 * j:] ** 2).sum() + ((db1[4 * j:] ** 2).sum() if bias else 0.0)
    assert abs(parts[j].item() - last.item()) <= 1e-12 * tot.item()


def test_head_fwd_orders_agree():
    """the pairwise summation order of head_fwd (the second float32 sample of the forward yardstick) is the same function"""
    out, w1, b1, w2, b2, _, _ = _operands(3, 517, 7, 5, 11)
    a, b = H.head_fwd(out, w1, b1, w2, b2), H.head_fwd(out, w1, b1, w2, b2, order="tree")
    assert torch.allclose(a[0], b[0], rtol=1e-12, atol=1e-12) and torch.allclose(a[1], b[1], rtol=1e-12, atol=1e-12)
    t = torch.arange(1.0, 8.0, dtype=D)
    assert float(H._tree_sum(t)) == 28.0 and float(H._tree_sum(t[:1])) == 1.0


def test_softmax_ce_large_logits():
    """rows of +/-80 (exp overflows fp32 without the max subtraction) stay finite in the float32 run of the reference"""
    y = torch.tensor([[80.0, -80.0, 0.0], [-80.0, -80.0, -80.0], [1.0, 2.0, 3.0]])
    label = torch.tensor([1, 2, 0])
    l64, d64 = H.softmax_ce(y, label)
    l32, d32 = H.softmax_ce(y, label, dtype=torch.float32)
    assert torch.isfinite(d32).all() and torch.isfinite(l32)
    assert abs(l64.item() - F_.cross_entropy(y.double(), label).item()) < 1e-12
    assert abs(l32.item() - l64.item()) < 1e-4 and (d32.double() - d64).abs().max() < 1e-6


def test_ordered_bits_follow_float_order():
    v = np.array([-np.inf, -3.5, -1e-30, 0.0, 1e-30, 2.0, np.inf], dtype=np.float32)
    o = H._f32_ordered(v).astype(np.int64)
    assert (np.diff(o) > 0).all() and (o > 0).all()
    assert np.array_equal(H._ordered_f32(H._f32_ordered(v)), v)
    # the documented word: value bits above, 0xFFFFFFFF - row below; no candidate -> 0
    w = H.encode_packed(np.array([2.0, 2.0, -1.0], dtype=np.float32), np.array([7, 3, -1]))
    assert int(w[0]) == ((0x80000000 | 0x40000000) << 32) | (0xFFFFFFFF - 7) and w[1] > w[0] and int(w[2]) == 0


@pytest.mark.parametrize("ghosts", [True, False], ids=["ghost", "noghost"])
@pytest.mark.parametrize("kind", ["random", "ties", "allneg"])
def test_packed_roundtrip_against_readout_max(kind, ghosts):
    """max of the encoded words over a graph's candidates, decoded == slot_ref.readout_max: ties (the smallest row, a real row before a
    ghost row), negative maxima, a graph without candidates (out 0, arg -1)"""
    nmax, Lyr, Fh, Fl, B = 6, 3, 8, 4, 5
    sizes = [6, 1, 3, 0 if not ghosts else 2, 5]
    L = S.Layout(sizes, nmax, nmax if ghosts else 0)
    widths = [Fh] * (Lyr - 1) + [Fl]
    xs = []
    for l, w in enumerate(widths):
        x = torch.randn(L.rows, w, generator=torch.Generator().manual_seed(10 * l + len(kind)))
        if kind == "allneg":
            x = -x.abs() - 0.125
        if kind == "ties":
            for b in range(B):
                r0 = int(L.graph_ptr[b])
                if sizes[b] >= 2:
                    x[r0 + 1, 0] = x[r0, 0] = 50.0
                if sizes[b] >= 3:
                    x[r0 + 2, 1] = x[r0 + 1, 1] = 50.0
                if ghosts and 1 <= sizes[b] < nmax:
                    x[r0 + sizes[b] - 1, 2] = x[L.n_real + sizes[b], 2] = 60.0
        xs.append(x)
    packed = H.pack_layers([H.packed_max(x, L) for x in xs])
    assert packed.numel() == B * ((Lyr - 1) * Fh + Fl)
    out, arg = H.decode_packed(packed, B, Lyr, Fh, Fl)
    off = 0
    for l, (x, w) in enumerate(zip(xs, widths)):
        o_ref, a_ref = S.readout_max(x, L)
        assert torch.equal(out[:, l * Fh:l * Fh + w], o_ref), "layer %d out" % l
        assert torch.equal(arg[off:off + B * w].reshape(B, w), a_ref), "layer %d arg" % l
        off += B * w
        if kind == "ties":
            assert int(a_ref[0, 0]) == 0 and int(a_ref[0, 1]) == 1
            if ghosts:
                assert int(a_ref[1, 2]) == int(L.graph_ptr[1])          # the real row, not ghost row n_real + 1
        if not ghosts:
            assert (a_ref[3] == -1).all() and (o_ref[3] == 0).all()


@pytest.mark.parametrize("B,N,F", [(1, 1, 4), (3, 17, 8), (2, 64, 4)])
def test_ro_tail_against_torch_max(B, N, F):
    gen = torch.Generator().manual_seed(B + N)
    z = torch.randn(B * N + 3, F, generator=gen, dtype=D)
    if N > 2:
        z[1, 0] = z[2, 0] = 9.0                                        # a tie: row 1 wins
        z[:N, 1] = -z[:N, 1].abs() - 1.0                               # an all-negative column
    out, arg = H.ro_tail(z, B, N)
    d = z[:B * N].reshape(B, N, F)
    assert torch.equal(out, d.max(dim=1)[0])
    assert torch.equal(z[arg.long(), torch.arange(F)[None, :]], out)
    assert (arg.long() // N == torch.arange(B)[:, None]).all()
    if N > 2:
        assert int(arg[0, 0]) == 1 and float(out[0, 1]) < 0
    # backward against autograd of the max itself (no ties in the differentiated columns' winners: autograd splits nothing here)
    zz = torch.randn(B * N, F, generator=gen, dtype=D).requires_grad_(True)
    dseg = torch.randn(B, F, generator=gen, dtype=D)
    o2, a2 = H.ro_tail(zz.detach(), B, N)
    (zz.reshape(B, N, F).max(dim=1)[0] * dseg).sum().backward()
    assert torch.equal(H.ro_tail_bwd(dseg, a2, B, N), zz.grad)
    a3 = a2.clone()
    a3[0, 0] = -1
    assert (H.ro_tail_bwd(dseg, a3, B, N)[:N, 0] == 0).all()


def test_du_ref_against_readout_l2_bwd():
    """guard_buf._du_ref (graph b's ghost contribution at row n_real + b) against slot_ref.readout_l2_bwd (one row per ghost slot): real
    rows equal, the contributions of the graphs of size n sum to ghost row n_real + n, a clamped row takes no projection, padding rows 0"""
    sizes, nmax, F, off = [4, 1, 4, 0, 6], 6, 8, 4
    B, pad = len(sizes), 3
    L = S.Layout(sizes, nmax, nmax, n_real=sum(sizes) + pad)
    gen = torch.Generator().manual_seed(5)
    u = torch.randn(L.rows, F, generator=gen, dtype=D)
    u[1] = u[1].abs() * (0.5e-12 / u[1].norm())
    nrm = u.norm(dim=1, keepdim=True).clamp(min=1e-12)
    v, rinv = (u / nrm).float(), (1.0 / nrm[:, 0]).float()
    dout = torch.randn(B, off + F, generator=gen)
    sz, gp = torch.tensor(sizes), torch.as_tensor(L.graph_ptr)
    arg = gp[:-1, None] + (torch.rand(B, F, generator=gen) * sz[:, None]).long()
    arg[:, 0] = L.n_real + sz                                          # every graph below nmax wins its ghost row in column 0
    arg[4, 0] = -1                                                     # (graph 4 fills every slot)
    arg[3, 1:] = -1                                                    # the empty graph has no real row
    arg[0, 1] = 1
    arg = arg.to(torch.int32)
    ours = _du_ref(v, rinv, arg, dout, off, gp, L.n_real, nmax, D)
    ref = S.readout_l2_bwd(v, rinv, dout[:, off:], arg, L.row_graph(), nmax)
    assert torch.allclose(ours[:L.n_real], ref[:L.n_real], rtol=1e-12, atol=1e-14)
    assert (ours[L.pad_rows] == 0).all()
    for n in range(nmax):
        tot = sum((ours[L.n_real + b] for b in range(B) if sizes[b] == n), torch.zeros(F, dtype=D))
        assert torch.allclose(tot, ref[L.n_real + n], rtol=1e-12, atol=1e-14), n
    g1 = torch.where(arg[0] == 1, dout[0, off:].double(), torch.zeros(F, dtype=D))
    assert torch.equal(ours[1], rinv[1].double() * g1) and float(g1.abs().max()) > 0
