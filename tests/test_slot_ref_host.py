"""tests/slot_ref.py anchored to the oracle the golden vectors pin (oracle/dense_ref.py): its slot batch-norm against
dense_ref.bn_slots on dense layouts, and its autograd-plus-closed-form dU against plain float64 autograd through
F.normalize -> gather -> relu -> bn_slots -> (max readout . dout + y . dxs).  No GPU."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import slot_ref as S
from oracle import dense_ref as R

SIZES = [9, 1, 4, 4, 7, 11, 2]
NMAX = 11


def _rows(sizes, nmax, n_ghost, Fw, seed):
    L = S.Layout(sizes, nmax, n_ghost)
    u = torch.randn(L.rows, Fw, dtype=torch.float64, generator=torch.Generator().manual_seed(seed))
    return L, u


def _dense_of(rows, L, fill):
    """[B, nmax, F] with the real rows in place and ``fill`` (a [nmax, F] tensor) in the padded slots"""
    x = fill[None].repeat(L.B, 1, 1)
    x[L.real] = rows[L.idx[L.real]]
    return x


@pytest.mark.parametrize("relu", [False, True])
def test_slot_bn_full_graphs_is_dense_bn(relu):
    """every size equal to nmax, no ghost rows: the rows ARE the dense tensor"""
    L, v = _rows([5] * 6, 5, 0, 12, 1)
    mean, rstd, y = S.slot_bn(v, L, relu=relu)
    x = v.reshape(6, 5, 12)
    x = torch.relu(x) if relu else x
    assert (y.reshape(6, 5, 12) - R.bn_slots(x)).abs().max().item() <= 1e-12
    assert (mean - x.mean(dim=(0, 2))).abs().max().item() <= 1e-12
    assert (rstd - 1.0 / torch.sqrt(x.var(dim=(0, 2), unbiased=False) + R.BN_EPS)).abs().max().item() <= 1e-12


@pytest.mark.parametrize("relu", [False, True])
def test_slot_bn_ragged_ghost_rows_are_the_padded_rows(relu):
    """ragged sizes, padded rows zero before the first layer: a ghost row stands for every padded row of its slot"""
    L, v = _rows(SIZES, NMAX, NMAX, 8, 2)
    v[L.n_real:] = 0.0
    mean, rstd, y = S.slot_bn(v, L, relu=relu)
    x = _dense_of(v, L, torch.zeros(NMAX, 8, dtype=torch.float64))
    yd = R.bn_slots(torch.relu(x) if relu else x)
    assert (y[L.idx[L.real]] - yd[L.real]).abs().max().item() <= 1e-12
    gb, gn = torch.nonzero(L.ghost, as_tuple=True)
    assert len(gb) > 0
    assert (y[L.n_real + gn] - yd[gb, gn]).abs().max().item() <= 1e-12
    for r in L.unused_ghost_rows:                       # slot 0: every graph has it
        assert r == L.n_real and (y[r] == 0).all()


def test_slot_bn_padded_layout_counts_present_rows_only():
    """no ghost rows: the statistics of slot n run over the slot_count[n] graphs that have it; a slot nobody has: mean 0, rstd 1/sqrt(eps)"""
    sizes = [9, 1, 4, 4, 7, 2]
    L, v = _rows(sizes, NMAX, 0, 8, 3)
    mean, rstd, y = S.slot_bn(v, L, relu=True)
    for n in range(NMAX):
        rows = [int(L.graph_ptr[b]) + n for b in range(L.B) if sizes[b] > n]
        if not rows:
            assert mean[n].item() == 0.0 and abs(rstd[n].item() - 1.0 / np.sqrt(1e-5)) <= 1e-9
            continue
        h = torch.relu(v[rows])
        assert abs(mean[n].item() - h.mean().item()) <= 1e-12
        assert (y[rows] - (h - h.mean()) / torch.sqrt(h.var(unbiased=False) + 1e-5)).abs().max().item() <= 1e-12


@pytest.mark.parametrize("n_ghost", [NMAX, 0])
def test_post_bwd_is_plain_autograd(n_ghost):
    """du of slot_ref.slot_post_bwd == d loss / d u of the chain written out with torch alone (random input: no ties)"""
    sizes = SIZES if n_ghost else [NMAX] * 5          # bn_slots takes a dense tensor: the padded layout must be full
    Fw = 8
    L, u0 = _rows(sizes, NMAX, n_ghost, Fw, 4)
    gen = torch.Generator().manual_seed(5)
    dout = torch.randn(L.B, Fw, dtype=torch.float64, generator=gen)
    dxs = torch.randn(L.rows, Fw, dtype=torch.float64, generator=gen)
    dxs[L.n_real:] = float("nan")                     # nothing aggregates from a ghost row
    u = u0.clone().requires_grad_(True)
    v = F.normalize(u, p=2, dim=1, eps=1e-12)
    y = R.bn_slots(torch.relu(v[L.idx]))              # every candidate is present
    out = y.max(dim=1)[0]
    loss = (out * dout).sum() + (y[L.real] * dxs[L.idx[L.real]]).sum()
    du_auto, = torch.autograd.grad(loss, u)
    vd = v.detach()
    rinv = 1.0 / u0.norm(dim=1)
    out_ref, arg = S.readout_max(S.slot_bn(vd, L)[2], L)
    assert (out_ref - out.detach()).abs().max().item() <= 1e-12
    du = S.slot_post_bwd(vd, rinv, L, dxs=dxs, dout=dout, arg=arg)
    assert (du - du_auto).abs().max().item() <= 1e-10 * du_auto.abs().max().item()
    for r in L.unused_ghost_rows:
        assert (du[r] == 0).all()


def test_readout_max_ties_and_empty_graph():
    L = S.Layout([3, 0, 2], 4, 0)
    x = torch.tensor([[1.0, 5.0], [1.0, 7.0], [0.5, 7.0], [2.0, -3.0], [2.0, -4.0]], dtype=torch.float64)
    out, arg = S.readout_max(x, L)
    assert out.tolist() == [[1.0, 7.0], [0.0, 0.0], [2.0, -3.0]]
    assert arg.tolist() == [[0, 1], [-1, -1], [3, 3]]
    Lg = S.Layout([1, 2], 2, 2)                       # rows: 0 | 1 2 | ghosts 3 4; graph 0's slot 1 is ghost row 4
    xg = torch.tensor([[4.0, 1.0], [0.0, 0.0], [0.0, 0.0], [9.0, 9.0], [4.0, 2.0]], dtype=torch.float64)
    out, arg = S.readout_max(xg, Lg)
    assert arg.tolist() == [[0, 4], [1, 1]] and out.tolist() == [[4.0, 2.0], [0.0, 0.0]]


def test_readout_l2_bwd_is_post_bwd_without_bn():
    L, u = _rows(SIZES, NMAX, NMAX, 8, 6)
    v = F.normalize(u, dim=1)
    rinv = 1.0 / u.norm(dim=1)
    _, arg = S.readout_max(v, L)
    dout = torch.randn(L.B, 8, dtype=torch.float64, generator=torch.Generator().manual_seed(7))
    a = S.slot_post_bwd(v, rinv, L, dout=dout, arg=arg, relu=False, bn=False)
    b = S.readout_l2_bwd(v, rinv, dout, arg, L.row_graph(), NMAX)
    assert (a - b).abs().max().item() <= 1e-13
