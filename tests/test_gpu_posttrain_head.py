"""The two launches of the fused post-training head (csrc/posttrain_head.hip) through the C ABI against tests/posttrain_ref.py in
float64, at the scheme of tests/fp32_yardstick.py: max|hip - ref64| <= 8 * max(max|cpu32 - ref64|, 2^-23 max|ref64|), the yardstick
being the reference's own fp32 on the CPU.  Checked: out, z, loss, dr and all eight parameter gradients.

Inputs: NaN in the padding behind each readout row (row stride P + 4), ids a permutation that is not the identity into a label table
longer than R, outputs pre-filled with NaN with guard words behind them, an upstream gradient of 0.5, two runs compared bit for bit.
One case has a hidden pre-activation that is exactly 0 in every arithmetic (a zero row of W1 with a zero bias): LeakyReLU's derivative
there is the slope, so that unit's gradients are neither 0 (a derivative of 0 at 0) nor a hundred times larger (a derivative of 1)."""
import numpy as np
import pytest
import torch

import posttrain_ref as PR
from fp32_yardstick import _check

pytestmark = pytest.mark.gpu

SLOPE, UPSTREAM, GUARD, NGUARD = 0.01, 0.5, 777.0, 16
GRID = [(1, 4, 4, 64, 32, 2),            # a single float4
        (1, 36, 6, 64, 32, 2),           # a column block that is not full, E no multiple of 4
        (1, 384, 64, 64, 32, 2),         # the benched shape
        (3, 384, 64, 16, 8, 3),
        (8, 132, 8, 5, 3, 2),            # odd hidden widths
        (1, 2048, 512, 64, 64, 64)]      # every limit
ZERO_CASE = (3, 384, 64, 16, 8, 3)       # the case whose z1[:, 0] is exactly 0


def _inputs(shape, seed=0):
    R, P, E, h1, h2, C = shape
    gen = torch.Generator().manual_seed(1000 + seed)
    rn = lambda *s: torch.randn(*s, generator=gen)
    p = {"map_model.weight": rn(E, P) / P ** 0.5, "map_model.bias": 0.3 * rn(E),
         "map2_model.0.weight": rn(h1, E) / E ** 0.5, "map2_model.0.bias": 0.3 * rn(h1),
         "map2_model.2.weight": rn(h2, h1) / h1 ** 0.5, "map2_model.2.bias": 0.3 * rn(h2),
         "map2_model.4.weight": rn(C, h2) / h2 ** 0.5, "map2_model.4.bias": 0.3 * rn(C)}
    if shape == ZERO_CASE:
        p["map2_model.0.weight"][0] = 0.0
        p["map2_model.0.bias"][0] = 0.0
    r = rn(R, P)
    G = R + 3
    ids = torch.roll(torch.randperm(G, generator=gen)[:R], 1) if R > 1 else torch.tensor([G - 2])
    if R > 1 and ids.tolist() == list(range(R)):
        ids = ids.flip(0)
    labels = torch.randint(0, C, (G,), generator=gen)
    return p, r, ids.int(), labels.int()


def _guarded(n, dev):
    buf = torch.full((n + NGUARD,), float("nan"), dtype=torch.float32, device=dev)
    buf[n:] = GUARD
    return buf


def _run(shape, p, r, ids, labels):
    """both launches on fresh poisoned outputs -> {name: guarded buffer}, shapes"""
    from two_stage_gnn_amd import _native as nat
    R, P, E, h1, h2, C = shape
    dev = torch.device("cuda")
    ld = P + 4
    rp = torch.full((R, ld), float("nan"), dtype=torch.float32, device=dev)
    rp[:, :P] = r.to(dev)
    w = {k: v.to(dev).contiguous() for k, v in p.items()}
    ids_d, lab_d = ids.to(dev), labels.to(dev)
    g = torch.tensor([UPSTREAM], dtype=torch.float32, device=dev)
    sizes = {"out": R * E, "z1": R * h1, "z2": R * h2, "z": R * C, "p": R * C, "loss": 1, "dr": R * P, "dw0": E * P, "db0": E,
             "dw1": h1 * E, "db1": h1, "dw2": h2 * h1, "db2": h2, "dw3": C * h2, "db3": C}
    o = {k: _guarded(n, dev) for k, n in sizes.items()}
    W = [w[k] for k in PR.HEAD_KEYS]
    assert nat.lib().tsgnn_posttrain_head_supported(P, E, h1, h2, C, R) == 1
    nat.call("posttrain_head_fwd_f32", rp, ld, R, P, W[0], W[1], E, W[2], W[3], h1, W[4], W[5], h2, W[6], W[7], C, SLOPE, ids_d, lab_d,
             int(lab_d.numel()), o["out"], o["z1"], o["z2"], o["z"], o["p"], o["loss"])
    nat.call("posttrain_head_bwd_f32", rp, ld, R, P, W[0], E, W[2], h1, W[4], h2, W[6], C, SLOPE, ids_d, lab_d, int(lab_d.numel()),
             o["out"], o["z1"], o["z2"], o["p"], g, o["dr"], P, o["dw0"], o["db0"], o["dw1"], o["db1"], o["dw2"], o["db2"], o["dw3"], o["db3"])
    torch.cuda.synchronize()
    return o, sizes


@pytest.mark.parametrize("shape", GRID, ids=lambda s: "R%d_P%d_E%d_h%d_%d_C%d" % s)
def test_both_launches_against_fp64(shape):
    R, P, E, h1, h2, C = shape
    p, r, ids, labels = _inputs(shape, GRID.index(shape))
    assert ids.tolist() != list(range(R)) and labels.numel() > R
    label = labels[ids.long()]
    ref64 = PR.head_grads(p, r, label, UPSTREAM, torch.float64, SLOPE)
    cpu32 = PR.head_grads(p, r, label, UPSTREAM, torch.float32, SLOPE)
    o, sizes = _run(shape, p, r, ids, labels)
    o2, _ = _run(shape, p, r, ids, labels)
    for k, n in sizes.items():
        assert bool((o[k][n:] == GUARD).all()), "%s: a guard word was overwritten" % k
        assert not bool(torch.isnan(o[k][:n]).any()), "%s: an element was never written" % k
        assert torch.equal(o[k].view(torch.int32), o2[k].view(torch.int32)), "%s: two runs differ" % k
    shapes = {"out": (R, E), "z": (R, C), "loss": (1,), "dr": (R, P), "dw0": (E, P), "db0": (E,), "dw1": (h1, E), "db1": (h1,),
              "dw2": (h2, h1), "db2": (h2,), "dw3": (C, h2), "db3": (C,)}
    names = dict(zip(("dw0", "db0", "dw1", "db1", "dw2", "db2", "dw3", "db3"), PR.HEAD_KEYS))
    for k, shp in shapes.items():
        key = names.get(k, k)
        _check("%s %s" % (shape, k), o[k][:sizes[k]].view(shp), ref64[key], cpu32[key])
    if shape == ZERO_CASE:
        z1 = o["z1"][:R * h1].view(R, h1)
        assert bool((z1[:, 0] == 0).all())                                       # exactly 0: the derivative there is the slope
        gb, gw = ref64["map2_model.0.bias"], ref64["map2_model.0.weight"]
        assert float(gb[0].abs()) > 1e-3 * float(gb.abs().max()) and float(gw[0].abs().max()) > 0     # ... and unit 0 HAS a gradient


def test_validator_refuses_without_a_launch():
    from two_stage_gnn_amd import _native as nat
    shape = (3, 384, 64, 16, 8, 3)
    R, P, E, h1, h2, C = shape
    p, r, ids, labels = _inputs(shape)
    dev = torch.device("cuda")
    rp = r.to(dev).contiguous()
    W = [p[k].to(dev).contiguous() for k in PR.HEAD_KEYS]
    ids_d, lab_d = ids.to(dev), labels.to(dev)
    poison = lambda n: torch.full((n,), float("nan"), dtype=torch.float32, device=dev)
    fo = [poison(R * E), poison(R * h1), poison(R * h2), poison(R * C), poison(R * C), poison(1)]
    bo = [poison(R * P), P, poison(E * P), poison(E), poison(h1 * E), poison(h1), poison(h2 * h1), poison(h2), poison(C * h2), poison(C)]

    def fwd(R=R, P=P, C=C, r_=rp, ld=P):
        return ("posttrain_head_fwd_f32", r_, ld, R, P, W[0], W[1], E, W[2], W[3], h1, W[4], W[5], h2, W[6], W[7], C, SLOPE, ids_d, lab_d,
                int(lab_d.numel())) + tuple(fo)

    def bwd(R=R, P=P, C=C, r_=rp, ld=P):
        return ("posttrain_head_bwd_f32", r_, ld, R, P, W[0], E, W[2], h1, W[4], h2, W[6], C, SLOPE, ids_d, lab_d, int(lab_d.numel()),
                fo[0], fo[1], fo[2], fo[4], None) + tuple(bo)
    lib = nat.lib()
    assert lib.tsgnn_posttrain_head_supported(P, E, h1, h2, C, R) == 1
    for bad in ((6, E, h1, h2, C, R), (2052, E, h1, h2, C, R), (P, 516, h1, h2, C, R), (P, E, 65, h2, C, R), (P, E, h1, 65, C, R),
                (P, E, h1, h2, 1, R), (P, E, h1, h2, 65, R), (P, E, h1, h2, C, 0), (P, E, h1, h2, C, 9)):
        assert lib.tsgnn_posttrain_head_supported(*bad) == 0, bad
    nat.trace = []
    try:
        for make in (fwd, bwd):
            for kw in (dict(R=0), dict(R=9), dict(P=6, ld=8), dict(C=1), dict(r_=None)):
                with pytest.raises(RuntimeError, match="posttrain_head_.* failed"):
                    nat.call(*make(**kw))
        with pytest.raises(RuntimeError, match="posttrain_head_fwd_f32 failed"):
            nat.call(*fwd(r_=rp.view(-1)[1:], ld=P))                          # 4 bytes off a 16-byte boundary
        assert nat.trace == []                                                # nothing was launched
        torch.cuda.synchronize()
        for t in fo + [b for b in bo if isinstance(b, torch.Tensor)]:
            assert bool(torch.isnan(t).all())                                 # the outputs still hold their poison
        nat.call(*fwd())
        nat.call(*bwd())
        assert [t[2] for t in nat.trace] == ["posttrain_head_fwd_kernel<4>", "posttrain_head_bwd_kernel<4>"]
    finally:
        nat.trace = None
    torch.cuda.synchronize()
    assert not any(bool(torch.isnan(t).any()) for t in fo + [b for b in bo if isinstance(b, torch.Tensor)])
