"""The four launches of csrc/posttrain_cls.hip (the mlp3 + nll head of the SAGPool post-training step, the mlp2 + cross-entropy head of
EigenGCN's) through the C ABI against tests/posttrain_cls_ref.py in float64, at the scheme of tests/fp32_yardstick.py:
max|hip - ref64| <= 8 * max(max|cpu32 - ref64|, 2^-23 max|ref64|), the yardstick being the reference's own fp32 on the CPU.

Every output sits in a guarded buffer (tests/guard_buf.py: every word one NaN pattern, guard words behind it), every cell is
launched twice and compared bit for bit.  Each cell runs in two variants: (upstream gradient NULL, ids[0] past the label table: the
clamp takes the table's last entry, whose label is the LAST class) and (upstream 0.5, ids[0] in range with the FIRST class; with
R > 1, ids[1] negative: clamped to entry 0).  The mlp2 variants also differ in biases and dr (present / NULL)."""
import numpy as np
import pytest
import torch

import posttrain_cls_ref as CR
from fp32_yardstick import _check
from guard_buf import Out

pytestmark = pytest.mark.gpu

MLP3_CELLS = [(1, 4, 4, 4, 2),                   # smallest
              (1, 64, 32, 16, 8),                # the small6 widths
              (1, 256, 128, 64, 64),             # the reference's defaults
              (3, 260, 132, 68, 65),             # one past a wave in C, partial 16-byte tiles everywhere
              (8, 2048, 1024, 512, 512)]         # the envelope's corner
WIDE_LDR = (3, 260, 132, 68, 65)                 # the cell whose rows are 8 floats (of NaN) wider than D0
MLP2_CELLS = [(1, 4, 1, 2),                      # smallest
              (3, 36, 7, 3),                     # odd widths
              (1, 1152, 50, 64),                 # the README's EigenGCN configuration; H % 4 != 0
              (2, 2048, 512, 512)]               # the envelope's corner
VARIANTS = ("last_class_clamped_id", "first_class_half_upstream")
SEED = 0x5EED0123456789


def _ids_labels(R, C, variant, gen):
    """-> (ids [R] int32 as the launch gets them, label table int32 [R + 3], the labels [R] the clamped ids select)"""
    G = R + 3
    labels = torch.randint(0, C, (G,), generator=gen)
    labels[0], labels[G - 1] = 0, C - 1
    ids = torch.randint(1, G - 1, (R,), generator=gen)
    if variant == VARIANTS[0]:
        ids[0] = G + 5
    else:
        ids[0] = 0
        if R > 1:
            ids[1] = -3
    y = labels[ids.clamp(0, G - 1)]
    return ids.int(), labels.int(), y


def _rows(r, ld):
    """the readout rows on the device at row stride ld, NaN in the padding"""
    rp = torch.full((r.size(0), ld), float("nan"), dtype=torch.float32, device="cuda")
    rp[:, :r.size(1)] = r.cuda()
    return rp


def _outs(shapes):
    return {k: Out(s[0], s[1]) for k, s in shapes.items()}


def _all_written_guards_whole(o):
    for k, b in o.items():
        b.rest_untouched(k, torch.ones(b.rows, b.ld, dtype=torch.bool))
        assert not bool(torch.isnan(b.mat).any()), "%s: an element was never written" % k


def _same_bits(o, o2):
    for k in o:
        assert torch.equal(o[k].bits, o2[k].bits), "%s: two launches differ" % k


# ------------------------------------------------------------------------------------------------ mlp3 + nll
def _mlp3_inputs(cell, variant):
    R, D0, D1, D2, C = cell
    gen = torch.Generator().manual_seed(31 * MLP3_CELLS.index(cell) + VARIANTS.index(variant))
    rn = lambda *s: torch.randn(*s, generator=gen)
    p = {"w1": rn(D1, D0) / D0 ** 0.5, "b1": 0.3 * rn(D1), "w2": rn(D2, D1) / D1 ** 0.5, "b2": 0.3 * rn(D2),
         "w3": rn(C, D2) / D2 ** 0.5, "b3": 0.3 * rn(C)}
    return p, rn(R, D0), _ids_labels(R, C, variant, gen)


def _mlp3_run(cell, p, r, ids, labels, upstream, drop_p=0.0, state=None, dr=True):
    from two_stage_gnn_amd import _native as nat
    R, D0, D1, D2, C = cell
    ld = D0 + 8 if cell == WIDE_LDR else D0
    rp = _rows(r, ld)
    w = {k: v.cuda().contiguous() for k, v in p.items()}
    ids_d, lab_d = ids.cuda(), labels.cuda()
    g = None if upstream is None else torch.tensor([upstream], dtype=torch.float32, device="cuda")
    used = torch.full((1,), -1, dtype=torch.int64, device="cuda")
    o = _outs({"a1": (R, D1), "a2": (R, D2), "logp": (R, C), "loss": (1, 1), "dr": (R, D0), "dw1": (D1, D0), "db1": (1, D1),
               "dw2": (D2, D1), "db2": (1, D2), "dw3": (C, D2), "db3": (1, C)})
    assert nat.lib().tsgnn_posttrain_mlp3_nll_supported(D0, D1, D2, C, R) == 1
    nat.call("posttrain_mlp3_nll_fwd_f32", rp, ld, R, w["w1"], w["b1"], float(drop_p), SEED, state, used if drop_p > 0 else None,
             w["w2"], w["b2"], w["w3"], w["b3"], D0, D1, D2, C, ids_d, lab_d, int(lab_d.numel()), o["a1"].mat, o["a2"].mat,
             o["logp"].mat, o["loss"].mat)
    fwd_kernel = nat.last_kernel()
    nat.call("posttrain_mlp3_nll_bwd_f32", rp, ld, R, w["w1"], w["w2"], w["w3"], D0, D1, D2, C, 1.0 / (1.0 - drop_p), ids_d, lab_d,
             int(lab_d.numel()), o["a1"].mat, o["a2"].mat, o["logp"].mat, g, o["dr"].mat if dr else None, D0, o["dw1"].mat,
             o["db1"].mat, o["dw2"].mat, o["db2"].mat, o["dw3"].mat, o["db3"].mat)
    torch.cuda.synchronize()
    rt = 1 if R <= 1 else 2 if R <= 2 else 4 if R <= 4 else 8
    assert fwd_kernel == "posttrain_mlp3_nll_fwd_kernel<%d>" % rt and nat.last_kernel() == "posttrain_mlp3_nll_bwd_kernel<%d>" % rt
    if not dr:
        assert bool((o["dr"].bits == o["dr"].bits[0]).all())            # a NULL dr: nothing was written for it
        del o["dr"]
    return o, used


def _mlp3_compare(cell, o, ref64, cpu32):
    for k, b in o.items():
        shape = ref64[k].shape
        _check("%s %s" % (cell, k), b.mat.view(shape), ref64[k], cpu32[k])


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("cell", MLP3_CELLS, ids=lambda s: "R%d_%d_%d_%d_C%d" % s)
def test_mlp3_nll_against_fp64(cell, variant):
    R, D0, D1, D2, C = cell
    p, r, (ids, labels, y) = _mlp3_inputs(cell, variant)
    upstream = None if variant == VARIANTS[0] else 0.5
    assert int(y[0]) == (C - 1 if variant == VARIANTS[0] else 0)
    o, _ = _mlp3_run(cell, p, r, ids, labels, upstream)
    o2, _ = _mlp3_run(cell, p, r, ids, labels, upstream)
    _all_written_guards_whole(o)
    _same_bits(o, o2)
    up = 1.0 if upstream is None else upstream
    _mlp3_compare(cell, o, CR.mlp3_nll(p, r, y, up, torch.float64), CR.mlp3_nll(p, r, y, up, torch.float32))


@pytest.mark.parametrize("cell", [(1, 256, 128, 64, 64), (3, 260, 132, 68, 65)], ids=lambda s: "R%d_%d_%d_%d_C%d" % s)
def test_mlp3_nll_dropout_mask_is_the_library_s(cell):
    """p = 0.5: the mask of the launch is what tsgnn_mlp3_dropout_mask_f32 regenerates from used[0] for B = R, a1 is zero exactly where
    it drops, the launch advances the counter by one, and the same counter gives the same bits"""
    from two_stage_gnn_amd import _native as nat
    R, D0, D1, D2, C = cell
    p, r, (ids, labels, y) = _mlp3_inputs(cell, VARIANTS[1])
    state = torch.zeros(2, dtype=torch.int64, device="cuda")
    o, used = _mlp3_run(cell, p, r, ids, labels, 0.5, drop_p=0.5, state=state, dr=False)
    assert int(used[0]) == 0 and state.tolist() == [1, 0]
    o2, used2 = _mlp3_run(cell, p, r, ids, labels, 0.5, drop_p=0.5, state=state, dr=False)
    assert int(used2[0]) - int(used[0]) == 1 and state.tolist() == [2, 0]
    masks = []
    for u in (used, used2):
        m = torch.empty(R, D1, dtype=torch.float32, device="cuda")
        nat.call("mlp3_dropout_mask_f32", 0.5, SEED, int(u[0]), R, D1, m)
        masks.append(m.cpu())
    assert not torch.equal(masks[0], masks[1]) and 0.3 < float(masks[0].mean()) < 0.7 and set(masks[0].unique().tolist()) <= {0.0, 1.0}
    for b, m in zip((o, o2), masks):
        _all_written_guards_whole(b)
        assert bool((b["a1"].mat.cpu()[m == 0] == 0).all())
        ref64 = CR.mlp3_nll(p, r, y, 0.5, torch.float64, mask=m, keep_scale=2.0)
        assert bool(((b["a1"].mat.cpu() == 0) == (ref64["a1"] == 0)).all())          # ... and nowhere else but at a dead ReLU
        del ref64["dr"]
        cpu32 = CR.mlp3_nll(p, r, y, 0.5, torch.float32, mask=m, keep_scale=2.0)
        _mlp3_compare(cell, b, ref64, cpu32)
    state.zero_()
    o3, used3 = _mlp3_run(cell, p, r, ids, labels, 0.5, drop_p=0.5, state=state, dr=False)
    assert int(used3[0]) == 0
    _same_bits(o, o3)


# ------------------------------------------------------------------------------------------------ mlp2 + cross-entropy
def _mlp2_inputs(cell, variant):
    R, D, H, C = cell
    gen = torch.Generator().manual_seed(77 * MLP2_CELLS.index(cell) + VARIANTS.index(variant))
    rn = lambda *s: torch.randn(*s, generator=gen)
    bias = variant == VARIANTS[0]
    p = {"w1": rn(H, D) / D ** 0.5, "b1": 0.3 * rn(H) if bias else None, "w2": rn(C, H) / H ** 0.5, "b2": 0.3 * rn(C) if bias else None}
    return p, rn(R, D), _ids_labels(R, C, variant, gen)


def _mlp2_run(cell, p, r, ids, labels, upstream, dr):
    from two_stage_gnn_amd import _native as nat
    R, D, H, C = cell
    ld = D + 4
    rp = _rows(r, ld)
    w = {k: (v.cuda().contiguous() if v is not None else None) for k, v in p.items()}
    ids_d, lab_d = ids.cuda(), labels.cuda()
    g = None if upstream is None else torch.tensor([upstream], dtype=torch.float32, device="cuda")
    o = _outs({"h": (R, H), "z": (R, C), "p": (R, C), "loss": (1, 1), "dr": (R, D), "dw1": (H, D), "db1": (1, H), "dw2": (C, H),
               "db2": (1, C)})
    assert nat.lib().tsgnn_posttrain_mlp2_ce_supported(D, H, C, R) == 1
    nat.call("posttrain_mlp2_ce_fwd_f32", rp, ld, R, w["w1"], w["b1"], w["w2"], w["b2"], D, H, C, ids_d, lab_d, int(lab_d.numel()),
             o["h"].mat, o["z"].mat, o["p"].mat, o["loss"].mat)
    fwd_kernel = nat.last_kernel()
    has_b = p["b1"] is not None
    nat.call("posttrain_mlp2_ce_bwd_f32", rp, ld, R, w["w1"], w["w2"], D, H, C, ids_d, lab_d, int(lab_d.numel()), o["h"].mat, o["p"].mat,
             g, o["dr"].mat if dr else None, D, o["dw1"].mat, o["db1"].mat if has_b else None, o["dw2"].mat,
             o["db2"].mat if has_b else None)
    torch.cuda.synchronize()
    rt = 1 if R <= 1 else 2 if R <= 2 else 4 if R <= 4 else 8
    assert fwd_kernel == "posttrain_mlp2_ce_fwd_kernel<%d>" % rt and nat.last_kernel() == "posttrain_mlp2_ce_bwd_kernel<%d>" % rt
    for k in [] if dr else ["dr"]:
        assert bool((o[k].bits == o[k].bits[0]).all())                  # a NULL output: nothing was written for it
        del o[k]
    if not has_b:
        for k in ("db1", "db2"):
            assert bool((o[k].bits == o[k].bits[0]).all())
            del o[k]
    return o


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("cell", MLP2_CELLS, ids=lambda s: "R%d_D%d_H%d_C%d" % s)
def test_mlp2_ce_against_fp64(cell, variant):
    R, D, H, C = cell
    p, r, (ids, labels, y) = _mlp2_inputs(cell, variant)
    first = variant == VARIANTS[0]                                       # biases, dr, NULL upstream | no biases, NULL dr, 0.5
    upstream = None if first else 0.5
    assert int(y[0]) == (C - 1 if first else 0)
    o = _mlp2_run(cell, p, r, ids, labels, upstream, dr=first)
    o2 = _mlp2_run(cell, p, r, ids, labels, upstream, dr=first)
    _all_written_guards_whole(o)
    _same_bits(o, o2)
    up = 1.0 if upstream is None else upstream
    ref64, cpu32 = CR.mlp2_ce(p, r, y, up, torch.float64), CR.mlp2_ce(p, r, y, up, torch.float32)
    for k, b in o.items():
        _check("%s %s" % (cell, k), b.mat.view(ref64[k].shape), ref64[k], cpu32[k])
