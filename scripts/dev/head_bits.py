"""Bits of the twelve head entry points (fwd and bwd of triplet_embed, mlp2_triplet, mlp3_triplet, posttrain_mlp3_nll,
posttrain_mlp2_ce, posttrain_head) of two builds of the library on the same seeded inputs.

    TSGNN_LIB_PATH=<the other build's libtsgnn_hip.so> python scripts/dev/head_bits.py run parent.npz     (a process of its own)
    python scripts/dev/head_bits.py run tree.npz                                                            (a process of its own)
    python scripts/dev/head_bits.py cmp parent.npz tree.npz                                                 (no GPU)

`cmp` prints np.array_equal per tensor (bit patterns); for the weight-gradient outer products of the three triplet backwards, whose
fold order  fmaf(g0, r0, fmaf(g1, r1, g2 r2))  is not the post-training heads' left fold from 0, also the largest difference in units
of 2^-23 max|parent|.  Exit status 1 when any tensor differs."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
OUTER_PRODUCTS = ("embed/dw1", "mlp2t/dw1", "mlp2t/dw2", "mlp3t/dw1", "mlp3t/dw2", "mlp3t/dw3")
EPS, SEED = 1e-6, 0x5EED0123456789


def run(path):
    import torch
    from two_stage_gnn_amd import _native as nat
    import test_gpu_posttrain_cls as PC
    import test_gpu_triplet_tail_kernels as TT
    res = {}
    gen = torch.Generator().manual_seed(27)
    rn = lambda *s: torch.randn(*s, generator=gen).cuda()
    new = lambda *s: torch.full(s, float("nan"), dtype=torch.float32, device="cuda")

    def keep(fam, cell, **o):
        for k, v in o.items():
            res["%s/%s/%s" % (fam, "x".join(map(str, cell)), k)] = v.cpu().numpy().view(np.uint32)

    def layers(dims):
        w = []
        for k, n in zip(dims[:-1], dims[1:]):
            w += [rn(n, k) / k ** 0.5, 0.3 * rn(n)]
        return w

    def labels(R, C):
        return torch.randint(0, R + 3, (R,), generator=gen).int().cuda(), torch.randint(0, C, (R + 3,), generator=gen).int().cuda()

    for cell in TT.EMBED_CELLS:
        D, E = cell
        r, (w, b), g = rn(3, D), layers(cell), [rn(1), rn(1), rn(E), rn(E), rn(E)]
        e, d, dr, dw, db = new(3, E), new(2), new(3, D), new(E, D), new(E)
        nat.call("triplet_embed_fwd_f32", r, D, w, D, b, D, E, EPS, e, d)
        nat.call("triplet_embed_bwd_f32", r, D, w, D, D, E, EPS, e, d, *g, dr, D, dw, D, db)
        keep("embed", cell, embed=e, dist=d, dr=dr, dw1=dw, db1=db)
    for cell in TT.MLP2_CELLS + [(1152, 50, 64)]:
        D, H, E = cell
        r, (w1, b1, w2, b2), g = rn(3, D), layers(cell), [rn(1), rn(1), rn(E), None, rn(E)]
        h, e, d, dr, dw1, db1, dw2, db2 = new(3, H), new(3, E), new(2), new(3, D), new(H, D), new(H), new(E, H), new(E)
        nat.call("mlp2_triplet_fwd_f32", r, D, w1, b1, w2, b2, D, H, E, EPS, h, e, d)
        nat.call("mlp2_triplet_bwd_f32", r, D, w1, w2, h, e, d, EPS, *g, D, H, E, dr, D, dw1, db1, dw2, db2)
        keep("mlp2t", cell, h=h, embed=e, dist=d, dr=dr, dw1=dw1, db1=db1, dw2=dw2, db2=db2)
    for p_drop in (0.0, 0.5):
        for cell in PC.MLP3_CELLS + [(2, 64, 32, 16, 8), (1, 256, 128, 64, 2)]:            # (+ RT = 2, the reference's defaults)
            R, D0, D1, D2, C = cell
            w = layers(cell[1:])
            st = lambda: (torch.zeros(2, dtype=torch.int64, device="cuda"), torch.zeros(1, dtype=torch.int64, device="cuda"))
            dro = lambda s, u: (float(p_drop), SEED, s if p_drop else None, u if p_drop else None)
            ks = 1.0 / (1.0 - p_drop)
            # the triplet tail at the cell's widths
            r, g = rn(3, D0), [rn(1), rn(1), None, rn(C), rn(C)]
            a1, a2, e, d, dx = new(3, D1), new(3, D2), new(3, C), new(2), new(3, D0)
            gw = [new(D1, D0), new(D1), new(D2, D1), new(D2), new(C, D2), new(C)]
            nat.call("mlp3_triplet_fwd_f32", r, D0, w[0], w[1], *dro(*st()), w[2], w[3], w[4], w[5], D0, D1, D2, C, EPS, a1, a2, e, d)
            nat.call("mlp3_triplet_bwd_f32", r, D0, w[0], w[2], w[4], a1, a2, e, d, EPS, ks, *g, D0, D1, D2, C, *gw, dx, D0)
            keep("mlp3t", cell[1:] + (p_drop,), a1=a1, a2=a2, embed=e, dist=d, dr=dx, dw1=gw[0], db1=gw[1], dw2=gw[2], db2=gw[3],
                 dw3=gw[4], db3=gw[5])
            # the post-training head on R rows
            r, (ids, lab), up = rn(R, D0), labels(R, C), rn(1)
            a1, a2, lp, loss, dr = new(R, D1), new(R, D2), new(R, C), new(1), new(R, D0)
            gw = [new(D1, D0), new(D1), new(D2, D1), new(D2), new(C, D2), new(C)]
            nat.call("posttrain_mlp3_nll_fwd_f32", r, D0, R, w[0], w[1], *dro(*st()), w[2], w[3], w[4], w[5], D0, D1, D2, C, ids, lab,
                     R + 3, a1, a2, lp, loss)
            nat.call("posttrain_mlp3_nll_bwd_f32", r, D0, R, w[0], w[2], w[4], D0, D1, D2, C, ks, ids, lab, R + 3, a1, a2, lp, up, dr, D0, *gw)
            keep("pt_mlp3", cell + (p_drop,), a1=a1, a2=a2, logp=lp, loss=loss, dr=dr, dw1=gw[0], db1=gw[1], dw2=gw[2], db2=gw[3],
                 dw3=gw[4], db3=gw[5])
    for cell in PC.MLP2_CELLS + [(4, 36, 7, 3), (8, 260, 130, 65), (1, 1152, 50, 2)]:
        R, D, H, C = cell
        r, (w1, b1, w2, b2), (ids, lab), up = rn(R, D), layers(cell[1:]), labels(R, C), rn(1)
        h, z, p, loss, dr, dw1, db1, dw2, db2 = new(R, H), new(R, C), new(R, C), new(1), new(R, D), new(H, D), new(H), new(C, H), new(C)
        nat.call("posttrain_mlp2_ce_fwd_f32", r, D, R, w1, b1, w2, b2, D, H, C, ids, lab, R + 3, h, z, p, loss)
        nat.call("posttrain_mlp2_ce_bwd_f32", r, D, R, w1, w2, D, H, C, ids, lab, R + 3, h, p, up, dr, D, dw1, db1, dw2, db2)
        keep("pt_mlp2", cell, h=h, z=z, p=p, loss=loss, dr=dr, dw1=dw1, db1=db1, dw2=dw2, db2=db2)
    for cell in [(1, 4, 1, 1, 1, 2), (2, 36, 5, 7, 3, 3), (3, 260, 130, 20, 10, 5), (8, 1152, 512, 64, 64, 64), (1, 256, 128, 64, 32, 2)]:
        R, P, E, h1, h2, C = cell
        r, W, (ids, lab), up = rn(R, P), layers(cell[1:]), labels(R, C), rn(1)
        out, z1, z2, z, p, loss, dr = new(R, E), new(R, h1), new(R, h2), new(R, C), new(R, C), new(1), new(R, P)
        gw = [new(E, P), new(E), new(h1, E), new(h1), new(h2, h1), new(h2), new(C, h2), new(C)]
        nat.call("posttrain_head_fwd_f32", r, P, R, P, W[0], W[1], E, W[2], W[3], h1, W[4], W[5], h2, W[6], W[7], C, 0.01, ids, lab, R + 3,
                 out, z1, z2, z, p, loss)
        nat.call("posttrain_head_bwd_f32", r, P, R, P, W[0], E, W[2], h1, W[4], h2, W[6], C, 0.01, ids, lab, R + 3, out, z1, z2, p, up, dr, P,
                 *gw)
        keep("pt_head", cell, out=out, z1=z1, z2=z2, z=z, p=p, loss=loss, dr=dr, **{"g%d" % i: t for i, t in enumerate(gw)})
    torch.cuda.synchronize()
    np.savez(path, **res)
    print("%d tensors of %s -> %s" % (len(res), os.environ.get("TSGNN_LIB_PATH") or nat.LIB_PATH, path))


def cmp(pa, pb):
    a, b = np.load(pa), np.load(pb)
    assert sorted(a.files) == sorted(b.files)
    bad = 0
    for k in a.files:
        same = np.array_equal(a[k], b[k])
        fam, _, name = k.split("/")
        line = "%-44s array_equal %s" % (k, same)
        if "%s/%s" % (fam, name) in OUTER_PRODUCTS:
            fa, fb = a[k].view(np.float32).astype(np.float64), b[k].view(np.float32).astype(np.float64)
            line += "   (outer product) max|tree - parent| = %.2f x 2^-23 max|parent|" % (np.abs(fb - fa).max() / (2.0 ** -23 * max(np.abs(fa).max(), 1e-300)))
        if not same:
            bad += 1
            line += "   %d of %d words differ" % (int((a[k] != b[k]).sum()), a[k].size)
        print(line)
    print("%d tensors, %d differ" % (len(a.files), bad))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(run(sys.argv[2]) if sys.argv[1] == "run" else cmp(sys.argv[2], sys.argv[3]))
