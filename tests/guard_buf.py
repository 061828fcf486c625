"""Shared by the kernel-placement tests (test_gpu_result_stores.py, test_gpu_head_kernels.py): the guarded output buffer `Out` — every
word one NaN bit pattern, guard words behind it —, the ownership mask of a launch, and `_du_ref`, the restatement of the dU rows the
head backward's dU role leaves.  TEST INFRASTRUCTURE: no project kernel."""
import torch

PAT = 0x7FC0BEEF                        # a quiet NaN with a payload of its own
GUARD = 64
CLAMPED = 0.999e12                      # rinv at or above this: the row's norm was clamped, no projection (slot_ref.CLAMPED)


class Out:
    """[rows, ld] float32 on the device, every word PAT, GUARD words of PAT behind it"""

    def __init__(self, rows, ld):
        self.rows, self.ld = rows, ld
        self.bits = torch.full((rows * ld + GUARD,), PAT, dtype=torch.int32, device="cuda")
        self.mat = self.bits[:rows * ld].view(torch.float32).view(rows, ld)

    def rest_untouched(self, what, owned):
        """owned: bool [rows, ld] on the CPU — the elements the launch may write"""
        torch.cuda.synchronize()
        b = self.bits.cpu()
        body, guard = b[:self.rows * self.ld].view(self.rows, self.ld), b[self.rows * self.ld:]
        assert bool((guard == PAT).all()), "%s: %d guard words overwritten" % (what, int((guard != PAT).sum()))
        bad = (body != PAT) & ~owned
        assert not bool(bad.any()), "%s: %d elements written outside the launch's own (first at %s)" % (
            what, int(bad.sum()), bad.nonzero()[0].tolist())


def _owned(rows, ld, r0, r1, c0, c1):
    m = torch.zeros(rows, ld, dtype=torch.bool)
    m[r0:r1, c0:c1] = True
    return m


def _du_ref(v, rinv, arg, dout, off, graph_ptr, n_real, n_ghost, dtype):
    """rows of the last layer's dU as the head backward's dU role leaves them: du[r] = rinv_r (g_r - v_r <v_r, g_r>) with g_r[f] =
    dout[b, off + f] where r won (graph b, column f); graph b's ghost contribution (its first ghost row, n_real + size_b) at n_real + b.
    <v_r, g_r> counts as 0 on a row whose norm was clamped (rinv_r >= CLAMPED); rows of no graph ([graph_ptr[B], n_real)) are 0"""
    B, F = arg.shape
    v, rinv, dout = v.to(dtype), rinv.to(dtype), dout.to(dtype)
    out = torch.zeros(n_real + B, F, dtype=dtype)

    def row(r, b):
        g = torch.where(arg[b] == r, dout[b, off:off + F], torch.zeros(F, dtype=dtype))
        dot = (v[r] * g).sum() if float(rinv[r]) < CLAMPED else 0.0
        return rinv[r] * (g - v[r] * dot)
    for b in range(B):
        for r in range(int(graph_ptr[b]), int(graph_ptr[b + 1])):
            out[r] = row(r, b)
        sz = int(graph_ptr[b + 1] - graph_ptr[b])
        if sz < n_ghost:
            out[n_real + b] = row(n_real + sz, b)
    return out
