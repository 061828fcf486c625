"""The tolerance scheme of the kernel-against-float64 tests (test_gpu_slot_kernels.py, test_gpu_gat_attn_kernels.py).  For every float
tensor (ref64: the reference in float64; cpu32: the SAME reference code with dtype=float32 on the CPU):

    max|hip - ref64|  <=  K * max( max|cpu32 - ref64| , 2**-23 * max|ref64| )

The yardstick is the reference's own fp32 rounding, never the kernel."""
import torch

EPS32 = 2.0 ** -23
K_DEFAULT = 8.0


def _yardstick(ref64, cpu32):
    ref64 = ref64.double()
    return max((cpu32.double() - ref64).abs().max().item(), EPS32 * ref64.abs().max().item()) if ref64.numel() else 0.0


def _ratio(hip, ref64, cpu32):
    ref64 = ref64.double()
    yard = _yardstick(ref64, cpu32)
    err = (hip.double() - ref64).abs().max().item() if ref64.numel() else 0.0
    if err != err:
        return float("inf")
    if yard == 0.0:
        return 0.0 if err == 0.0 else float("inf")
    return err / yard


def _check(what, hip, ref64, cpu32, K=K_DEFAULT):
    hip = hip.detach().cpu()
    assert hip.shape == ref64.shape, (what, hip.shape, ref64.shape)
    assert not torch.isnan(hip).any().item(), "%s: %d elements were never written" % (what, int(torch.isnan(hip).sum()))
    r = _ratio(hip, ref64, cpu32)
    print("%s: max|hip - ref64| / yardstick = %.3f" % (what, r))
    assert r <= K, "%s: %.3f x the fp32 yardstick (bound %g)" % (what, r, K)
    return r
