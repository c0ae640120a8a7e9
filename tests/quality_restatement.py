"""The per-image scores of csrc/quality.hip restated in float64 with their error bounds, on the bound arithmetic of
tests/test_gpu_helper_kernels.py (class E, filter1d: every fp32 operation adds 2^-24 of its result to what its operands
bring), and the same formulas in plain torch fp32 for the CPU test that shows the bounds admit an honest evaluation."""
import math

import numpy as np
import torch
import torch.nn.functional as F

import test_gpu_helper_kernels as hk

E, U24, filter1d, hold = hk.E, hk.U24, hk.filter1d, hk.hold
ROWS = ("mse", "ssim", "psnr", "loss")
# quality_partial_kernel's sum of one tile: at most seven adds in a thread (an element of the 42 x 42 fill per trip; the
# row filter hands a thread four ss values), six shuffle steps and a tree of four (two levels): 15 roundings of sums that
# are at most the sum of the absolute terms.  quality_finalize_kernel adds the tile sums in float64 (2^-53 each: covered
# by the factor 1 + 1e-6), divides once and rounds the quotient to fp32 once.
PARTIAL_ROUNDINGS = 15
# psnr = -10 log10(mse01): the bound of mse01 through d log10(m) / dm = 1 / (m ln 10), taken at the near end m - err of the
# interval (the derivative falls with m); an fp32 log10 is accurate to 2 units in the last place (2 * 2^-23 relative; the
# kernel's own, evaluated in float64 and rounded once, is inside that), and the product with 10 is rounded once.
LOG10_ULPS = 2


def quality_reference(p, t, lo=-1.0, hi=1.0):
    """p, t: [B, 3, H, W] float64 tensors holding fp32 values -> {row: E of shape [B]}"""
    f32 = lambda v: float(np.float32(v))
    B, _, H, W = p.shape
    pp, tt = p.reshape(-1, H, W), t.reshape(-1, H, W)
    rng_ = f32(np.float32(hi) - np.float32(lo))
    xh, yh = ((E(pp) - lo) / rng_).clip01(), ((E(tt) - lo) / rng_).clip01()
    both = lambda q: filter1d(filter1d(q, 1, False), 2, False)
    mux, muy, m2, m3, m4 = both(xh), both(yh), both(xh * xh), both(yh * yh), both(xh * yh)
    c1, c2 = f32(np.float32(0.01) * np.float32(0.01)), f32(np.float32(0.03) * np.float32(0.03))
    sxx, syy, sxy = m2 - mux * mux, m3 - muy * muy, m4 - mux * muy
    a1, b1 = (mux.twice() * muy) + c1, (mux * mux + muy * muy) + c1
    a2, b2 = sxy.twice() + c2, (sxx + syy) + c2
    ss = (a1 / b1) * (a2 / b2)
    diff, diff01 = E(pp) - E(tt), xh - yh

    def image_mean(q):
        count = q.val[0].numel() * 3
        val, err = q.val.reshape(B, -1), q.err.reshape(B, -1)
        tot = val.sum(1) / count
        return E(tot, (err.sum(1) + PARTIAL_ROUNDINGS * U24 * (val.abs() + err).sum(1)) / count * (1 + 1e-6) + U24 * tot.abs())

    mse, ssim, mse01 = image_mean(diff * diff), image_mean(ss), image_mean(diff01 * diff01)
    loss = mse + (E.lift(1.0) - ssim)
    assert bool((mse01.val > 2 * mse01.err).all()), "an mse01 the bound cannot separate from 0"
    psnr = -10.0 * torch.log10(mse01.val)
    psnr_err = (10.0 / math.log(10.0) * mse01.err / (mse01.val - mse01.err)
                + 10.0 * torch.log10(mse01.val).abs() * LOG10_ULPS * 2.0 ** -23 + U24 * psnr.abs()) * (1 + 1e-6)
    return {"mse": mse, "ssim": ssim, "psnr": E(psnr, psnr_err), "loss": E(loss.val / 2, loss.err / 2), "mse01": mse01}


def quality_torch_fp32(p, t, lo=-1.0, hi=1.0):
    """the same four values per image in plain torch fp32 (conv2d's and mean's own summation orders): [4, B]"""
    B, _, H, W = p.shape
    g = hk.gauss_window().float()
    x, y = ((p - lo) / (hi - lo)).clamp(0, 1), ((t - lo) / (hi - lo)).clamp(0, 1)
    f = lambda q: F.conv2d(F.conv2d(q.reshape(-1, 1, H, W), g.view(1, 1, 11, 1)), g.view(1, 1, 1, 11))
    mux, muy = f(x), f(y)
    sxx, syy, sxy = f(x * x) - mux * mux, f(y * y) - muy * muy, f(x * y) - mux * muy
    c1, c2 = np.float32(0.01) * np.float32(0.01), np.float32(0.03) * np.float32(0.03)
    ss = ((2 * mux * muy + c1) / (mux * mux + muy * muy + c1)) * ((2 * sxy + c2) / (sxx + syy + c2))
    mse = ((p - t) ** 2).reshape(B, -1).mean(1)
    ssim = ss.reshape(B, -1).mean(1)
    psnr = -10 * torch.log10(((x - y) ** 2).reshape(B, -1).mean(1))
    return torch.stack([mse, ssim, psnr, (mse + (1 - ssim)) / 2])


def hold_rows(what, got, ref):
    """got: [4, B] (rows ROWS) against quality_reference's dict; prints each row's worst error over its bound first"""
    for i, row in enumerate(ROWS):
        err = (got[i].double() - ref[row].val).abs()
        print(f"{what} {row}: worst error {float(err.max()):.3e}, worst error / bound {float((err / ref[row].err).max()):.3f}")
    for i, row in enumerate(ROWS):
        hold(f"{what} {row}", got[i], ref[row])
