"""The crop + bicubic resize contract restated in float64 numpy (csrc/resize.hip, include/d3f_hip.h:
d3f_crop_resize_cubic_u8), independent of the library: cv2.INTER_CUBIC in float arithmetic.  Source coordinates are
exact rationals (integers here, as in the kernel), the weights and the two passes are float64, which is what the fp32
kernel is measured against."""
import numpy as np

A = -0.75


def keys_weight(x):
    """Keys cubic convolution kernel, A = -0.75, for x >= 0"""
    x = np.asarray(x, dtype=np.float64)
    inner = ((A + 2) * x - (A + 3)) * x * x + 1          # |x| <= 1
    outer = ((A * x - 5 * A) * x + 8 * A) * x - 4 * A    # 1 < |x| < 2
    return np.where(x <= 1, inner, outer)


def axis_taps(n_in, n_out):
    """for every output index of an axis n_in -> n_out: the four clamped tap indices [n_out, 4] and weights [n_out, 4].
    f = (d + 0.5) * n_in / n_out - 0.5 = num / den with num = (2d + 1) n_in - n_out, den = 2 n_out"""
    d = np.arange(n_out, dtype=np.int64)
    num, den = (2 * d + 1) * n_in - n_out, 2 * n_out
    s = num // den                      # floor division
    t = (num - s * den) / den           # exact remainder over den, in [0, 1)
    idx = np.clip(s[:, None] + np.arange(-1, 3)[None, :], 0, n_in - 1)   # replicate border
    w = np.stack([keys_weight(t + 1), keys_weight(t), keys_weight(1 - t), keys_weight(2 - t)], axis=1)
    return idx, w


def crop_resize_cubic_f64(frame, box, size):
    """frame [h, w, c] uint8, box (x1, y1, cw, ch), size (H, W) -> float64 [H, W, c] before rounding"""
    x1, y1, cw, ch = box
    H, W = size
    crop = frame[y1:y1 + ch, x1:x1 + cw].astype(np.float64)
    ix, wx = axis_taps(cw, W)
    iy, wy = axis_taps(ch, H)
    horizontal = (crop[:, ix, :] * wx[None, :, :, None]).sum(axis=2)       # [ch, W, c]
    return (horizontal[iy, :, :] * wy[:, :, None, None]).sum(axis=1)       # [H, W, c]


def round_u8(v):
    """rint (half to even), clamp to 0..255"""
    return np.clip(np.rint(v), 0, 255).astype(np.uint8)

