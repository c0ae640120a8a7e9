"""The colour match contract restated in numpy (include/d3f_hip.h: d3f_channel_sums_u8, d3f_color_match_coef,
d3f_paste_resize_cubic_color_u8), independent of the library: the sums with Python integers, the coefficients in float64
operation for operation and then rounded to float32, and the colour paste built on the resize and paste restatements -- the
float32 coefficients widened to float64, gain, offset and the second clip applied in front of the blend, so that the only
differences from the kernel are its fp32 accumulation and the fp32 roundings of gain * v + offset."""
import numpy as np

from paste_restatement import ramp
from resize_restatement import crop_resize_cubic_f64

GAIN_MIN, GAIN_MAX = 0.5, 2.0   # D3F_COLOR_GAIN_MIN, D3F_COLOR_GAIN_MAX
MAX_PIXELS = 1 << 22


def channel_sums(img):
    """img [B, H, W, 3] (or [H, W, 3]) uint8 -> nested lists [B][3][2] of Python integers: S = sum p, Q = sum p * p"""
    x = np.asarray(img)
    x = x[None] if x.ndim == 3 else x
    out = []
    for frame in x:
        per_channel = []
        for c in range(3):
            # 256 bins of exact counts, then Python integers: no fixed-width accumulator anywhere
            counts = np.bincount(frame[:, :, c].reshape(-1), minlength=256)
            s = sum(int(k) * v for v, k in enumerate(counts))
            q = sum(int(k) * v * v for v, k in enumerate(counts))
            per_channel.append([s, q])
        out.append(per_channel)
    return out


def sums_array(sums):
    """the nested lists as a uint64 array [B, 3, 2]"""
    return np.array(sums, dtype=np.uint64).reshape(-1, 3, 2)


def color_match_coef(sums_from, sums_to, n):
    """nested lists / arrays [B][3][2] of integers -> float32 [B, 3, 2], gain then offset"""
    n = int(n)
    B = len(sums_from)
    coef = np.zeros((B, 3, 2), dtype=np.float32)
    for b in range(B):
        for c in range(3):
            s_f, q_f = int(sums_from[b][c][0]), int(sums_from[b][c][1])
            s_t, q_t = int(sums_to[b][c][0]), int(sums_to[b][c][1])
            d_f, d_t = n * q_f - s_f * s_f, n * q_t - s_t * s_t
            assert 0 <= d_f < 1 << 60 and 0 <= d_t < 1 << 60
            m_f = np.float64(s_f) / np.float64(n)
            m_t = np.float64(s_t) / np.float64(n)
            if d_f == 0 or d_t == 0:
                g = np.float64(1.0)
            else:
                g = np.sqrt(np.float64(d_t) / np.float64(d_f))   # int -> float64 rounds to nearest even, as the device's
            g = np.minimum(np.maximum(g, np.float64(GAIN_MIN)), np.float64(GAIN_MAX))
            scaled = g * m_f
            o = m_t - scaled
            coef[b, c, 0] = np.float32(g)
            coef[b, c, 1] = np.float32(o)
    return coef


def paste_color_f64(patch, frame, box, feather, coef):
    """patch [H, W, 3] uint8, frame [h, w, 3] uint8, box (x1, y1, cw, ch), coef float32 [3, 2] -> float64 [h, w, 3] before
    rounding: paste_restatement.paste_f64 with w = clip(gain * clip(v) + offset) in place of clip(v)"""
    x1, y1, cw, ch = box
    H, W = patch.shape[:2]
    coef = np.asarray(coef)
    assert coef.dtype == np.float32 and coef.shape == (3, 2)
    v = np.clip(crop_resize_cubic_f64(patch, (0, 0, W, H), (ch, cw)), 0.0, 255.0)
    gain, offset = coef[:, 0].astype(np.float64), coef[:, 1].astype(np.float64)
    w = np.clip(gain[None, None, :] * v + offset[None, None, :], 0.0, 255.0)
    a = ramp(cw, ch, feather)
    na = np.float32(1) - a
    assert na.dtype == np.float32
    out = frame.astype(np.float64)
    s = out[y1:y1 + ch, x1:x1 + cw]
    out[y1:y1 + ch, x1:x1 + cw] = a.astype(np.float64)[:, :, None] * w + na.astype(np.float64)[:, :, None] * s
    return out
