"""The paste contract restated in float64 numpy (csrc/resize.hip: paste_resize_cubic_kernel, include/d3f_hip.h:
d3f_paste_resize_cubic_u8), independent of the library and built on the resize restatement: the patch resized H x W ->
ch x cw in float64, clamped to 0..255, blended into the box over the separable ramp.  The ramp is formed as the device forms
it -- float32 quotients of exact integers, their float32 product, 1 - a in float32 -- and then widened, so that the only
difference from the kernel is its fp32 accumulation."""
import numpy as np

from resize_restatement import crop_resize_cubic_f64


def axis_ramp(n, feather):
    """float32 [n]: min(d + 1, feather + 1) / (feather + 1) with d the distance to the nearer end of the axis"""
    i = np.arange(n)
    d = np.minimum(i, n - 1 - i)
    return np.minimum(d + 1, feather + 1).astype(np.float32) / np.float32(feather + 1)


def ramp(cw, ch, feather):
    """float32 [ch, cw]: a = a_y * a_x, one float32 product"""
    a = axis_ramp(ch, feather)[:, None] * axis_ramp(cw, feather)[None, :]
    assert a.dtype == np.float32
    return a


def paste_f64(patch, frame, box, feather):
    """patch [H, W, 3] uint8, frame [h, w, 3] uint8, box (x1, y1, cw, ch) -> float64 [h, w, 3] before rounding: the frame
    outside the box, a * v + (1 - a) * s inside"""
    x1, y1, cw, ch = box
    H, W = patch.shape[:2]
    v = np.clip(crop_resize_cubic_f64(patch, (0, 0, W, H), (ch, cw)), 0.0, 255.0)
    a = ramp(cw, ch, feather)
    na = np.float32(1) - a
    assert na.dtype == np.float32
    out = frame.astype(np.float64)
    s = out[y1:y1 + ch, x1:x1 + cw]
    out[y1:y1 + ch, x1:x1 + cw] = a.astype(np.float64)[:, :, None] * v + na.astype(np.float64)[:, :, None] * s
    return out
