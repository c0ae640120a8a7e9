"""The rotated crop and paste contracts restated in numpy (csrc/resize.hip: crop_resize_cubic_rot_kernel,
paste_resize_cubic_rot_kernel; include/d3f_hip.h: the _rboxes_ operators; DESIGN.md section 4 "Rotated crop"), independent of
the library.  Positions are exact integers reduced by one floor to 16 fractional bits, as in the kernels.  The values are
computed in `dtype`:
  * np.float32 follows the device operation for operation (numpy rounds every float32 operation once and fuses nothing, as
    the library's -ffp-contract=off build does), so its rounded bytes are the kernels' bytes;
  * np.float64 is the same definition without the fp32 rounding: what the float64 oracle (torch's grid_sample on the real
    cos / sin) is compared with, so that only the two quantisations separate them.
Angle convention: x right, y down; a positive angle turns the box clockwise on the screen about its centre; the crop's column
direction is (cos a, sin a), its row direction (-sin a, cos a)."""
import math

import numpy as np

FRAC_BITS = 16
ONE = 1 << FRAC_BITS


def box_rotation(angle_degrees):
    """(c16, s16) of an angle: rounded to hundredths of a degree, wrapped to (-180, 180], then round(cos * 65536),
    round(sin * 65536) -- the multiples of 90 degrees exactly"""
    h = int(round(float(angle_degrees) * 100.0)) % 36000
    if h > 18000:
        h -= 36000
    exact = {0: (ONE, 0), 9000: (0, ONE), 18000: (-ONE, 0), -9000: (0, -ONE)}
    if h in exact:
        return exact[h]
    a = math.radians(h / 100.0)
    return int(round(math.cos(a) * ONE)), int(round(math.sin(a) * ONE))


def keys_weights(t, dtype):
    """[..., 4]: the Keys weights (A = -0.75) at t + 1, t, 1 - t, 2 - t, every operation rounded in dtype"""
    t = np.asarray(t, dtype=dtype)
    A, one, two = dtype(-0.75), dtype(1), dtype(2)

    def inner(x):  # |x| <= 1
        return ((A + dtype(2)) * x - (A + dtype(3))) * x * x + one

    def outer(x):  # 1 < |x| < 2
        return ((A * x - dtype(5) * A) * x + dtype(8) * A) * x - dtype(4) * A

    w = np.stack([outer(t + one), inner(t), inner(one - t), outer(two - t)], axis=-1)
    assert w.dtype == dtype
    return w


def sample(img, px, py, dtype):
    """img [h, w, 3] uint8, fixed-point positions px, py (int64, any shape S) -> dtype [S..., 3]: taps s - 1 .. s + 2 clamped
    inside img, horizontal pass then vertical pass, each sum taken left to right"""
    h, w = img.shape[:2]
    shape = px.shape
    px, py = px.reshape(-1), py.reshape(-1)
    wx = keys_weights((px & (ONE - 1)).astype(dtype) / dtype(ONE), dtype)
    wy = keys_weights((py & (ONE - 1)).astype(dtype) / dtype(ONE), dtype)
    ix = np.clip((px >> FRAC_BITS)[:, None] + np.arange(-1, 3)[None, :], 0, w - 1)
    iy = np.clip((py >> FRAC_BITS)[:, None] + np.arange(-1, 3)[None, :], 0, h - 1)
    taps = img[iy[:, :, None], ix[:, None, :]].astype(dtype)  # [N, row, column, 3]
    hrow = wx[:, None, 0, None] * taps[:, :, 0]
    for k in range(1, 4):
        hrow = hrow + wx[:, None, k, None] * taps[:, :, k]
    v = wy[:, 0, None] * hrow[:, 0]
    for r in range(1, 4):
        v = v + wy[:, r, None] * hrow[:, r]
    assert v.dtype == dtype
    return v.reshape(shape + (3,))


def crop_positions(box, rot, size):
    """the fixed-point frame positions (px, py), int64 [H, W], of the output pixels of an H x W crop of the rotated box"""
    x1, y1, cw, ch = (int(v) for v in box)
    c16, s16 = (int(v) for v in rot)
    H, W = size
    ox, oy = np.arange(W, dtype=np.int64)[None, :], np.arange(H, dtype=np.int64)[:, None]
    nu, nv = cw * (2 * ox + 1 - W), ch * (2 * oy + 1 - H)
    base = ONE * W * H
    numx = (2 * x1 + cw - 1) * base + c16 * nu * H - s16 * nv * W
    numy = (2 * y1 + ch - 1) * base + s16 * nu * H + c16 * nv * W
    den = 2 * W * H
    return numx // den, numy // den  # floor division


def rot_crop(frame, box, rot, size, dtype=np.float32):
    """frame [h, w, 3] uint8 -> dtype [H, W, 3] before rounding; taps clamp to the FRAME"""
    px, py = crop_positions(box, rot, size)
    return sample(frame, px, py, dtype)


def round_u8(v):
    """rint (half to even), clamp to 0..255"""
    return np.clip(np.rint(v), 0, 255).astype(np.uint8)


def local_numerators(box, rot, h, w):
    """(n_j, n_i), int64 [h, w]: the box-local position (j', i') of every frame pixel, times 2^17"""
    x1, y1, cw, ch = (int(v) for v in box)
    c16, s16 = (int(v) for v in rot)
    dx2 = 2 * np.arange(w, dtype=np.int64)[None, :] - 2 * x1 - cw + 1
    dy2 = 2 * np.arange(h, dtype=np.int64)[:, None] - 2 * y1 - ch + 1
    return (cw - 1) * ONE + c16 * dx2 + s16 * dy2, (ch - 1) * ONE - s16 * dx2 + c16 * dy2


def inside(n, extent):
    """-0.5 <= position < extent - 0.5"""
    return (n >= -ONE) & (n < (2 * extent - 1) * ONE)


def patch_position(n, extent, n_out):
    """(j' + 0.5) n_out / extent - 0.5 in fixed point"""
    return ((n + ONE) * n_out - ONE * extent) // (2 * extent)


def axis_ramp(n, extent, feather):
    """float32: min(d' + 1, feather + 1) / (feather + 1) on the fixed-point distance, two integers converted to float32 and
    one division"""
    fx = n >> 1
    d = np.minimum(fx, (extent - 1) * ONE - fx)
    full = (feather + 1) * ONE
    a = np.minimum(d + ONE, full).astype(np.float32) / np.float32(full)
    assert a.dtype == np.float32
    return a


def rot_paste(patch, frame, box, rot, feather, coef=None, dtype=np.float32):
    """patch [H, W, 3] uint8, frame [h, w, 3] uint8 -> (dtype [h, w, 3] before rounding, the mask [h, w] of the box's pixels):
    the frame outside the rotated rectangle, a * v + (1 - a) * s inside.  coef: float32 [3, 2], gain and offset per
    byte-in-pixel (the colour form)"""
    cw, ch = int(box[2]), int(box[3])
    h, w = frame.shape[:2]
    H, W = patch.shape[:2]
    nj, ni = local_numerators(box, rot, h, w)
    nj, ni = np.broadcast_arrays(nj, ni)
    mask = inside(nj, cw) & inside(ni, ch)
    out = frame.astype(dtype)
    nj, ni = nj[mask], ni[mask]
    v = sample(patch, patch_position(nj, cw, W), patch_position(ni, ch, H), dtype)
    v = np.minimum(np.maximum(v, dtype(0)), dtype(255))
    if coef is not None:
        coef = np.asarray(coef, dtype=np.float32).astype(dtype)
        scaled = coef[None, :, 0] * v
        v = np.minimum(np.maximum(scaled + coef[None, :, 1], dtype(0)), dtype(255))
    a = axis_ramp(ni, ch, feather) * axis_ramp(nj, cw, feather)  # one float32 product
    na = np.float32(1) - a
    assert a.dtype == np.float32 and na.dtype == np.float32
    pv, ps = a.astype(dtype)[:, None] * v, na.astype(dtype)[:, None] * out[mask]
    out[mask] = pv + ps
    assert out.dtype == dtype
    return out, mask
