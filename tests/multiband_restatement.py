"""The multiband paste contract restated in numpy integers (csrc/multiband.hip, include/d3f_hip.h: d3f_paste_multiband_u8),
independent of the library.  Everything behind the target byte V is integer arithmetic -- the difference image, REDUCE,
EXPAND, the band masks, the collapse -- and is restated here operation for operation in int64, so every comparison with
the device is exact.  V itself is an INPUT: the byte the plain paste writes in the box at feather 0 (on the device,
`ops.paste_resize_cubic_u8(..., feather=0)`; without one, the float64 paste restatement's rounded interior).

Arrays are [h, w] or [h, w, C]; the two leading axes are filtered, anything behind them rides along."""
import numpy as np

REDUCE_W = (1, 4, 6, 4, 1)


def level_sizes(n, levels):
    """[n_0 .. n_levels]: n_0 = n, n_{l+1} = (n_l + 1) // 2"""
    sizes = [int(n)]
    for _ in range(levels):
        sizes.append((sizes[-1] + 1) // 2)
    return sizes


def _take(g, idx, axis):
    """g at `idx` along `axis`, indices clamped into the level"""
    return np.take(g, np.clip(idx, 0, g.shape[axis] - 1), axis=axis)


def _reduce_axis(g, axis):
    n_out = (g.shape[axis] + 1) // 2
    centre = 2 * np.arange(n_out)
    return sum(w * _take(g, centre + a, axis) for a, w in zip(range(-2, 3), REDUCE_W))


def reduce_level(g):
    """g_{l+1} = (sum over a, b of w_a w_b g_l[clamp(2i + a)][clamp(2j + b)] + 128) >> 8: separable, nothing rounded between
    the passes"""
    g = np.asarray(g, dtype=np.int64)
    return (_reduce_axis(_reduce_axis(g, 1), 0) + 128) >> 8


def _expand_axis(g, n_out, axis):
    """per axis, unnormalised (weights sum to 8): index 2k takes g[k-1] + 6 g[k] + g[k+1], index 2k+1 takes 4 g[k] + 4 g[k+1]"""
    i = np.arange(n_out)
    k = i >> 1
    even = _take(g, k - 1, axis) + 6 * _take(g, k, axis) + _take(g, k + 1, axis)
    odd = 4 * _take(g, k, axis) + 4 * _take(g, k + 1, axis)
    shape = [1] * g.ndim
    shape[axis] = n_out
    return np.where((i & 1).reshape(shape) == 1, odd, even)


def expand_level(g, h, w):
    """EXPAND of a level to h x w: the product form of the two axes, (sum + 32) >> 6"""
    g = np.asarray(g, dtype=np.int64)
    return (_expand_axis(_expand_axis(g, w, 1), h, 0) + 32) >> 6


def band_F(feather, levels):
    """the ramp's width in samples of every level"""
    return (int(feather) + (1 << levels) - 1) >> levels


def band_M(h, w, F):
    """M = n_y n_x [h, w] with n(i) = min(min(i, n - 1 - i) + 1, F + 1)"""
    def n(size):
        i = np.arange(size)
        return np.minimum(np.minimum(i, size - 1 - i) + 1, F + 1)
    return (n(h)[:, None] * n(w)[None, :]).astype(np.int64)


def band_mask(x, F):
    """m_l(x) = floor((2 x M + den) / (2 den)), den = (F + 1)^2; numpy's // floors for negative x as well"""
    x = np.asarray(x, dtype=np.int64)
    den = (F + 1) ** 2
    M = band_M(x.shape[0], x.shape[1], F).reshape(x.shape[:2] + (1,) * (x.ndim - 2))
    return (2 * x * M + den) // (2 * den)


def multiband_E(D, feather, levels):
    """D [ch, cw(, C)] integers in -255..255 -> E, the blended difference: g_0 = D << 6, the pyramid, the masked collapse,
    E = (R_0 + 32) >> 6"""
    D = np.asarray(D, dtype=np.int64)
    if not 1 <= levels <= 6 or min(D.shape[:2]) < (1 << levels):
        raise ValueError("levels outside 1..6, or a box below 1 << levels on a side")
    F = band_F(feather, levels)
    g = [D << 6]
    for _ in range(levels):
        g.append(reduce_level(g[-1]))
        assert np.abs(g[-1]).max(initial=0) <= 16320
    R = band_mask(g[levels], F)
    for l in range(levels - 1, -1, -1):
        h, w = g[l].shape[:2]
        lap = g[l] - expand_level(g[l + 1], h, w)
        assert np.abs(lap).max(initial=0) <= 32640  # fits int16
        R = expand_level(R, h, w) + band_mask(lap, F)
        assert np.abs(R).max(initial=0) < 2 ** 31
    return (R + 32) >> 6


def paste_multiband(V, frame, box, feather, levels):
    """V [ch, cw, 3] uint8: the target bytes of the box; frame [h, w, 3] uint8; box (x1, y1, cw, ch) -> uint8 [h, w, 3]:
    clamp(s + E, 0, 255) in the box, the frame outside"""
    x1, y1, cw, ch = box
    assert V.shape == (ch, cw, 3) and V.dtype == np.uint8 and frame.dtype == np.uint8
    out = frame.copy()
    s = frame[y1:y1 + ch, x1:x1 + cw].astype(np.int64)
    E = multiband_E(V.astype(np.int64) - s, feather, levels)
    out[y1:y1 + ch, x1:x1 + cw] = np.clip(s + E, 0, 255).astype(np.uint8)
    return out


def target_bytes_f64(patch, box):
    """V without a device: the float64 paste restatement's interior, rounded half to even and clamped.  (The device's V is
    rintf of an fp32 sum and may differ by one level where the float64 value lies near a half: the device tests take V from
    `ops.paste_resize_cubic_u8(..., feather=0)` instead.)"""
    from resize_restatement import crop_resize_cubic_f64
    x1, y1, cw, ch = box
    H, W = patch.shape[:2]
    v = np.clip(crop_resize_cubic_f64(patch, (0, 0, W, H), (ch, cw)), 0.0, 255.0)
    return np.clip(np.rint(v), 0, 255).astype(np.uint8)
