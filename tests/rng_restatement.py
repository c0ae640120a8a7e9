"""The device RNG's contract restated in numpy (csrc/philox.h, include/d3f_hip.h): Philox4x32-10 and the draw layout,
independent of the library.  Integers and the uniforms are exact; the normals are evaluated in float64 from the same
words, which is what the fp32 kernels are measured against."""
import math

import numpy as np

M0, M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
W0, W1 = 0x9E3779B9, 0xBB67AE85
G_Y, G_AUG, G_APPLY = 0xFFFFFFFF, 0xFFFFFFFE, 0xFFFFFFFD
MASK = np.uint64(0xFFFFFFFF)
S32 = np.uint64(32)


def philox4x32_10(counter, key):
    """counter: 4 arrays (or ints) of uint32 words, broadcast together; key: 2 ints.  Returns 4 uint32 arrays."""
    c = [np.asarray(v, dtype=np.uint64) & MASK for v in counter]
    c = list(np.broadcast_arrays(*c))
    k0, k1 = int(key[0]) & 0xFFFFFFFF, int(key[1]) & 0xFFFFFFFF
    for _ in range(10):
        p0, p1 = M0 * c[0], M1 * c[2]          # 32 x 32 -> 64 bit products: no overflow in uint64
        c = [(p1 >> S32) ^ c[1] ^ np.uint64(k0), p1 & MASK, (p0 >> S32) ^ c[3] ^ np.uint64(k1), p0 & MASK]
        k0, k1 = (k0 + W0) & 0xFFFFFFFF, (k1 + W1) & 0xFFFFFFFF
    return [v.astype(np.uint32) for v in c]


def block(seed, offset, b, g):
    """the four words of group g of image b in the stream (seed, offset)"""
    seed, offset = int(seed), int(offset)
    return philox4x32_10((g, b, offset & 0xFFFFFFFF, offset >> 32), (seed & 0xFFFFFFFF, seed >> 32))


def uniform24(x):
    """[0, 1) on the 2^-24 grid: exact in float32"""
    return ((np.asarray(x, dtype=np.uint32) >> np.uint32(8)).astype(np.float64) * 2.0 ** -24).astype(np.float32)


def y_uniform(seed, offset, B):
    return uniform24(block(seed, offset, np.arange(B), G_Y)[0])


def normals64(seed, offset, B, per_image, images=None):
    """float64 Box-Muller from the same words: (z [B, per_image], R [B, per_image]); images: which b (default all)"""
    assert per_image % 4 == 0 and per_image // 4 < G_APPLY
    bs = np.arange(B) if images is None else np.asarray(images)
    g = np.arange(per_image // 4)
    x = block(seed, offset, bs[:, None], g[None, :])
    z = np.empty((len(bs), per_image // 4, 4), dtype=np.float64)
    rr = np.empty_like(z)
    for j in (0, 1):
        ua = ((x[2 * j] >> np.uint32(9)).astype(np.float64) + 0.5) * 2.0 ** -23
        ub = (x[2 * j + 1] >> np.uint32(8)).astype(np.float64) * 2.0 ** -24
        r = np.sqrt(-2.0 * np.log(ua))
        z[:, :, 2 * j], z[:, :, 2 * j + 1] = r * np.cos(2 * np.pi * ub), r * np.sin(2 * np.pi * ub)
        rr[:, :, 2 * j] = rr[:, :, 2 * j + 1] = r
    return z.reshape(len(bs), per_image), rr.reshape(len(bs), per_image)


def augmentation_uniforms(seed, offset, B):
    """u [5, B] float32: u0..u3 from group 0xFFFFFFFE, u4 from word 0 of group 0xFFFFFFFD"""
    b = np.arange(B)
    return np.stack([uniform24(w) for w in block(seed, offset, b, G_AUG)] + [uniform24(block(seed, offset, b, G_APPLY)[0])])


def shift_scale_rotate64(u, shift_limit, scale_limit, rotate_limit, p, H, W):
    """ShiftScaleRotate.draw / .theta (train_deep_fake/lit_module.py) in float64 from the uniforms: (theta, apply)"""
    u = u.astype(np.float64)
    angle, scale = (2 * u[0] - 1) * rotate_limit, 1 + (2 * u[1] - 1) * scale_limit
    dx, dy = (2 * u[2] - 1) * shift_limit, (2 * u[3] - 1) * shift_limit
    a = angle * (math.pi / 180.0)
    cos, sin = np.cos(a) / scale, np.sin(a) / scale
    a11, a12, a21, a22 = cos, -sin * (H / W), sin * (W / H), cos
    t1, t2 = -2.0 * (a11 * dx + a12 * dy), -2.0 * (a21 * dx + a22 * dy)
    return np.stack([np.stack([a11, a12, t1], 1), np.stack([a21, a22, t2], 1)], 1), u[4] < p


def random_affine64(u, degrees, translate, scale):
    """RandomAffine.forward (train_denoiser/lit_module.py) in float64 from the uniforms: theta (always applied)"""
    u = u.astype(np.float64)
    ang = (2 * u[0] - 1) * math.radians(degrees)
    sc = u[1] * (scale[1] - scale[0]) + scale[0]
    tx, ty = (2 * u[2] - 1) * translate[0] * 2, (2 * u[3] - 1) * translate[1] * 2
    cos, sin = np.cos(ang) / sc, np.sin(ang) / sc
    return np.stack([np.stack([cos, -sin, tx], 1), np.stack([sin, cos, ty], 1)], 1)
