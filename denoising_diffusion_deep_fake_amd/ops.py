"""Thin torch-tensor wrappers over the single-operator entry points of libd3f_hip.so.

Activations are NHWC torch tensors ([B, H, W, C], C padded to 4 for f32 / 8 for bf16) that live
on the HIP device; weights are the f32 torch-layout masters.  These wrappers exist for the
parity tests and for callers that want one kernel at a time; the training path goes through
`Unet` (one C call per forward / backward).  No fallbacks: every function launches a HIP kernel.
"""
import ctypes as C
import math

import torch

from . import _lib
from ._lib import ConvDesc, check, ptr, stream_ptr

F32, BF16, F32X3 = _lib.F32, _lib.BF16, _lib.F32X3


def _tdtype(dtype):
    return torch.bfloat16 if dtype == BF16 else torch.float32


def _dev(t):
    if t.device.type != "cuda":
        raise _lib.D3FError("libd3f_hip ops need tensors on the HIP device (no CPU fallback)")
    return t.device


def make_desc(B, H, W, C0, C1, Cout, k, stride, pad, upsample0=False, cin_real=None):
    return ConvDesc(B, H, W, C0, C1, 1 if upsample0 else 0, Cout, k, k, stride, pad,
                    cin_real if cin_real is not None else C0 + C1)


def out_hw(d):
    return (d.H + 2 * d.pad - d.KH) // d.stride + 1, (d.W + 2 * d.pad - d.KW) // d.stride + 1


def nchw_to_nhwc(x, cpad, dtype=F32):
    B, Cc, H, W = x.shape
    out = torch.empty((B, H, W, cpad), dtype=_tdtype(dtype), device=_dev(x))
    check(_lib.lib().d3f_nchw_to_nhwc(dtype, ptr(x.contiguous().float()), ptr(out), B, Cc, H, W, cpad, stream_ptr()))
    return out


def nhwc_to_nchw(x, c, dtype=F32):
    B, H, W, cpad = x.shape
    out = torch.empty((B, c, H, W), dtype=torch.float32, device=_dev(x))
    check(_lib.lib().d3f_nhwc_to_nchw(dtype, ptr(x.contiguous()), ptr(out), B, c, H, W, cpad, stream_ptr()))
    return out


def head_activation_code(act):
    """D3F_ACT_* code of an activation given by code or by one of the names `Unet(activation=...)` accepts"""
    if isinstance(act, int) and not isinstance(act, bool):
        return act
    from .unet import canonical_activation
    return _lib.HEAD_ACTIVATIONS[canonical_activation(act)]


def head_activation_forward(act, z):
    """a = act(z) over the channel axis of z [B, C, H, W] f32 (C <= 16): the launch the engine makes behind the
    segmentation head's convolution"""
    z = z.contiguous().float()
    B, Cc, H, W = z.shape
    a = torch.empty_like(z)
    _dev(z)
    check(_lib.lib().d3f_head_activation_forward(head_activation_code(act), ptr(z), ptr(a), B, Cc, H, W, stream_ptr()))
    return a


def head_activation_backward(act, z, g, dtype=F32, cpad=None):
    """(z, g = d loss / d act(z)), both [B, C, H, W] f32 -> (dz NCHW f32, dY NHWC [B, H, W, cpad] in the storage dtype,
    rounded once from the f32 dz, padding channels zero): the launch at the head of the engine's backward pass"""
    z, g = z.contiguous().float(), g.contiguous().float()
    B, Cc, H, W = z.shape
    if g.shape != z.shape:
        raise ValueError(f"head_activation_backward: g {tuple(g.shape)} does not match z {tuple(z.shape)}")
    if cpad is None:
        ve = 8 if dtype == BF16 else 4
        cpad = (Cc + ve - 1) // ve * ve
    dz = torch.empty_like(z)
    dy = torch.empty((B, H, W, cpad), dtype=_tdtype(dtype), device=_dev(z))
    check(_lib.lib().d3f_head_activation_backward(head_activation_code(act), dtype, ptr(z), ptr(g), ptr(dz), ptr(dy),
                                                  B, Cc, H, W, cpad, stream_ptr()))
    return dz, dy


def pack_weights(d, w, dtype=F32, dgrad=True):
    L = _lib.lib()
    dev = _dev(w)
    wf = torch.empty(L.d3f_conv_packed_bytes(dtype, C.byref(d), 0), dtype=torch.uint8, device=dev)
    wd = torch.empty(L.d3f_conv_packed_bytes(dtype, C.byref(d), 1), dtype=torch.uint8, device=dev) if dgrad else None
    check(L.d3f_conv_pack_weights(dtype, C.byref(d), ptr(w.contiguous().float()), ptr(wf), ptr(wd), stream_ptr()))
    return wf, wd


def _conv_ws(d, dtype, which, dev, splitk):
    if not splitk:
        return None
    n = _lib.lib().d3f_conv_workspace_bytes(dtype, C.byref(d), which)
    return torch.empty(max(n, 16), dtype=torch.uint8, device=dev)


def conv_forward(d, src0, src1, wf, dtype=F32, want_stats=True, splitk=False):
    """splitk=True hands the kernel a workspace so small-M layers may split their K loop."""
    L = _lib.lib()
    ho, wo = out_hw(d)
    y = torch.empty((d.B, ho, wo, d.Cout), dtype=_tdtype(dtype), device=_dev(src0))
    ws = _conv_ws(d, dtype, 0, y.device, splitk)
    tiles = C.c_int()
    n = L.d3f_conv_stats_floats(dtype, C.byref(d), int(splitk), C.byref(tiles))
    stats = torch.zeros(n, dtype=torch.float32, device=y.device) if want_stats else None
    check(L.d3f_conv_forward(dtype, C.byref(d), ptr(src0), ptr(src1), ptr(wf), ptr(y), ptr(stats), ptr(ws),
                             stream_ptr()))
    return y, stats, tiles.value


def conv_winograd_applies(d, dtype=F32):
    """does the whole-network plan run this layer's forward as Winograd F(2x2, 3x3) (conv_winograd.hip)?"""
    return bool(_lib.lib().d3f_conv_winograd_applies(dtype, C.byref(d)))


def conv_winograd_pack(d, w):
    L = _lib.lib()
    n = L.d3f_conv_winograd_filter_bytes(C.byref(d))
    if n == 0:
        raise _lib.D3FError("conv_winograd_pack: the layer does not fit the Winograd kernel")
    u = torch.empty(n, dtype=torch.uint8, device=_dev(w))
    check(L.d3f_conv_winograd_pack(C.byref(d), ptr(w.contiguous().float()), ptr(u), stream_ptr()))
    return u


def conv_winograd_forward(d, src0, u, want_stats=True, scale=None, shift=None, residual=None, relu=False):
    """fp32 Winograd forward on its own.  scale / shift given: the eval epilogue relu?(y * scale + shift + residual?);
    else the raw conv output and one (sum, sumsq) statistics row per workgroup -> (y, stats, tiles)."""
    L = _lib.lib()
    y = torch.empty((d.B, d.H, d.W, d.Cout), dtype=torch.float32, device=_dev(src0))
    tiles = C.c_int()
    n = L.d3f_conv_winograd_stats_floats(C.byref(d), C.byref(tiles))
    stats = torch.zeros(n, dtype=torch.float32, device=y.device) if (want_stats and scale is None) else None
    check(L.d3f_conv_winograd_forward(C.byref(d), ptr(src0), ptr(u), ptr(y), ptr(stats), ptr(scale), ptr(shift),
                                      ptr(residual), int(relu), stream_ptr()))
    return y, stats, tiles.value


def conv_upsample_folded(d, dtype=F32):
    """does this conv(cat(upsample2x(src0), src1)) run with the up-sampling folded into pre-summed weights?"""
    return bool(d.upsample0) and bool(_lib.lib().d3f_conv_upsample_folded(dtype, C.byref(d)))


def conv_backward_data(d, dy, wd, dtype=F32, dx0=None, dx1=None, acc0=False, acc1=False, splitk=False, summed=None):
    """(dx0, dx1): gradients of src0 and src1.  For an up-sampled src0 (d.upsample0) dx0 is the gradient of the
    LOW-resolution tensor [B, H/2, W/2, C0] -- written directly by the folded 4x4 stride-2 kernel where the layer
    qualifies, else reduced here from the full-resolution gradient of the up-sampled operand.  summed=False keeps the
    full-resolution + d3f_upsample2x_backward route also where the launch could sum the 2x2 blocks itself."""
    dev = _dev(dy)
    ws = _conv_ws(d, dtype, 1, dev, splitk)
    folded = bool(d.upsample0) and bool(_lib.lib().d3f_conv_upsample_folded(dtype, C.byref(d)))
    # ... or summed 2x2 in the launch's own epilogue (the patch form of the bf16 16 -> 32 layer): low resolution too.
    # That form is opt-in (upsample0 = 2 in the descriptor): a C caller on the full-resolution contract keeps it.
    if bool(d.upsample0) and not folded and summed is not False and \
            bool(_lib.lib().d3f_conv_upsample_summed(dtype, C.byref(d))):
        d = ConvDesc(*[getattr(d, n) for n, _ in ConvDesc._fields_])
        d.upsample0 = 2
        folded = True
    low = (d.B, d.H // 2, d.W // 2, d.C0)
    if d.upsample0 and not folded:
        if acc0 or dx0 is not None:
            raise ValueError("conv_backward_data: an up-sampled source that is not folded takes no dx0 / acc0")
        full = torch.empty((d.B, d.H, d.W, d.C0), dtype=_tdtype(dtype), device=dev)
    elif dx0 is None:
        full = None
        dx0 = torch.empty(low if d.upsample0 else (d.B, d.H, d.W, d.C0), dtype=_tdtype(dtype), device=dev)
    else:
        full = None
    if dx1 is None and d.C1 > 0:
        dx1 = torch.empty((d.B, d.H, d.W, d.C1), dtype=_tdtype(dtype), device=dev)
    check(_lib.lib().d3f_conv_backward_data(dtype, C.byref(d), ptr(dy), ptr(wd), ptr(full if full is not None else dx0),
                                            ptr(dx1), int(acc0), int(acc1), ptr(ws), stream_ptr()))
    if full is not None:
        dx0 = upsample2x_backward(full, dtype)
    return dx0, dx1


def conv_backward_weight(d, dy, src0, src1, dtype=F32):
    L = _lib.lib()
    ws = torch.empty(L.d3f_conv_backward_weight_workspace_bytes(dtype, C.byref(d)), dtype=torch.uint8, device=_dev(dy))
    dw = torch.empty((d.Cout, d.CinReal, d.KH, d.KW), dtype=torch.float32, device=dy.device)
    check(L.d3f_conv_backward_weight(dtype, C.byref(d), ptr(dy), ptr(src0), ptr(src1), ptr(ws), ptr(dw), stream_ptr()))
    return dw


def bn_finalize(stats, tiles, Cc, count, gamma, beta, running_mean=None, running_var=None):
    coef = torch.empty(4 * Cc, dtype=torch.float32, device=_dev(stats))
    check(_lib.lib().d3f_bn_finalize(ptr(stats), tiles, Cc, count, ptr(gamma), ptr(beta), ptr(running_mean),
                                     ptr(running_var), ptr(coef), stream_ptr()))
    return coef


def bn_apply(y, coef, residual=None, relu=True, dtype=F32):
    Cc = y.shape[-1]
    out = torch.empty_like(y)
    check(_lib.lib().d3f_bn_apply(dtype, ptr(y), ptr(coef), Cc, y.numel() // Cc, ptr(residual), int(relu),
                                  ptr(out), stream_ptr()))
    return out


def bn_backward(dA, a, y, coef, gamma, want_dres=False, dtype=F32):
    L = _lib.lib()
    Cc = y.shape[-1]
    rows = y.numel() // Cc
    ws = torch.empty(L.d3f_bn_backward_workspace_bytes(dtype, Cc, rows), dtype=torch.uint8, device=_dev(y))
    dy = torch.empty_like(y)
    dres = torch.empty_like(y) if want_dres else None
    dgamma = torch.empty(Cc, dtype=torch.float32, device=y.device)
    dbeta = torch.empty(Cc, dtype=torch.float32, device=y.device)
    check(L.d3f_bn_backward(dtype, ptr(dA), ptr(a), ptr(y), ptr(coef), ptr(gamma), Cc, rows, ptr(dy), ptr(dres),
                            ptr(dgamma), ptr(dbeta), ptr(ws), stream_ptr()))
    return dy, dres, dgamma, dbeta


def bn_desc(C_, rows, dtype=F32, cpad=None, apply=True, relu=True, res=0, mask=0, fwd_rows=0, fused_rows=0,
            allow_fused=True, plan_nets=1):
    """a BatchNorm layer description (d3f_bn_desc).  res: 0 none, 1 a tensor, 2 another layer's y with its coefficient
    block; mask: 0 none, 1 recomputed from y, 2 read from a"""
    return _lib.BnDesc(dtype, C_, C_ if cpad is None else cpad, rows, int(apply), int(relu), res, mask, fwd_rows,
                       fused_rows, int(allow_fused), plan_nets)


def bn_layer_plan(d):
    """the plan of a description (host only: needs no GPU)"""
    p = _lib.BnPlan()
    check(_lib.lib().d3f_bn_layer_plan(C.byref(d), C.byref(p)))
    return p


def bn_layer_forward(d, stats, gamma, beta, coef, y, a=None, res=None, res_coef=None, running_mean=None,
                     running_var=None):
    """one forward pass of the layer in its planned form, on the caller's buffers (nothing is allocated here)"""
    check(_lib.lib().d3f_bn_layer_forward(C.byref(d), ptr(stats), ptr(gamma), ptr(beta), ptr(running_mean),
                                          ptr(running_var), ptr(coef), ptr(y), ptr(res), ptr(res_coef), ptr(a),
                                          stream_ptr()))


def bn_layer_backward(d, partial, gamma, coef, y, dA, dy, a=None, dres=None, dres_acc=False, dgamma=None, dbeta=None):
    """one backward pass of the layer in its planned form, on the caller's buffers"""
    check(_lib.lib().d3f_bn_layer_backward(C.byref(d), ptr(partial), ptr(gamma), ptr(coef), ptr(y), ptr(a), ptr(dA),
                                           ptr(dy), ptr(dres), int(dres_acc), ptr(dgamma), ptr(dbeta), stream_ptr()))


def maxpool_forward(x, dtype=F32):
    B, H, W, Cc = x.shape
    out = torch.empty((B, H // 2, W // 2, Cc), dtype=x.dtype, device=_dev(x))
    idx = torch.empty((B, H // 2, W // 2, Cc), dtype=torch.uint8, device=x.device)
    check(_lib.lib().d3f_maxpool3x3s2_forward(dtype, ptr(x), ptr(out), ptr(idx), B, H, W, Cc, stream_ptr()))
    return out, idx


def maxpool_backward(dout, idx, H, W, dtype=F32, din=None):
    B, _, _, Cc = dout.shape
    acc = din is not None
    if din is None:
        din = torch.empty((B, H, W, Cc), dtype=dout.dtype, device=_dev(dout))
    check(_lib.lib().d3f_maxpool3x3s2_backward(dtype, ptr(dout), ptr(idx), ptr(din), int(acc), B, H, W, Cc, stream_ptr()))
    return din


def upsample2x_backward(dfull, dtype=F32):
    B, H, W, Cc = dfull.shape
    out = torch.empty((B, H // 2, W // 2, Cc), dtype=dfull.dtype, device=_dev(dfull))
    check(_lib.lib().d3f_upsample2x_backward(dtype, ptr(dfull), ptr(out), B, H // 2, W // 2, Cc, stream_ptr()))
    return out


def affine_warp(x, theta):
    """affine_grid + grid_sample(bilinear, zeros, align_corners=False) of NCHW f32 images, theta [B, 2, 3]."""
    x = x.contiguous().float()
    B, Cc, H, W = x.shape
    theta = theta.to(device=_dev(x), dtype=torch.float32).contiguous()
    if theta.shape != (B, 2, 3):
        raise ValueError(f"theta must be [{B}, 2, 3], got {list(theta.shape)}")
    out = torch.empty_like(x)
    check(_lib.lib().d3f_affine_warp(ptr(x), ptr(theta), ptr(out), B, Cc, H, W, stream_ptr()))
    return out


def _affine_rng_params(kind, params):
    kinds = {"random_affine": 0, "shift_scale_rotate": 1}
    kind = kinds.get(kind, kind)
    if kind not in (0, 1):
        raise ValueError(f"kind must be one of {sorted(kinds)} (or 0 / 1), got {kind!r}")
    params = [float(v) for v in params]
    if len(params) != (5 if kind == 0 else 4):
        raise ValueError("params: (degrees, translate_x, translate_y, scale_lo, scale_hi) for random_affine, "
                         "(shift_limit, scale_limit, rotate_limit, p) for shift_scale_rotate")
    return kind, (C.c_float * 5)(*(params + [0.0] * (5 - len(params))))


def affine_warp_rng(x, seed, offset, kind, params):
    """affine_warp with its per-image parameters drawn inside the kernel (d3f_affine_warp_rng; csrc/philox.h has the draw
    layout).  kind "random_affine": params (degrees, translate_x, translate_y, scale_lo, scale_hi), every image warped;
    kind "shift_scale_rotate": params (shift_limit, scale_limit, rotate_limit, p), an image is warped with probability p
    and copied otherwise."""
    x = x.contiguous().float()
    B, Cc, H, W = x.shape
    kind, cparams = _affine_rng_params(kind, params)
    out = torch.empty_like(x)
    check(_lib.lib().d3f_affine_warp_rng(ptr(x), ptr(out), int(seed), int(offset), kind, cparams, B, Cc, H, W,
                                         stream_ptr()))
    return out


def affine_theta_draw(seed, offset, kind, params, B, H, W, device="cuda"):
    """the (theta [B, 2, 3] f32, apply [B] bool) affine_warp_rng uses for the same arguments"""
    kind, cparams = _affine_rng_params(kind, params)
    theta = torch.empty((B, 2, 3), dtype=torch.float32, device=device)
    apply = torch.empty(B, dtype=torch.uint8, device=device)
    _dev(theta)
    check(_lib.lib().d3f_affine_theta_draw(int(seed), int(offset), kind, cparams, ptr(theta), ptr(apply), B, H, W,
                                           stream_ptr()))
    return theta, apply.bool()


def u8rgb_normalise(frames, mean, std):
    """uint8 RGB [B, H, W, 3] on the HIP device -> normalised NCHW float32 ((u8 / 255 - mean) / std per channel): the
    host transform NormalizeToTensor bit for bit (d3f_u8rgb_normalise)"""
    if frames.dtype != torch.uint8 or frames.dim() != 4 or frames.shape[-1] != 3:
        raise ValueError("u8rgb_normalise expects uint8 frames [B, H, W, 3] (RGB)")
    frames = frames.contiguous()
    B, H, W, _ = frames.shape
    out = torch.empty((B, 3, H, W), dtype=torch.float32, device=_dev(frames))
    m = (C.c_float * 3)(*[float(v) for v in mean])
    s = (C.c_float * 3)(*[float(v) for v in std])
    check(_lib.lib().d3f_u8rgb_normalise(ptr(frames), ptr(out), B, H, W, m, s, stream_ptr()))
    return out


def _pool_batch_args(pool, index, mean, std):
    if pool.dtype != torch.uint8 or pool.dim() != 4 or pool.shape[-1] != 3 or not pool.is_contiguous():
        raise ValueError("pool_batch expects a contiguous uint8 pool [N, H, W, 3] (RGB)")
    dev = _dev(pool)
    if index.dtype != torch.int64 or index.dim() != 1 or index.device != dev:
        raise ValueError("pool_batch expects an int64 index [B] on the pool's device")
    N, H, W, _ = pool.shape
    out = torch.empty((index.shape[0], 3, H, W), dtype=torch.float32, device=dev)
    m = (C.c_float * 3)(*[float(v) for v in mean])
    s = (C.c_float * 3)(*[float(v) for v in std])
    return index.contiguous(), out, m, s


def pool_batch(pool, index, mean, std, theta=None, apply=None):
    """a training batch from a device-resident pool [N, H, W, 3] uint8 in one launch (d3f_pool_batch): gather by index [B]
    (int64, on the device), u8rgb_normalise, and with theta [B, 2, 3] affine_warp of the images whose apply [B] (bool /
    uint8; None: all) is set -- bit for bit torch.where(apply, affine_warp(x, theta), x) of x = u8rgb_normalise(pool[index]).
    An index outside [0, N) gives an all-NaN image."""
    index, out, m, s = _pool_batch_args(pool, index, mean, std)
    N, H, W, _ = pool.shape
    B = index.shape[0]
    if theta is not None:
        theta = theta.to(device=pool.device, dtype=torch.float32).contiguous()
        if theta.shape != (B, 2, 3):
            raise ValueError(f"theta must be [{B}, 2, 3], got {list(theta.shape)}")
    if apply is not None:
        if theta is None:
            raise ValueError("pool_batch: apply without theta")
        if apply.dtype == torch.bool:
            apply = apply.view(torch.uint8) if apply.is_contiguous() else apply.to(torch.uint8)
        apply = apply.to(device=pool.device, dtype=torch.uint8).contiguous()
        if apply.shape != (B,):
            raise ValueError(f"apply must be [{B}], got {list(apply.shape)}")
    check(_lib.lib().d3f_pool_batch(ptr(pool), N, ptr(index), ptr(out), B, H, W, m, s, ptr(theta), ptr(apply),
                                    stream_ptr()))
    return out


def pool_batch_rng(pool, index, mean, std, seed, offset, kind, params):
    """pool_batch with the augmentation of affine_warp_rng (same kinds, params and draws) instead of a given theta
    (d3f_pool_batch_rng): bit for bit affine_warp_rng(u8rgb_normalise(pool[index]), seed, offset, kind, params)"""
    index, out, m, s = _pool_batch_args(pool, index, mean, std)
    N, H, W, _ = pool.shape
    kind, cparams = _affine_rng_params(kind, params)
    check(_lib.lib().d3f_pool_batch_rng(ptr(pool), N, ptr(index), ptr(out), index.shape[0], H, W, m, s, int(seed),
                                        int(offset), kind, cparams, stream_ptr()))
    return out


def _balance_table_args(members, class_start, dev):
    for name, t in (("members", members), ("class_start", class_start)):
        if t.dtype != torch.int64 or t.dim() != 1 or t.device != dev or not t.is_contiguous():
            raise ValueError(f"balanced sampling expects {name} as a contiguous int64 vector on {dev}")
    if class_start.shape[0] < 2:
        raise ValueError("balanced sampling: class_start [Kn + 1] names no class (Kn == 0)")
    return class_start.shape[0] - 1


def pool_batch_balanced_rng(pool, members, class_start, B, mean, std, seed, offset, kind, params=None):
    """pool_batch_rng with the B indices drawn inside the launch from a balance table (d3f_pool_batch_balanced_rng;
    DeviceImagePool.balance_table builds members [M] and class_start [Kn + 1]): every non-empty class with equal probability,
    every image of a class with equal probability, with replacement.  kind as pool_batch_rng, or "none" (params ignored): no
    augmentation.  Returns (batch [B, 3, H, W], index [B] int64) with batch bit for bit pool_batch_rng(pool, index, ...) and
    index = balanced_index_draw(members, class_start, seed, offset, B)."""
    if pool.dtype != torch.uint8 or pool.dim() != 4 or pool.shape[-1] != 3 or not pool.is_contiguous():
        raise ValueError("pool_batch expects a contiguous uint8 pool [N, H, W, 3] (RGB)")
    dev = _dev(pool)
    Kn = _balance_table_args(members, class_start, dev)
    N, H, W, _ = pool.shape
    B = int(B)
    out = torch.empty((B, 3, H, W), dtype=torch.float32, device=dev)
    index = torch.empty(B, dtype=torch.int64, device=dev)
    m = (C.c_float * 3)(*[float(v) for v in mean])
    s = (C.c_float * 3)(*[float(v) for v in std])
    if kind in ("none", None, _lib.AUGMENT_NONE):
        kind, cparams = _lib.AUGMENT_NONE, None
    else:
        kind, cparams = _affine_rng_params(kind, params)
    check(_lib.lib().d3f_pool_batch_balanced_rng(ptr(pool), N, ptr(members), ptr(class_start), Kn, ptr(out), ptr(index), B, H,
                                                 W, m, s, int(seed), int(offset), kind, cparams, stream_ptr()))
    return out, index


def balanced_index_draw(members, class_start, seed, offset, B):
    """the index [B] int64 pool_batch_balanced_rng draws for the same table, seed and offset (d3f_balanced_index_draw)"""
    dev = _dev(members)
    Kn = _balance_table_args(members, class_start, dev)
    index = torch.empty(int(B), dtype=torch.int64, device=dev)
    check(_lib.lib().d3f_balanced_index_draw(ptr(members), ptr(class_start), Kn, int(seed), int(offset), ptr(index), int(B),
                                             stream_ptr()))
    return index


def noise_blend(x, noise, y_uniform, lam, return_r=False):
    x = x.contiguous().float()
    out = torch.empty_like(x)
    B = x.shape[0]
    r = torch.empty(B, dtype=torch.float32, device=_dev(x)) if return_r else None
    check(_lib.lib().d3f_noise_blend(ptr(x), ptr(noise.contiguous().float()), ptr(y_uniform.contiguous().float()),
                                     float(lam), ptr(out), ptr(r), B, x.numel() // max(B, 1), stream_ptr()))
    return (out, r) if return_r else out


def noise_blend_fixed(x, noise, ratio):
    """sqrt(1-r)*x + sqrt(r)*noise with one ratio for every image (float) or a per-image tensor [B]."""
    x = x.contiguous().float()
    B = x.shape[0]
    r = ratio if torch.is_tensor(ratio) else torch.ones(B, device=_dev(x)) * float(ratio)
    r = r.to(device=_dev(x), dtype=torch.float32).reshape(-1).contiguous()
    out = torch.empty_like(x)
    check(_lib.lib().d3f_noise_blend_fixed(ptr(x), ptr(noise.contiguous().float()), ptr(r), ptr(out), B,
                                           x.numel() // max(B, 1), stream_ptr()))
    return out


def noise_blend_rng(x, seed, offset, lam, return_r=False):
    """noise_blend with its normals and its per-image uniform drawn inside the kernel: no noise tensor exists"""
    x = x.contiguous().float()
    out = torch.empty_like(x)
    B = x.shape[0]
    r = torch.empty(B, dtype=torch.float32, device=_dev(x)) if return_r else None
    check(_lib.lib().d3f_noise_blend_rng(ptr(x), int(seed), int(offset), float(lam), ptr(out), ptr(r), B,
                                         x.numel() // max(B, 1), stream_ptr()))
    return (out, r) if return_r else out


def noise_blend_fixed_rng(x, seed, offset, ratio):
    """noise_blend_fixed with its normals drawn inside the kernel"""
    x = x.contiguous().float()
    B = x.shape[0]
    r = ratio if torch.is_tensor(ratio) else torch.ones(B, device=_dev(x)) * float(ratio)
    r = r.to(device=_dev(x), dtype=torch.float32).reshape(-1).contiguous()
    out = torch.empty_like(x)
    check(_lib.lib().d3f_noise_blend_fixed_rng(ptr(x), int(seed), int(offset), ptr(r), ptr(out), B,
                                               x.numel() // max(B, 1), stream_ptr()))
    return out


def noise_blend_fixed_index_rng(x, seed, offset, ratio, index):
    """noise_blend_fixed_rng with the counter's image word taken from index[b] instead of b: the draws of image b depend on
    (seed, offset, index[b]) alone, so a held-out image meets the same noise in any batch.  index: [B] int64; a host
    tensor or a sequence is checked here (every value in [0, 2**32), else ValueError) and moved to the device; a device
    tensor is not read back -- an image whose index is outside the range comes out as NaN.  With index = arange(B) the
    result is noise_blend_fixed_rng's bit for bit.  (include/d3f_hip.h: d3f_noise_blend_fixed_index_rng)"""
    B = x.shape[0]
    if not torch.is_tensor(index):
        index = torch.as_tensor(index, dtype=torch.int64)
    if index.dtype != torch.int64 or index.numel() != B:
        raise ValueError(f"index must be an int64 tensor of {B} entries")
    if index.device.type != "cuda" and B and (int(index.min()) < 0 or int(index.max()) >= 1 << 32):
        raise ValueError("noise_blend_fixed_index_rng: an index outside [0, 2**32) names no counter")  # the host can see it
    x = x.contiguous().float()
    dev = _dev(x)
    index = index.to(dev).reshape(-1).contiguous()
    r = ratio if torch.is_tensor(ratio) else torch.ones(B, device=dev) * float(ratio)
    r = r.to(device=dev, dtype=torch.float32).reshape(-1).contiguous()
    out = torch.empty_like(x)
    check(_lib.lib().d3f_noise_blend_fixed_index_rng(ptr(x), int(seed), int(offset), ptr(r), ptr(index), ptr(out), B,
                                                     x.numel() // max(B, 1), stream_ptr()))
    return out


def noise_draw(seed, offset, shape, device="cuda", noise=True, y=True):
    """the draws noise_blend_rng / noise_blend_fixed_rng make for a batch of this shape: (noise [shape] or None, y [B] or
    None)"""
    shape = tuple(int(v) for v in shape)
    B = shape[0]
    per_image = 1
    for v in shape[1:]:
        per_image *= v
    n = torch.empty(shape, dtype=torch.float32, device=device) if noise else None
    yy = torch.empty(B, dtype=torch.float32, device=device) if y else None
    _dev(n if n is not None else yy)
    check(_lib.lib().d3f_noise_draw(int(seed), int(offset), ptr(n), ptr(yy), B, per_image, stream_ptr()))
    return n, yy


def philox4x32_10(counter, key):
    """one Philox4x32-10 block on the host: counter 4 and key 2 uint32 words -> 4 uint32 words"""
    c = (C.c_uint32 * 4)(*[int(v) & 0xFFFFFFFF for v in counter])
    k = (C.c_uint32 * 2)(*[int(v) & 0xFFFFFFFF for v in key])
    out = (C.c_uint32 * 4)()
    check(_lib.lib().d3f_philox4x32_10(c, k, out))
    return tuple(int(v) for v in out)


def l1_per_image(pred, target):
    """mean |pred - target| over each image: [B] f32."""
    L = _lib.lib()
    pred, target = pred.contiguous().float(), target.contiguous().float()
    B = pred.shape[0]
    ws = torch.empty(L.d3f_l1_per_image_workspace_bytes(B), dtype=torch.uint8, device=_dev(pred))
    out = torch.empty(B, dtype=torch.float32, device=pred.device)
    check(L.d3f_l1_per_image(ptr(pred), ptr(target), ptr(out), ptr(ws), B, pred.numel() // max(B, 1), stream_ptr()))
    return out


def l1_per_image_scatter(pred, target, index, scores):
    """scores[index[b]] = l1_per_image(pred, target)[b], bit for bit, without leaving the device: index [B] int64 and scores
    [N] contiguous f32 on the HIP device (a slice of a larger buffer will do).  An index outside [0, N) writes nothing;
    entries no index names keep their value.  Returns scores.  (include/d3f_hip.h: d3f_l1_per_image_scatter)"""
    L = _lib.lib()
    pred, target = pred.contiguous().float(), target.contiguous().float()
    dev = _dev(pred)
    B = pred.shape[0]
    if scores.dtype != torch.float32 or scores.dim() != 1 or scores.device != dev or not scores.is_contiguous():
        raise ValueError("scores must be a contiguous 1-D float32 tensor on the device of pred")
    if index.dtype != torch.int64 or index.device != dev or index.numel() != B:
        raise ValueError(f"index must be an int64 tensor of {B} entries on the device of pred")
    if B == 0:
        return scores
    index = index.reshape(-1).contiguous()
    ws = torch.empty(L.d3f_l1_per_image_workspace_bytes(B), dtype=torch.uint8, device=dev)
    check(L.d3f_l1_per_image_scatter(ptr(pred), ptr(target), ptr(index), ptr(scores), scores.numel(), ptr(ws), B,
                                     pred.numel() // B, stream_ptr()))
    return scores


def _out_or_new(out, shape, dtype, dev, what):
    if out is None:
        return torch.empty(shape, dtype=dtype, device=dev)
    if tuple(out.shape) != tuple(shape) or out.dtype != dtype or out.device != dev or not out.is_contiguous():
        raise ValueError(f"{what} must be a contiguous {dtype} tensor of shape {tuple(shape)} on the input's device")
    return out


def difficulty_classes(scores, number_of_classes, out=None):
    """compute_difficulty_index_for_each_loss of the balance LitModule over a device score buffer [N] f32 in which NaN
    means "not scored": (classes [N] int64, -1 where not scored; counts [number_of_classes] int32; minmax [2] f32).  The
    reference's fp32 arithmetic operation for operation, except that max == min gives class 0.  out: the three tensors to
    write into.  (include/d3f_hip.h: d3f_difficulty_classes)"""
    L = _lib.lib()
    dev = _dev(scores)
    if scores.dtype != torch.float32 or scores.dim() != 1 or not scores.is_contiguous():
        raise ValueError("scores must be a contiguous 1-D float32 tensor")
    N, nc = scores.numel(), int(number_of_classes)
    classes, counts, minmax = out if out is not None else (None, None, None)
    classes = _out_or_new(classes, (N,), torch.int64, dev, "classes")
    counts = _out_or_new(counts, (max(nc, 0),), torch.int32, dev, "counts")
    minmax = _out_or_new(minmax, (2,), torch.float32, dev, "minmax")
    ws = torch.empty(L.d3f_difficulty_classes_workspace_bytes(N), dtype=torch.uint8, device=dev)
    check(L.d3f_difficulty_classes(ptr(scores), N, nc, ptr(classes), ptr(counts), ptr(minmax), ptr(ws), stream_ptr()))
    return classes, counts, minmax


def difficulty_histogram_u8(classes, bins=10, size=(480, 640), out=None):
    """what axes.hist(difficulty_index) of the balance LitModule computes, and a chart of it: classes [N] int64 on the HIP
    device (entries < 0 passed over) -> (bin_counts [bins] int32 and range [2] f64 as numpy.histogram(x, bins) gives them,
    chart [H, W, 3] uint8).  bins = 10 and size = (480, 640) are matplotlib's defaults.  out: the three tensors to write
    into.  (include/d3f_hip.h: d3f_difficulty_histogram_u8)"""
    L = _lib.lib()
    dev = _dev(classes)
    if classes.dtype != torch.int64 or classes.dim() != 1 or not classes.is_contiguous():
        raise ValueError("classes must be a contiguous 1-D int64 tensor")
    N, bins, H, W = classes.numel(), int(bins), int(size[0]), int(size[1])
    bin_counts, rng_, chart = out if out is not None else (None, None, None)
    bin_counts = _out_or_new(bin_counts, (max(bins, 0),), torch.int32, dev, "bin_counts")
    rng_ = _out_or_new(rng_, (2,), torch.float64, dev, "range")
    chart = _out_or_new(chart, (max(H, 0), max(W, 0), 3), torch.uint8, dev, "chart")
    ws = torch.empty(L.d3f_difficulty_histogram_u8_workspace_bytes(N), dtype=torch.uint8, device=dev)
    check(L.d3f_difficulty_histogram_u8(ptr(classes), N, bins, ptr(bin_counts), ptr(rng_), ptr(chart), H, W, ptr(ws),
                                        stream_ptr()))
    return bin_counts, rng_, chart


def mse_ssim_loss(pred, target, in_min=-1.0, in_max=1.0):
    """returns (loss[3] = {loss, mse, ssim} device tensor, grad wrt pred)."""
    L = _lib.lib()
    B, Cc, H, W = pred.shape
    if Cc != 3:
        raise ValueError("SSIM is defined for 3-channel images (piqa n_channels=3)")
    pred = pred.contiguous().float()
    target = target.contiguous().float()
    ws = torch.empty(L.d3f_mse_ssim_loss_workspace_bytes(B, H, W), dtype=torch.uint8, device=_dev(pred))
    out = torch.empty(3, dtype=torch.float32, device=pred.device)
    grad = torch.empty_like(pred)
    check(L.d3f_mse_ssim_loss(ptr(pred), ptr(target), float(in_min), float(in_max), ptr(out), ptr(grad), ptr(ws),
                              B, H, W, stream_ptr()))
    return out, grad


QUALITY_ROWS = ("mse", "ssim", "psnr", "loss")  # the rows of quality_per_image's result


def quality_per_image(pred, target, lo=-1.0, hi=1.0, index=None, out=None, N=None):
    """the criterion's terms per image, forward only: [4, N] f32 with rows QUALITY_ROWS, image b's values at column
    index[b] (int64 on the device), or at column b when index is None (then N defaults to B).  out: a contiguous [4, N] f32
    device tensor to scatter into -- columns no index names keep their value, an index outside [0, N) writes nothing;
    without out the result starts as NaN.  An image's values do not depend on the batch it is scored in.  Refused before
    any device call: images smaller than 11 x 11, hi <= lo, N < 1.  (include/d3f_hip.h: d3f_quality_per_image_scatter)"""
    if pred.dim() != 4 or pred.shape[1] != 3 or pred.shape != target.shape:
        raise ValueError("quality_per_image expects prediction and target of one shape [B, 3, H, W] (piqa n_channels=3)")
    B, _, H, W = pred.shape
    if H < 11 or W < 11:
        raise ValueError(f"quality_per_image: image {H}x{W} smaller than the 11x11 SSIM window")
    if not float(hi) > float(lo):
        raise ValueError("quality_per_image: hi must be above lo")
    if N is None:
        N = out.shape[-1] if out is not None else B
    N = int(N)
    if N < 1:
        raise ValueError(f"quality_per_image: N = {N}")
    if index is not None and (index.dtype != torch.int64 or index.numel() != B):
        raise ValueError(f"index must be an int64 tensor of {B} entries")
    L = _lib.lib()
    pred, target = pred.contiguous().float(), target.contiguous().float()
    dev = _dev(pred)
    if out is None:
        out = torch.full((4, N), float("nan"), dtype=torch.float32, device=dev)
    elif tuple(out.shape) != (4, N) or out.dtype != torch.float32 or out.device != dev or not out.is_contiguous():
        raise ValueError(f"out must be a contiguous float32 tensor of shape (4, {N}) on the device of pred")
    if B == 0:
        return out
    if index is not None:
        index = index.to(dev).reshape(-1).contiguous()
    ws = torch.empty(L.d3f_quality_per_image_workspace_bytes(B, H, W), dtype=torch.uint8, device=dev)
    check(L.d3f_quality_per_image_scatter(ptr(pred), ptr(target), float(lo), float(hi), ptr(index), ptr(out), N, ptr(ws),
                                          B, H, W, stream_ptr()))
    return out


def adam_step(p, g, m, v, lr, beta1, beta2, eps, step, grad_scale=1.0):
    check(_lib.lib().d3f_adam_step(ptr(p), ptr(g), ptr(m), ptr(v), p.numel(), lr, beta1, beta2, eps, step,
                                   grad_scale, stream_ptr()))


def ema_lerp(ema, online, weight):
    check(_lib.lib().d3f_ema_lerp(ptr(ema), ptr(online), ema.numel(), float(weight), stream_ptr()))


def center_crop_box(h, w, width, height):
    """crop_image_at_center of the script tools (d3f/script_tools/put_video_through_fake_model.py:121-138): the largest
    centred box of the target aspect inside an h x w frame, as (x1, y1, crop_width, crop_height) -- the reference's float
    division and int() truncation, kept in Python"""
    width_scale = w / width
    height_scale = h / height
    scale = min(width_scale, height_scale)
    crop_width = int(width * scale)
    crop_height = int(height * scale)
    x1 = (w - crop_width) // 2
    y1 = (h - crop_height) // 2
    return x1, y1, crop_width, crop_height


TRACK_MARGIN = 1.6  # a design choice, not a measurement: how much wider than the detector's box the crop is cut


def track_crop_box(h, w, width, height, face, margin=TRACK_MARGIN):
    """the crop box of the target aspect (width x height) around a detector's box face = (fx, fy, fw, fh) in an h x w frame,
    as (x1, y1, crop_width, crop_height): `margin` times the face on the axis that needs the larger scale, capped by
    `center_crop_box`'s own scale -- so the box always fits -- and moved inside the frame.  The face may stick out of the
    frame.  The scale in Python floats with int() truncation, as `center_crop_box`; the position in integers."""
    fx, fy, fw, fh = [int(v) for v in face]
    if fw <= 0 or fh <= 0:
        raise ValueError(f"track_crop_box: face extent {fw} x {fh} is not positive")
    s = max(fw / width, fh / height) * margin
    s = min(s, w / width, h / height)
    cw = max(int(width * s), 1)
    ch = max(int(height * s), 1)
    x1 = min(max((2 * fx + fw - cw) // 2, 0), w - cw)
    y1 = min(max((2 * fy + fh - ch) // 2, 0), h - ch)
    return x1, y1, cw, ch


def read_box_track(path):
    """a detector's track file -> a list of boxes (fx, fy, fw, fh), entry k for frame k.  A line is four integers `x y w h`
    separated by blanks or commas; `#` starts a comment; blank lines are skipped; a lone `-` is a frame without a
    detection.  A gap takes the previous detection, leading gaps the first one; a file without any detection is a
    ValueError.  (Frames past the last line keep the last box: `box_of_frame`.)"""
    faces = []
    with open(path) as f:
        for number, line in enumerate(f, 1):
            fields = line.split("#", 1)[0].replace(",", " ").split()
            if not fields:
                continue
            if fields == ["-"]:
                faces.append(None)
                continue
            try:
                if len(fields) != 4:
                    raise ValueError
                faces.append(tuple(int(v) for v in fields))
            except ValueError:
                raise ValueError(f"{path}, line {number}: expected four integers `x y w h` or `-`, "
                                 f"got {line.strip()!r}") from None
    first = next((face for face in faces if face is not None), None)
    if first is None:
        raise ValueError(f"{path}: no detection in the track")
    last = first
    for k, face in enumerate(faces):
        if face is None:
            faces[k] = last
        else:
            last = face
    return faces


def smooth_box_track(faces, n):
    """a centred moving average over up to 2 n + 1 entries of a track (the window is truncated at both ends): the mean of
    (2 fx + fw, 2 fy + fh, fw, fh) in integers with floor division, turned back into (fx, fy, fw, fh).  n = 0 returns its
    input.  A detector's jitter otherwise becomes crop jitter, which the temporal filter reads as motion."""
    n = int(n)
    if n < 0:
        raise ValueError(f"smooth_box_track: n = {n} is negative")
    if n == 0:
        return list(faces)
    faces = [tuple(int(v) for v in face) for face in faces]
    out = []
    for k in range(len(faces)):
        window = faces[max(k - n, 0):k + n + 1]
        m = len(window)
        cx2 = sum(2 * fx + fw for fx, _, fw, _ in window) // m
        cy2 = sum(2 * fy + fh for _, fy, _, fh in window) // m
        fw = sum(face[2] for face in window) // m
        fh = sum(face[3] for face in window) // m
        out.append(((cx2 - fw) // 2, (cy2 - fh) // 2, fw, fh))
    return out


def angle_hundredths(angle_degrees):
    """an angle in degrees -> integer hundredths of a degree, wrapped to (-18000, 18000]"""
    a = float(angle_degrees)
    if not math.isfinite(a):
        raise ValueError(f"angle {angle_degrees!r} is not a finite number of degrees")
    h = int(round(a * 100.0)) % 36000
    return h - 36000 if h > 18000 else h


def box_rotation(angle_degrees):
    """(c16, s16) = (round(cos a * 65536), round(sin a * 65536)) of an angle in degrees, first rounded to hundredths of a degree
    and wrapped to (-180, 180]: the rotation of a box as the _rboxes_ operators take it (include/d3f_hip.h; the device does
    no trigonometry).  x right, y down: a positive angle turns the box clockwise on the screen about its centre."""
    a = math.radians(angle_hundredths(angle_degrees) / 100.0)
    return int(round(math.cos(a) * 65536.0)), int(round(math.sin(a) * 65536.0))


def read_rbox_track(path):
    """`read_box_track` for a track with head roll -> a list of (fx, fy, fw, fh, a), entry k for frame k.  A line is
    `x y w h` or `x y w h a` with a the box's angle in decimal degrees (`box_rotation`'s convention; a missing a is 0; it is
    rounded to hundredths and wrapped to (-180, 180]); comments, blank lines, `-` and gaps as in `read_box_track`, which
    itself keeps refusing a fifth field."""
    faces = []
    with open(path) as f:
        for number, line in enumerate(f, 1):
            fields = line.split("#", 1)[0].replace(",", " ").split()
            if not fields:
                continue
            if fields == ["-"]:
                faces.append(None)
                continue
            try:
                if len(fields) not in (4, 5):
                    raise ValueError
                angle = angle_hundredths(fields[4]) / 100.0 if len(fields) == 5 else 0.0
                faces.append(tuple(int(v) for v in fields[:4]) + (angle,))
            except ValueError:
                raise ValueError(f"{path}, line {number}: expected `x y w h` (integers), `x y w h a` (a in degrees) or `-`, "
                                 f"got {line.strip()!r}") from None
    first = next((face for face in faces if face is not None), None)
    if first is None:
        raise ValueError(f"{path}: no detection in the track")
    last = first
    for k, face in enumerate(faces):
        if face is None:
            faces[k] = last
        else:
            last = face
    return faces


def smooth_rbox_track(faces, n):
    """`smooth_box_track` of a track with angles: the box of (fx, fy, fw, fh, a) is smoothed as there, the angle is the mean
    of the window's angles in integer hundredths of a degree with floor division (no wrap-around handling: a head does not
    roll past 180 degrees).  n = 0 returns its input."""
    n = int(n)
    if n < 0:
        raise ValueError(f"smooth_rbox_track: n = {n} is negative")
    if n == 0:
        return list(faces)
    boxes = smooth_box_track([face[:4] for face in faces], n)
    hundredths = [angle_hundredths(face[4]) for face in faces]
    out = []
    for k, box in enumerate(boxes):
        window = hundredths[max(k - n, 0):k + n + 1]
        out.append(tuple(box) + ((sum(window) // len(window)) / 100.0,))
    return out


def _rot_arg(angles, B, who):
    """angles = B numbers of degrees -> (a ctypes int32 array [B * 2] in host memory holding `box_rotation` of each, or None
    when every angle is zero after rounding to hundredths: the caller then takes the axis-aligned entries)"""
    if isinstance(angles, torch.Tensor):
        angles = angles.tolist()
    try:
        hundredths = [angle_hundredths(a) for a in angles]
    except TypeError:
        raise ValueError(f"{who}: angles must be {B} numbers of degrees, one per frame") from None
    if len(hundredths) != B:
        raise ValueError(f"{who}: angles must be {B} numbers of degrees, one per frame")
    if not any(hundredths):
        return None
    return (C.c_int32 * (2 * B))(*[v for h in hundredths for v in box_rotation(h / 100.0)])


def box_of_frame(track, k):
    """entry k of a track; frames past its last line keep the last box"""
    return track[min(int(k), len(track) - 1)]


def track_crop_boxes(track, first, count, h, w, width, height, margin=TRACK_MARGIN):
    """`track_crop_box` of frames first .. first + count - 1 of a track (what `read_box_track` returns) in h x w frames: the
    [count][4] boxes of one batch of a frame loop"""
    return [track_crop_box(h, w, width, height, box_of_frame(track, first + i), margin) for i in range(count)]


def track_crop_rboxes(track, first, count, h, w, width, height, margin=TRACK_MARGIN):
    """`track_crop_boxes` of a track with angles (what `read_rbox_track` returns) -> (the [count][4] boxes, the count angles
    in degrees): the box is `track_crop_box` of the entry's (fx, fy, fw, fh), the angle the entry's own"""
    entries = [box_of_frame(track, first + i) for i in range(count)]
    return ([track_crop_box(h, w, width, height, e[:4], margin) for e in entries], [float(e[4]) for e in entries])


def _boxes_arg(boxes, B, who):
    """boxes = [B][4] integers (a sequence, a numpy array or a host tensor) -> a ctypes int32 array [B * 4] in host memory
    and the boxes as a list of 4-tuples"""
    if isinstance(boxes, torch.Tensor):
        boxes = boxes.tolist()
    rows = [tuple(int(v) for v in row) for row in boxes]
    if len(rows) != B or any(len(row) != 4 for row in rows):
        raise ValueError(f"{who}: boxes must be [{B}][4] integers (x1, y1, cw, ch), one box per frame")
    if any(not -2 ** 31 <= v < 2 ** 31 for row in rows for v in row):
        raise ValueError(f"{who}: boxes holds a value outside 32 bits")
    flat = (C.c_int32 * (4 * B))(*[v for row in rows for v in row])
    return flat, rows


def crop_resize_cubic_u8(frames, size, box=None, out=None, antialias=False, boxes=None, angles=None):
    """uint8 frames [h, w, 3] or [B, h, w, 3] on the HIP device -> the crop box (x1, y1, cw, ch) resized to size = (H, W)
    as cv2.resize(..., INTER_CUBIC) defines it in float arithmetic (include/d3f_hip.h: d3f_crop_resize_cubic_u8).
    box=None: the reference's centre crop to the target aspect.  out: a uint8 tensor [B, H, W, 3] whose pixels are packed
    and whose rows may be strided -- the left half of a [B, H, 2W, 3] side-by-side buffer, for one.
    antialias=True: Pillow's bicubic instead, whose window widens with the scale -- what
    torch.nn.functional.interpolate(mode="bicubic", antialias=True) computes (d3f_crop_resize_cubic_aa_u8); for crops several
    times the size of the output, where four taps per axis skip most of the source pixels.
    boxes: [B][4] integers in host memory, a box per frame, instead of box= (one of the two at most): frame b is byte for
    byte the single-box call on frame b with boxes[b], still one device call (d3f_crop_resize_cubic_boxes_u8 and its _aa
    form; one launch per 64 frames).
    angles: B angles in degrees next to boxes=, a rotation of each box about its centre (`box_rotation`): the crop's columns
    run along (cos a, sin a) of the frame, and taps clamp to the frame (d3f_crop_resize_cubic_rboxes_u8).  None, or all zero
    after rounding to hundredths, is the boxes= call, byte for byte and launch for launch.  Not with antialias=True."""
    if frames.dtype != torch.uint8 or frames.shape[-1] != 3 or frames.dim() not in (3, 4):
        raise ValueError("crop_resize_cubic_u8 expects uint8 frames [h, w, 3] or [B, h, w, 3]")
    if box is not None and boxes is not None:
        raise ValueError("crop_resize_cubic_u8: box= and boxes= exclude each other")
    if angles is not None and boxes is None:
        raise ValueError("crop_resize_cubic_u8: angles= needs boxes=")
    rot = None if angles is None else _rot_arg(angles, 1 if frames.dim() == 3 else int(frames.shape[0]), "crop_resize_cubic_u8")
    if rot is not None and antialias:
        raise ValueError("crop_resize_cubic_u8: antialias=True with non-zero angles: the antialiased crop of a rotated box "
                         "is out of scope")
    dev = _dev(frames)
    single = frames.dim() == 3
    x = (frames.unsqueeze(0) if single else frames).contiguous()
    B, h, w, _ = x.shape
    H, W = int(size[0]), int(size[1])
    if boxes is not None:
        table, _ = _boxes_arg(boxes, B, "crop_resize_cubic_u8")
    else:
        x1, y1, cw, ch = center_crop_box(h, w, W, H) if box is None else [int(v) for v in box]
    if out is None:
        out = torch.empty((B, H, W, 3), dtype=torch.uint8, device=dev)
    elif (tuple(out.shape) != (B, H, W, 3) or out.dtype != torch.uint8 or out.device != dev or out.stride(3) != 1
          or out.stride(2) != 3 or (B > 1 and out.stride(0) != H * out.stride(1))):
        raise ValueError(f"out must be a uint8 tensor of shape {(B, H, W, 3)} on the input's device with packed pixels "
                         f"and frames H rows apart")
    L = _lib.lib()
    if rot is not None:
        check(L.d3f_crop_resize_cubic_rboxes_u8(ptr(x), B, h, w, table, rot, ptr(out), H, W, out.stride(1), stream_ptr()))
        return out[0] if single else out
    if boxes is not None:
        resize = L.d3f_crop_resize_cubic_aa_boxes_u8 if antialias else L.d3f_crop_resize_cubic_boxes_u8
        check(resize(ptr(x), B, h, w, table, ptr(out), H, W, out.stride(1), stream_ptr()))
        return out[0] if single else out
    resize = L.d3f_crop_resize_cubic_aa_u8 if antialias else L.d3f_crop_resize_cubic_u8
    check(resize(ptr(x), B, h, w, x1, y1, cw, ch, ptr(out), H, W, out.stride(1), stream_ptr()))
    return out[0] if single else out


def default_feather(cw, ch):
    """width in source pixels of the ramp over which a pasted patch fades into its frame: the one place the default lives"""
    return min(int(cw), int(ch)) // 16


def channel_sums_u8(img, out=None):
    """uint8 images [H, W, 3] / [B, H, W, 3] on the HIP device -> uint64 sums [3, 2] / [B, 3, 2]: per frame and byte-in-pixel
    S = sum of p and Q = sum of p * p over the H * W pixels, exact (include/d3f_hip.h: d3f_channel_sums_u8; at most 2^22
    pixels per frame).  img: packed pixels at any byte address, rows may be strided -- one half of a [B, H, 2W, 3] pair
    buffer, for one.  out: a contiguous uint64 tensor [B, 3, 2] to overwrite."""
    if img.dtype != torch.uint8 or img.shape[-1] != 3 or img.dim() not in (3, 4):
        raise ValueError("channel_sums_u8 expects uint8 images [H, W, 3] or [B, H, W, 3]")
    single = img.dim() == 3
    x = img.unsqueeze(0) if single else img
    B, H, W, _ = x.shape
    if x.stride(3) != 1 or x.stride(2) != 3 or x.stride(1) < 3 * W or (B > 1 and x.stride(0) != H * x.stride(1)):
        raise ValueError("channel_sums_u8 expects packed pixels and frames H rows apart")
    dev = _dev(img)
    if out is None:
        sums = torch.empty((B, 3, 2), dtype=torch.uint64, device=dev)
    else:
        sums = out.unsqueeze(0) if single and out.dim() == 2 else out
        if tuple(sums.shape) != (B, 3, 2) or sums.dtype != torch.uint64 or sums.device != dev or not sums.is_contiguous():
            raise ValueError(f"out must be a contiguous uint64 tensor of shape {(B, 3, 2)} on the images' device")
    if B > 0:
        check(_lib.lib().d3f_channel_sums_u8(ptr(x), B, H, W, x.stride(1), ptr(sums), stream_ptr()))
    return sums[0] if single else sums


def color_match_coef(sums_from, sums_to, n):
    """sums [B, 3, 2] (or [3, 2]) uint64 of two image sets over n pixels per frame, as `channel_sums_u8` gives them -> float32
    coefficients of the same shape, gain then offset: gain * p + offset takes the mean and standard deviation of `from` to
    those of `to`, the gain clamped to 0.5 .. 2 (include/d3f_hip.h: d3f_color_match_coef)."""
    if (sums_from.dtype != torch.uint64 or sums_to.dtype != torch.uint64 or sums_from.shape != sums_to.shape
            or tuple(sums_from.shape[-2:]) != (3, 2) or sums_from.dim() not in (2, 3)):
        raise ValueError("color_match_coef expects two uint64 tensors [B, 3, 2] or [3, 2] of one shape")
    dev = _dev(sums_from)
    if sums_to.device != dev:
        raise ValueError("color_match_coef expects both sums on one device")
    f, t = sums_from.contiguous(), sums_to.contiguous()
    B = 1 if f.dim() == 2 else f.shape[0]
    coef = torch.empty(tuple(f.shape), dtype=torch.float32, device=dev)
    if B > 0:  # (an empty tensor has no pointer to hand over)
        check(_lib.lib().d3f_color_match_coef(ptr(f), ptr(t), B, int(n), ptr(coef), stream_ptr()))
    return coef


class TemporalState:
    """The state of the temporal filter for H x W images: `temporal_filter_u8`'s (`fake` [H, W, 3] float32, the last frame's
    unrounded filtered values; `real` [H, W, 3] uint8, its real bytes) and `color_coef_smooth`'s (`coef` [3, 2] float32,
    `sums` [3] uint64), with `valid` int32 [2]: the filter's flag, then the smoothing's.  A new state is invalid, so the
    first frame passes through; the buffers are uninitialised and are not read before they are written.  `reset()` makes
    the next frame a first frame again (both flags, on the current stream)."""

    def __init__(self, H, W, device="cuda"):
        H, W = int(H), int(W)
        if H <= 0 or W <= 0:
            raise ValueError(f"TemporalState: non-positive size ({H} x {W})")
        device = torch.device(device)
        if device.type != "cuda":
            raise _lib.D3FError("libd3f_hip ops need tensors on the HIP device (no CPU fallback)")
        self.H, self.W = H, W
        self.fake = torch.empty((H, W, 3), dtype=torch.float32, device=device)
        self.real = torch.empty((H, W, 3), dtype=torch.uint8, device=device)
        self.coef = torch.empty((3, 2), dtype=torch.float32, device=device)
        self.sums = torch.empty((3,), dtype=torch.uint64, device=device)
        self.valid = torch.zeros((2,), dtype=torch.int32, device=device)

    def reset(self):
        for k in range(2):
            check(_lib.lib().d3f_temporal_flag_set(self.valid.data_ptr() + 4 * k, 0, stream_ptr()))
        return self


def _strength(strength, what):
    if isinstance(strength, bool) or not isinstance(strength, (int, float)) or not 0.0 <= strength < 1.0:
        raise ValueError(f"{what}: the strength is a number in [0, 1), not {strength!r}")
    return float(strength)


def temporal_filter_u8(real, fake, state, strength=_lib.TEMPORAL_STRENGTH, threshold=_lib.TEMPORAL_THRESHOLD):
    """The motion-gated recursive filter against flicker (include/d3f_hip.h: d3f_temporal_filter_u8): uint8 `fake` [H, W, 3]
    / [B, H, W, 3] on the HIP device is filtered IN PLACE along time and returned; `real`, of the same shape, is the crop
    the network saw, and the 3 x 3 sum of absolute differences of it against its predecessor gates the filter per pixel
    (27 * threshold and above: the fake's byte passes bit for bit).  The frames of a call are consecutive in time and follow
    the last frame of the previous call on the same `state` (a `TemporalState` of this H x W).  Both images: packed pixels at
    any byte address, rows may be strided, frames H rows apart -- the halves of a [B, H, 2W, 3] pair buffer, for one."""
    if (real.dtype != torch.uint8 or fake.dtype != torch.uint8 or real.shape[-1] != 3 or real.dim() not in (3, 4)
            or tuple(real.shape) != tuple(fake.shape)):
        raise ValueError("temporal_filter_u8 expects uint8 real and fake of one shape, [H, W, 3] or [B, H, W, 3]")
    strength = _strength(strength, "temporal_filter_u8")
    if isinstance(threshold, bool) or not isinstance(threshold, int) or not 1 <= threshold <= 255:
        raise ValueError(f"temporal_filter_u8: the threshold is an integer in 1..255, not {threshold!r}")
    single = real.dim() == 3
    r, f = (real.unsqueeze(0), fake.unsqueeze(0)) if single else (real, fake)
    B, H, W, _ = r.shape
    for x in (r, f):
        if x.stride(3) != 1 or x.stride(2) != 3 or x.stride(1) < 3 * W or (B > 1 and x.stride(0) != H * x.stride(1)):
            raise ValueError("temporal_filter_u8 expects packed pixels and frames H rows apart")
    if not isinstance(state, TemporalState) or (state.H, state.W) != (H, W):
        raise ValueError(f"temporal_filter_u8: state must be a TemporalState of {H} x {W}")
    dev = _dev(real)
    if fake.device != dev or state.fake.device != dev:
        raise ValueError("temporal_filter_u8 expects real, fake and state on one device")
    if B > 0:
        check(_lib.lib().d3f_temporal_filter_u8(ptr(r), r.stride(1), ptr(f), f.stride(1), B, H, W, ptr(state.fake),
                                                ptr(state.real), ptr(state.valid), strength, threshold, stream_ptr()))
    return fake


def color_coef_smooth(coef, sums_to, n, state, strength=_lib.TEMPORAL_STRENGTH):
    """`color_match_coef`'s float32 coefficients [B, 3, 2] (or [3, 2]) smoothed across frames IN PLACE and returned
    (include/d3f_hip.h: d3f_color_coef_smooth): c = c' + strength * (c_prev - c'), the frames in order behind the last frame
    of the previous call on `state` (a `TemporalState`).  sums_to: the real crop's `channel_sums_u8` over n pixels, of the
    same shape in uint64 -- where any channel's sum moves by more than 16 * n against the predecessor's (a cut), and at a
    first frame, the coefficients pass as they are."""
    if (coef.dtype != torch.float32 or sums_to.dtype != torch.uint64 or tuple(coef.shape) != tuple(sums_to.shape)
            or tuple(coef.shape[-2:]) != (3, 2) or coef.dim() not in (2, 3)):
        raise ValueError("color_coef_smooth expects float32 coef and uint64 sums_to of one shape, [B, 3, 2] or [3, 2]")
    strength = _strength(strength, "color_coef_smooth")
    if not isinstance(state, TemporalState):
        raise ValueError("color_coef_smooth: state must be a TemporalState")
    if not coef.is_contiguous():
        raise ValueError("color_coef_smooth works in place: coef must be contiguous")
    dev = _dev(coef)
    if sums_to.device != dev or state.coef.device != dev:
        raise ValueError("color_coef_smooth expects coef, sums_to and state on one device")
    t = sums_to.contiguous()
    B = 1 if coef.dim() == 2 else coef.shape[0]
    if B > 0:
        check(_lib.lib().d3f_color_coef_smooth(ptr(coef), ptr(t), B, int(n), strength, ptr(state.coef), ptr(state.sums),
                                               state.valid.data_ptr() + 4, stream_ptr()))
    return coef


# ---- template tracker: the face box of a track file from hand-set key boxes (include/d3f_hip.h: "Template tracker") ----
TRACK_TEMPLATE_SIDE, TRACK_SEARCH, TRACK_ADAPT, TRACK_LOST = (_lib.TRACK_TEMPLATE_SIDE, _lib.TRACK_SEARCH, _lib.TRACK_ADAPT,
                                                              _lib.TRACK_LOST)
TRACK_SCALE_PENALTY = _lib.TRACK_SCALE_PENALTY
TRACK_RELOST = _lib.TRACK_RELOST
TRACK_ROT_STEP, TRACK_ROT_MAX, TRACK_ROT_PENALTY = _lib.TRACK_ROT_STEP, _lib.TRACK_ROT_MAX, _lib.TRACK_ROT_PENALTY


def gray_decimate_u8(frames, s, out=None):
    """uint8 BGR frames [h, w, 3] / [B, h, w, 3] on the HIP device -> the reduced grey image [h // s, w // s] /
    [B, h // s, w // s] uint8: (sum over each s x s block of B + 2 G + R) // (4 s s), partial blocks at the right and bottom
    dropped (include/d3f_hip.h: d3f_gray_decimate_u8).  frames: contiguous, at any byte address.  out: a contiguous uint8
    tensor of the result's shape to write into."""
    if frames.dtype != torch.uint8 or frames.shape[-1] != 3 or frames.dim() not in (3, 4):
        raise ValueError("gray_decimate_u8 expects uint8 frames [h, w, 3] or [B, h, w, 3]")
    s = int(s)
    if not 1 <= s <= _lib.TRACK_MAX_STRIDE:
        raise ValueError(f"gray_decimate_u8: the stride is an integer in 1..{_lib.TRACK_MAX_STRIDE}, not {s}")
    dev = _dev(frames)
    single = frames.dim() == 3
    x = (frames.unsqueeze(0) if single else frames).contiguous()
    B, h, w, _ = x.shape
    shape = (B, h // s, w // s)
    if out is None:
        g = torch.empty(shape, dtype=torch.uint8, device=dev)
    else:
        g = out.unsqueeze(0) if single and out.dim() == 2 else out
        if tuple(g.shape) != shape or g.dtype != torch.uint8 or g.device != dev or not g.is_contiguous():
            raise ValueError(f"out must be a contiguous uint8 tensor of shape {shape} on the frames' device")
    if g.numel() > 0:
        check(_lib.lib().d3f_gray_decimate_u8(ptr(x), B, h, w, s, ptr(g), stream_ptr()))
    return g[0] if single else g


def track_template_geometry(h, w, face, side=TRACK_TEMPLATE_SIDE):
    """The tracker's geometry for a face box (fx, fy, fw, fh) marked in an h x w frame, as (s, tx, ty, tw, th, ox, oy, fw, fh):
    the face clipped to the frame; the stride s = max(1, ceil(max(fw, fh) / side)) of the reduced grey image; the template's
    box there, tx = fx // s, ty = fy // s, tw = (fx + fw) // s - tx, th = (fy + fh) // s - ty; and ox = fx - tx s,
    oy = fy - ty s, so that a reduced position (px, py) is the face (px s + ox, py s + oy, fw, fh).  A ValueError: an empty
    clip, a side above 64, a stride above 32, a template below 4 samples on an axis."""
    h, w, side = int(h), int(w), int(side)
    fx, fy, fw, fh = [int(v) for v in face]
    if not 1 <= side <= _lib.TRACK_MAX_SIDE:
        raise ValueError(f"track_template_geometry: side {side} outside 1..{_lib.TRACK_MAX_SIDE}")
    x0, y0, x1, y1 = max(fx, 0), max(fy, 0), min(fx + fw, w), min(fy + fh, h)
    if x1 <= x0 or y1 <= y0:
        raise ValueError(f"track_template_geometry: the face {(fx, fy, fw, fh)} has nothing inside the {w} x {h} frame")
    fx, fy, fw, fh = x0, y0, x1 - x0, y1 - y0
    s = max(1, -(-max(fw, fh) // side))
    if s > _lib.TRACK_MAX_STRIDE:
        raise ValueError(f"track_template_geometry: a face of {fw} x {fh} at side {side} needs stride {s}, above "
                         f"{_lib.TRACK_MAX_STRIDE}")
    tx, ty = fx // s, fy // s
    tw, th = (fx + fw) // s - tx, (fy + fh) // s - ty
    if tw < _lib.TRACK_MIN_SIDE or th < _lib.TRACK_MIN_SIDE:
        raise ValueError(f"track_template_geometry: the face {fw} x {fh} gives a template of {tw} x {th}, below "
                         f"{_lib.TRACK_MIN_SIDE} samples")
    return s, tx, ty, tw, th, fx - tx * s, fy - ty * s, fw, fh


class TrackState:
    """The state of the template tracker: `templ`, the template's th rows of tw bytes packed at the front of 64 * 64 uint8,
    and `pos` int32 [2], both on the device; `geometry`, what `track_template_geometry` gave at the seed, and the frame
    size (h, w) it was given for, on the host; a grey workspace grown on demand; `seeded`.  `pos_level` int32 [3] is `pos`
    with the scale search's level behind it (`pos` is a view of its front): the seed sets it to L0 = max(tw, th), only
    `track_template_scale_u8` reads and moves it, and with it `templ` stays at the seed's size.  A seed with `angle=`
    makes the state one of the rotation search instead: the third entry is the angle index, `rot` = (step, max_degrees) of
    the seed (None otherwise), `templ` the upright face; only `track_template_rot_u8` follows such a state.  A seed with
    `reacquire=True` keeps `key_templ`, a copy of the template's bytes as the seed wrote them, which nothing adapts and the
    next seed replaces (None otherwise): what `track_template_reacq_u8` looks for in the whole frame; its keys live in a
    workspace of their own, grown on demand."""

    def __init__(self, device="cuda"):
        device = torch.device(device)
        if device.type != "cuda":
            raise _lib.D3FError("libd3f_hip ops need tensors on the HIP device (no CPU fallback)")
        self.templ = torch.zeros((_lib.TRACK_MAX_SIDE * _lib.TRACK_MAX_SIDE,), dtype=torch.uint8, device=device)
        self.pos_level = torch.zeros((3,), dtype=torch.int32, device=device)
        self.pos = self.pos_level[:2]
        self.geometry = None
        self.h = self.w = 0
        self.gray = None
        self.seeded = False
        self.rot = None
        self.key_templ = None
        self.keys = None

    def workspace(self, n):
        if self.gray is None or self.gray.numel() < n:
            self.gray = torch.empty((n,), dtype=torch.uint8, device=self.templ.device)
        return self.gray

    def keys_workspace(self, n):
        if self.keys is None or self.keys.numel() < n:
            self.keys = torch.empty((n,), dtype=torch.int64, device=self.templ.device)
        return self.keys


def track_rot_table(step=TRACK_ROT_STEP, max_degrees=TRACK_ROT_MAX):
    """the rotation search's table: [(c16, s16)] = `box_rotation(a * step / 100)` for the angle indices a = -amax..amax (entry
    a + amax), index a the angle a * step hundredths of a degree, amax = floor(max_degrees * 100 / step).  A ValueError: a
    step that is no positive integer, a range that is negative, beyond 180 degrees or of more than 64 steps."""
    if isinstance(step, bool) or not isinstance(step, int) or step < 1:
        raise ValueError(f"track_rot_table: the step is a positive integer of hundredths of a degree, not {step!r}")
    try:
        reach = float(max_degrees)
    except (TypeError, ValueError):
        reach = -1.0
    if not 0.0 <= reach <= 180.0:  # (a NaN fails both comparisons)
        raise ValueError(f"track_rot_table: the range is a number of degrees in 0..180, not {max_degrees!r}")
    amax = int(reach * 100.0) // step
    if amax > _lib.TRACK_ROT_MAX_INDEX:
        raise ValueError(f"track_rot_table: {max_degrees} degrees in steps of {step / 100.0:.2f} are {amax} indices, above "
                         f"{_lib.TRACK_ROT_MAX_INDEX}")
    return [box_rotation(a * step / 100.0) for a in range(-amax, amax + 1)]


def _rot_table_arg(step, max_degrees):
    """(amax, the table as a ctypes int32 array in host memory)"""
    table = track_rot_table(step, max_degrees)
    flat = [v for pair in table for v in pair]
    return len(table) // 2, (C.c_int32 * len(flat))(*flat)


def track_seed(state, frame, face, side=TRACK_TEMPLATE_SIDE, angle=None, step=TRACK_ROT_STEP, max_degrees=TRACK_ROT_MAX,
               reacquire=False):
    """(re-)seed `state` from the face box (fx, fy, fw, fh) marked in `frame`, uint8 BGR [h, w, 3] on the HIP device: the
    template is the reduced grey of the box, the level the seed's own (include/d3f_hip.h: d3f_track_seed_scale_u8, the
    launch of d3f_track_seed_u8 with the level stored beside the position).  Returns the geometry.
    angle: the head's roll in the key frame in degrees (0: the tracked angle is relative to the key frame's pose): the seed of
    the rotation search with `step` and `max_degrees` (`track_rot_table`) -- the angle index a0 = round(angle / step), a
    ValueError outside the table; the template is the box's grey turned back by that angle on the disc (d3f_track_seed_rot_u8).
    reacquire: True keeps the seed's template bytes in `state.key_templ` as well, the key template of
    `track_template_reacq_u8`; every seed replaces it (a seed without reacquire=True by None).  Not together with angle=:
    the whole-frame search looks for one size at one angle."""
    if not isinstance(state, TrackState):
        raise ValueError("track_seed: state must be a TrackState")
    if reacquire and angle is not None:
        raise ValueError("track_seed: reacquire=True with angle=: the whole-frame search looks for the key template at one "
                         "angle and cannot restore the one the rotation search keeps")
    if frame.dtype != torch.uint8 or frame.dim() != 3 or frame.shape[-1] != 3:
        raise ValueError("track_seed expects one uint8 frame [h, w, 3]")
    h, w = int(frame.shape[0]), int(frame.shape[1])
    geometry = track_template_geometry(h, w, face, side)
    s, tx, ty, tw, th = geometry[:5]
    if _dev(frame) != state.templ.device:
        raise ValueError("track_seed expects the frame on the state's device")
    x = frame.contiguous()
    if angle is None:
        check(_lib.lib().d3f_track_seed_scale_u8(ptr(x), h, w, s, tx, ty, tw, th, ptr(state.templ), ptr(state.pos_level),
                                                 stream_ptr()))
        rot = None
    else:
        table = track_rot_table(step, max_degrees)
        hundredths = angle_hundredths(angle)
        a0 = (2 * abs(hundredths) + step) // (2 * step) * (1 if hundredths >= 0 else -1)  # halves away from zero
        if abs(a0) > len(table) // 2:
            raise ValueError(f"track_seed: the angle {angle} is index {a0} at step {step}, outside the table of "
                             f"+-{len(table) // 2}")
        c16, s16 = table[a0 + len(table) // 2]
        check(_lib.lib().d3f_track_seed_rot_u8(ptr(x), h, w, s, tx, ty, tw, th, a0, c16, s16, ptr(state.templ),
                                               ptr(state.pos_level), stream_ptr()))
        rot = (step, max_degrees)
    state.geometry, state.h, state.w, state.seeded, state.rot = geometry, h, w, True, rot
    state.key_templ = state.templ.clone() if reacquire else None  # (on the current stream, behind the seed's launch)
    return geometry


def track_template_u8(frames, state, search=TRACK_SEARCH, adapt=TRACK_ADAPT, lost=TRACK_LOST):
    """follow the seeded template through uint8 BGR frames [B, h, w, 3] on the HIP device, consecutive in time and behind the
    last frame of the previous call on `state` -> int32 [B, 4] on the device, a row (px, py, cost, found) per frame in the
    reduced image (`track_faces` turns host rows into boxes).  One device call: the reduced grey of every frame, then the
    search, frame by frame, inside one kernel (include/d3f_hip.h: d3f_track_template_u8)."""
    if not isinstance(state, TrackState) or not state.seeded:
        raise ValueError("track_template_u8: state must be a TrackState seeded by track_seed")
    if frames.dtype != torch.uint8 or frames.dim() != 4 or frames.shape[-1] != 3:
        raise ValueError("track_template_u8 expects uint8 frames [B, h, w, 3]")
    B, h, w, _ = frames.shape
    if (h, w) != (state.h, state.w):
        raise ValueError(f"track_template_u8: frames of {h} x {w}, the state was seeded on {state.h} x {state.w}")
    if _dev(frames) != state.templ.device:
        raise ValueError("track_template_u8 expects the frames on the state's device")
    s, _, _, tw, th = state.geometry[:5]
    out = torch.empty((B, 4), dtype=torch.int32, device=frames.device)
    if B > 0:
        x = frames.contiguous()
        ws = state.workspace(B * (h // s) * (w // s))
        check(_lib.lib().d3f_track_template_u8(ptr(x), B, h, w, s, tw, th, int(search), int(adapt), int(lost),
                                               ptr(state.templ), ptr(state.pos), ptr(ws), ptr(out), stream_ptr()))
    return out


def track_global_u8(gray, key_templ, tw, th, out=None):
    """the whole-frame search: the key template (uint8 on the HIP device, th rows of tw bytes packed at the front, as
    `TrackState.key_templ` holds them) against EVERY position of the reduced grey image(s) [gh, gw] / [B, gh, gw] uint8
    (contiguous, at any byte address) -> the smallest key of each frame, int64 [B] on the device ([1] for one image).  A key
    is the C entry's unsigned 64 bits carried in an int64 (never negative: the cost is below 2^20):
    cost = key >> 32, y = (key >> 16) & 0xffff, x = key & 0xffff -- the smallest sum of absolute differences, and among equal
    sums the top-most, then the left-most position (include/d3f_hip.h: d3f_track_global_u8).  out: a contiguous int64 tensor
    [B] to write into."""
    if gray.dtype != torch.uint8 or gray.dim() not in (2, 3):
        raise ValueError("track_global_u8 expects a uint8 grey image [gh, gw] or [B, gh, gw]")
    tw, th = int(tw), int(th)
    dev = _dev(gray)
    if key_templ.dtype != torch.uint8 or key_templ.numel() < tw * th or key_templ.device != dev or not key_templ.is_contiguous():
        raise ValueError(f"track_global_u8: key_templ must be contiguous uint8 of at least {tw} x {th} bytes on the image's device")
    g = (gray.unsqueeze(0) if gray.dim() == 2 else gray).contiguous()
    B, gh, gw = g.shape
    if out is None:
        keys = torch.empty((B,), dtype=torch.int64, device=dev)
    else:
        keys = out
        if tuple(keys.shape) != (B,) or keys.dtype != torch.int64 or keys.device != dev or not keys.is_contiguous():
            raise ValueError(f"out must be a contiguous int64 tensor of shape ({B},) on the image's device")
    if B > 0:
        check(_lib.lib().d3f_track_global_u8(ptr(g), B, gh, gw, tw, th, ptr(key_templ), ptr(keys), stream_ptr()))
    return keys


def track_template_reacq_u8(frames, state, search=TRACK_SEARCH, adapt=TRACK_ADAPT, lost=TRACK_LOST, relost=TRACK_RELOST):
    """`track_template_u8` with re-acquisition: a frame that the search window does not find is looked for in the whole
    frame with the state's key template, and taken from there when that costs at most `relost` (0..255) grey levels a
    sample -- the position becomes the whole-frame winner's, the template the key template's bytes -> int32 [B, 4] on the
    device, a row (px, py, cost, found) per frame, found 1 by the window, 2 re-acquired (cost: the whole-frame winner's),
    0 lost (`track_faces` takes 1 and 2 alike).  The state is one that `track_seed(..., reacquire=True)` seeded.  One device
    call: the reduced grey of every frame, the whole-frame search of every frame over all CUs, then the serial search
    (include/d3f_hip.h: d3f_track_template_reacq_u8)."""
    if not isinstance(state, TrackState) or not state.seeded:
        raise ValueError("track_template_reacq_u8: state must be a TrackState seeded by track_seed")
    if state.key_templ is None:
        raise ValueError("track_template_reacq_u8: the state was seeded without reacquire=True and holds no key template")
    if frames.dtype != torch.uint8 or frames.dim() != 4 or frames.shape[-1] != 3:
        raise ValueError("track_template_reacq_u8 expects uint8 frames [B, h, w, 3]")
    B, h, w, _ = frames.shape
    if (h, w) != (state.h, state.w):
        raise ValueError(f"track_template_reacq_u8: frames of {h} x {w}, the state was seeded on {state.h} x {state.w}")
    if _dev(frames) != state.templ.device:
        raise ValueError("track_template_reacq_u8 expects the frames on the state's device")
    s, _, _, tw, th = state.geometry[:5]
    out = torch.empty((B, 4), dtype=torch.int32, device=frames.device)
    if B > 0:
        x = frames.contiguous()
        ws = state.workspace(B * (h // s) * (w // s))
        check(_lib.lib().d3f_track_template_reacq_u8(ptr(x), B, h, w, s, tw, th, int(search), int(adapt), int(lost), int(relost),
                                                     ptr(state.templ), ptr(state.key_templ), ptr(state.pos), ptr(ws),
                                                     ptr(state.keys_workspace(B)), ptr(out), stream_ptr()))
    return out


def track_faces(rows, state):
    """host rows (px, py, cost, found) of `track_template_u8` or `track_template_reacq_u8` -> a list of face boxes (x, y, w, h)
    in frame pixels, None where the frame's row says not found (found 0; 1 and 2, a re-acquired frame, are boxes alike).
    state: the TrackState the rows came from, or the geometry it had then"""
    s, _, _, _, _, ox, oy, fw, fh = getattr(state, "geometry", state)
    return [(int(px) * s + ox, int(py) * s + oy, fw, fh) if int(found) else None for px, py, _, found in rows]


def track_template_scale_u8(frames, state, search=TRACK_SEARCH, adapt=TRACK_ADAPT, lost=TRACK_LOST, levels=1,
                            penalty=TRACK_SCALE_PENALTY):
    """`track_template_u8` with the scale search: the box may change its level, one sample on the template's longer side,
    by up to `levels` (0 or 1) a frame; `penalty` (0..65535, in 1/4096 grey levels per sample) is what a change of level
    must win by -> int32 [B, 8] on the device, a row (px, py, tw, th, ncost, found, L, cost) per frame in the reduced image
    (`track_scale_faces` turns host rows into boxes).  The state's template stays at the seed's size and its level moves;
    do not mix calls of this and of `track_template_u8` on one state between two seeds.  One device call: the reduced grey
    of every frame, then the search inside one kernel (include/d3f_hip.h: d3f_track_template_scale_u8)."""
    if not isinstance(state, TrackState) or not state.seeded:
        raise ValueError("track_template_scale_u8: state must be a TrackState seeded by track_seed")
    if frames.dtype != torch.uint8 or frames.dim() != 4 or frames.shape[-1] != 3:
        raise ValueError("track_template_scale_u8 expects uint8 frames [B, h, w, 3]")
    B, h, w, _ = frames.shape
    if (h, w) != (state.h, state.w):
        raise ValueError(f"track_template_scale_u8: frames of {h} x {w}, the state was seeded on {state.h} x {state.w}")
    if _dev(frames) != state.templ.device:
        raise ValueError("track_template_scale_u8 expects the frames on the state's device")
    s, _, _, tw, th = state.geometry[:5]
    out = torch.empty((B, 8), dtype=torch.int32, device=frames.device)
    if B > 0:
        x = frames.contiguous()
        ws = state.workspace(B * (h // s) * (w // s))
        check(_lib.lib().d3f_track_template_scale_u8(ptr(x), B, h, w, s, tw, th, int(search), int(adapt), int(lost),
                                                     int(levels), int(penalty), ptr(state.templ), ptr(state.pos_level),
                                                     ptr(ws), ptr(out), stream_ptr()))
    return out


def track_scale_faces(rows, state, frame=None):
    """host rows (px, py, tw, th, ncost, found, L, cost) of `track_template_scale_u8` -> a list of face boxes (x, y, w, h) in
    frame pixels, None where the frame's row says not found: the seed's face scaled by L / L0 about the centre of the
    reduced box, then moved so that at least one of its pixels lies inside the frame (`track_crop_box` accepts a face that
    sticks out).  state: the TrackState the rows came from, or the geometry it had then with frame=(h, w) -- a geometry
    alone says nothing of the frame's size, and the boxes are then left where they fall"""
    s, _, _, tw0, th0, ox, oy, fw, fh = getattr(state, "geometry", state)
    if frame is None:
        frame = (state.h, state.w) if hasattr(state, "h") else None
    L0 = max(tw0, th0)
    boxes = []
    for px, py, tw, th, _, found, L, _ in rows:
        if not int(found):
            boxes.append(None)
            continue
        px, py, tw, th, L = int(px), int(py), int(tw), int(th), int(L)
        fw1, fh1 = (fw * L + L0 // 2) // L0, (fh * L + L0 // 2) // L0
        x = ((2 * px + tw) * s + 2 * ox + fw - tw0 * s - fw1) // 2
        y = ((2 * py + th) * s + 2 * oy + fh - th0 * s - fh1) // 2
        if frame is not None:
            x, y = min(max(x, 1 - fw1), frame[1] - 1), min(max(y, 1 - fh1), frame[0] - 1)
        boxes.append((x, y, fw1, fh1))
    return boxes


def track_template_rot_u8(frames, state, search=TRACK_SEARCH, adapt=TRACK_ADAPT, lost=TRACK_LOST, steps=1,
                          penalty=TRACK_ROT_PENALTY, step=TRACK_ROT_STEP, max_degrees=TRACK_ROT_MAX):
    """`track_template_u8` with the rotation search: the box may turn about its centre by up to `steps` (0 or 1) angle
    indices a frame, an index `step` hundredths of a degree, within +-`max_degrees`; `penalty` (0..65535, in 1/4096 grey
    levels per sample) is what a turn must win by -> int32 [B, 8] on the device, a row (px, py, tw0, th0, ncost, found, a,
    cost) per frame in the reduced image (`track_rot_faces` turns host rows into boxes and angles).  The state is one that
    `track_seed(..., angle=)` seeded with the same step and range: its template is the upright face, its third entry the
    angle index.  One device call: the reduced grey of every frame, then the search inside one kernel (include/d3f_hip.h:
    d3f_track_template_rot_u8)."""
    if not isinstance(state, TrackState) or not state.seeded:
        raise ValueError("track_template_rot_u8: state must be a TrackState seeded by track_seed")
    if state.rot != (step, max_degrees):
        raise ValueError(f"track_template_rot_u8: step {step} and range {max_degrees}, the state was seeded "
                         + ("without angle=" if state.rot is None else f"with {state.rot}"))
    if frames.dtype != torch.uint8 or frames.dim() != 4 or frames.shape[-1] != 3:
        raise ValueError("track_template_rot_u8 expects uint8 frames [B, h, w, 3]")
    B, h, w, _ = frames.shape
    if (h, w) != (state.h, state.w):
        raise ValueError(f"track_template_rot_u8: frames of {h} x {w}, the state was seeded on {state.h} x {state.w}")
    if _dev(frames) != state.templ.device:
        raise ValueError("track_template_rot_u8 expects the frames on the state's device")
    s, _, _, tw, th = state.geometry[:5]
    amax, table = _rot_table_arg(step, max_degrees)
    out = torch.empty((B, 8), dtype=torch.int32, device=frames.device)
    if B > 0:
        x = frames.contiguous()
        ws = state.workspace(B * (h // s) * (w // s))
        check(_lib.lib().d3f_track_template_rot_u8(ptr(x), B, h, w, s, tw, th, int(search), int(adapt), int(lost), int(steps),
                                                   int(penalty), amax, table, ptr(state.templ), ptr(state.pos_level), ptr(ws),
                                                   ptr(out), stream_ptr()))
    return out


def track_rot_faces(rows, state, step=TRACK_ROT_STEP):
    """host rows (px, py, tw0, th0, ncost, found, a, cost) of `track_template_rot_u8` -> a list of (x, y, w, h, hundredths),
    None where the frame's row says not found: the box is `track_faces`' box, which turns about its centre, the angle
    a * step in hundredths of a degree.  state: the TrackState the rows came from, or the geometry it had then"""
    s, _, _, _, _, ox, oy, fw, fh = getattr(state, "geometry", state)
    return [(int(r[0]) * s + ox, int(r[1]) * s + oy, fw, fh, int(r[6]) * int(step)) if int(r[5]) else None for r in rows]


def _paste_args(who, patch, frames, box, out, color, boxes):
    """the arguments the paste operators share, checked: (patch [B,H,W,3], frames [B,h,w,3] contiguous, out, geo = the box's
    four integers or (the ctypes boxes table,), coef [B,3,2] or None, single, rows = the boxes as 4-tuples)"""
    if (box is None) == (boxes is None):
        raise ValueError(f"{who}: exactly one of box= and boxes=")
    if (patch.dtype != torch.uint8 or patch.shape[-1] != 3 or patch.dim() not in (3, 4) or frames.dtype != torch.uint8
            or frames.shape[-1] != 3 or frames.dim() != patch.dim()):
        raise ValueError(f"{who} expects a uint8 patch [H, W, 3] and frames [h, w, 3], or a batch of both")
    dev = _dev(frames)
    single = frames.dim() == 3
    p = patch.unsqueeze(0) if single else patch
    in_place = out is frames
    f = frames.unsqueeze(0) if single else frames
    if in_place and not f.is_contiguous():
        raise ValueError("out=frames (in place) needs contiguous frames")
    f = f.contiguous()
    B = f.shape[0]
    H, W = int(p.shape[1]), int(p.shape[2])
    if (p.shape[0] != B or p.device != dev or p.stride(3) != 1 or p.stride(2) != 3 or p.stride(1) < 3 * W
            or (B > 1 and p.stride(0) != H * p.stride(1))):
        raise ValueError(f"patch must be a uint8 tensor [{B}, H, W, 3] on the frames' device with packed pixels and frames "
                         f"H rows apart")
    if boxes is not None:
        table, rows = _boxes_arg(boxes, B, who)
        geo = (table,)
    else:
        geo = tuple(int(v) for v in box)
        rows = [geo] * B
    if in_place:
        o = f
    elif out is None:
        o = torch.empty_like(f)
    else:
        o = out.unsqueeze(0) if single and out.dim() == 3 else out
        if tuple(o.shape) != tuple(f.shape) or o.dtype != torch.uint8 or o.device != dev or not o.is_contiguous():
            raise ValueError(f"out must be a contiguous uint8 tensor of shape {tuple(frames.shape)} on the frames' device")
    coef = None
    if color is not None:
        coef = color.unsqueeze(0) if single and color.dim() == 2 else color
        if tuple(coef.shape) != (B, 3, 2) or coef.dtype != torch.float32 or coef.device != dev:
            raise ValueError(f"color must be a float32 tensor of shape {(B, 3, 2)} on the frames' device")
        coef = coef.contiguous()
    return p, f, o, geo, coef, single, rows


def paste_resize_cubic_u8(patch, frames, box=None, feather=0, out=None, color=None, boxes=None, angles=None):
    """The inverse of `crop_resize_cubic_u8` with a blend: uint8 `patch` [H, W, 3] / [B, H, W, 3] on the HIP device is resized
    to the box (x1, y1, cw, ch) of uint8 `frames` [h, w, 3] / [B, h, w, 3] with the same arithmetic and blended in over a
    ramp of `feather` pixels; outside the box the result is the frame (include/d3f_hip.h: d3f_paste_resize_cubic_u8).
    patch: packed pixels, rows may be strided -- the right half of a [B, H, 2W, 3] pair buffer, for one.  out=frames runs in
    place; otherwise out is a contiguous tensor shaped like frames, allocated when None.
    color: float32 coefficients [B, 3, 2] ([3, 2] for a single frame), gain then offset per frame and byte-in-pixel, as
    `color_match_coef` gives them: the patch's resized, clamped value goes through gain * v + offset and a second clamp before
    the blend (d3f_paste_resize_cubic_color_u8).  None: the plain call.
    boxes: [B][4] integers in host memory, a box per frame, instead of box= (exactly one of the two); one `feather` for the
    call.  Frame b is byte for byte the single-box call on frame b with boxes[b] (d3f_paste_resize_cubic_boxes_u8 and its
    _color form; one launch per 64 frames).
    angles: B angles in degrees next to boxes=, as `crop_resize_cubic_u8` takes them: the patch goes back into the rotated
    rectangle -- a frame pixel belongs to the box when its centre lies in it, the ramp runs on the distance to the
    rectangle's sides (d3f_paste_resize_cubic_rboxes_u8 and its _color form).  None or all zero: the boxes= call."""
    if angles is not None and boxes is None:
        raise ValueError("paste_resize_cubic_u8: angles= needs boxes=")
    rot = None if angles is None else _rot_arg(angles, 1 if frames.dim() == 3 else int(frames.shape[0]), "paste_resize_cubic_u8")
    p, f, o, geo, coef, single, _ = _paste_args("paste_resize_cubic_u8", patch, frames, box, out, color, boxes)
    B, h, w, _ = f.shape
    H, W = int(p.shape[1]), int(p.shape[2])
    L = _lib.lib()
    if rot is not None:
        if coef is None:
            check(L.d3f_paste_resize_cubic_rboxes_u8(ptr(p), B, H, W, p.stride(1), ptr(f), h, w, geo[0], rot, int(feather),
                                                     ptr(o), stream_ptr()))
        else:
            check(L.d3f_paste_resize_cubic_color_rboxes_u8(ptr(p), B, H, W, p.stride(1), ptr(f), h, w, geo[0], rot,
                                                           int(feather), ptr(coef), ptr(o), stream_ptr()))
        return o[0] if single else o
    if coef is None:
        paste = L.d3f_paste_resize_cubic_u8 if boxes is None else L.d3f_paste_resize_cubic_boxes_u8
        check(paste(ptr(p), B, H, W, p.stride(1), ptr(f), h, w, *geo, int(feather), ptr(o), stream_ptr()))
        return o[0] if single else o
    paste = L.d3f_paste_resize_cubic_color_u8 if boxes is None else L.d3f_paste_resize_cubic_color_boxes_u8
    check(paste(ptr(p), B, H, W, p.stride(1), ptr(f), h, w, *geo, int(feather), ptr(coef), ptr(o), stream_ptr()))
    return o[0] if single else o


def multiband_levels(feather):
    """the pyramid levels of a multiband paste over `feather` pixels when the caller names none -- the one place the default
    lives: the largest N in 1..5 with (feather >> N) >= 2, else 1, so that the coarsest band's ramp is still at least two of
    its own samples wide.  A design choice, not a measurement."""
    feather = int(feather)
    return max([n for n in range(1, 6) if (feather >> n) >= 2], default=1)


def paste_multiband_u8(patch, frames, box=None, feather=0, levels=None, out=None, color=None, boxes=None):
    """`paste_resize_cubic_u8` with a multiband (Burt & Adelson) blend in place of the single ramp: the difference between the
    resized patch and the frame is split into `levels` frequency bands, the coarsest fades over about `feather` pixels and
    every finer band over half the band above, in integer arithmetic throughout (include/d3f_hip.h: d3f_paste_multiband_u8;
    tests/multiband_restatement.py restates it).  feather=0 is byte for byte `paste_resize_cubic_u8(..., feather=0)`.
    levels: 1..6, None: `multiband_levels(feather)`; every box needs min(cw, ch) >= 2 ** levels.  patch, out, color and
    boxes: as `paste_resize_cubic_u8` (the _color, _boxes and _color_boxes forms of the operator).  The pyramid workspace is
    allocated here, per call."""
    p, f, o, geo, coef, single, rows = _paste_args("paste_multiband_u8", patch, frames, box, out, color, boxes)
    B, h, w, _ = f.shape
    H, W = int(p.shape[1]), int(p.shape[2])
    levels = multiband_levels(feather) if levels is None else int(levels)
    L = _lib.lib()
    need = L.d3f_paste_multiband_workspace_bytes(B, max([r[2] for r in rows], default=1), max([r[3] for r in rows], default=1),
                                                 levels)
    if need < 0:
        check(-1)
    ws = torch.empty(max(int(need), 16), dtype=torch.uint8, device=f.device)
    tail = (ptr(ws), int(need), ptr(o), stream_ptr())
    if coef is None:
        paste = L.d3f_paste_multiband_u8 if boxes is None else L.d3f_paste_multiband_boxes_u8
        check(paste(ptr(p), B, H, W, p.stride(1), ptr(f), h, w, *geo, int(feather), levels, *tail))
    else:
        paste = L.d3f_paste_multiband_color_u8 if boxes is None else L.d3f_paste_multiband_color_boxes_u8
        check(paste(ptr(p), B, H, W, p.stride(1), ptr(f), h, w, *geo, int(feather), levels, ptr(coef), *tail))
    return o[0] if single else o


def image_grid_shape(images, nrow=3, padding=2, size=(1, 1)):
    """(GH, GW) of torchvision.utils.make_grid over `images` images of size = (H, W) (d3f_image_grid_shape; host only)"""
    dims = (C.c_int32 * 2)()
    check(_lib.lib().d3f_image_grid_shape(int(images), int(nrow), int(padding), int(size[0]), int(size[1]), dims))
    return int(dims[0]), int(dims[1])


def image_grid_u8(batches, nrow=3, padding=2, pad_value=0.0, scale=0.5, shift=0.5, max_images=9, out=None):
    """log_batch_as_image_grid of the LitModules (d3f/train_deep_fake/lit_module.py:235-249) for up to 8 tags in one
    launch: an NCHW batch, or a list of up to 8 of one shape, on the HIP device -> uint8 [n, GH, GW, 3], grid i being
    make_grid(batches[i][:max_images], nrow, padding, pad_value) * scale + shift, clamped to 0..1, times 255, truncated
    (include/d3f_hip.h: d3f_image_grid_u8).  out: a contiguous uint8 tensor of that shape to write into."""
    single = isinstance(batches, torch.Tensor)
    xs = [b.detach().contiguous().float() for b in ([batches] if single else list(batches))]
    if not xs or any(x.dim() != 4 or x.shape != xs[0].shape or x.device != xs[0].device for x in xs):
        raise ValueError("image_grid_u8 expects an NCHW batch or a list of NCHW batches of one shape on one device")
    dev = _dev(xs[0])
    n, (B, Cc, H, W) = len(xs), xs[0].shape
    images = min(B, int(max_images))
    GH, GW = image_grid_shape(images, nrow, padding, (H, W))
    if out is None:
        out = torch.empty((n, GH, GW, 3), dtype=torch.uint8, device=dev)
    elif tuple(out.shape) != (n, GH, GW, 3) or out.dtype != torch.uint8 or out.device != dev or not out.is_contiguous():
        raise ValueError(f"out must be a contiguous uint8 tensor of shape {(n, GH, GW, 3)} on the input's device")
    pointers = (C.c_void_p * n)(*[x.data_ptr() for x in xs])
    check(_lib.lib().d3f_image_grid_u8(pointers, n, B, Cc, H, W, images, int(nrow), int(padding), float(pad_value),
                                       float(scale), float(shift), ptr(out), stream_ptr()))
    return out
