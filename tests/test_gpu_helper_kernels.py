"""The step's memory-bound helper kernels at operator level against float64, at the shapes where their unrolled loops,
tails and grid edges change.

Kernels and what reaches them (all through the single-operator entries of the C ABI):

| kernel                                         | reached by                                                           |
|------------------------------------------------|----------------------------------------------------------------------|
| maxpool_bwd_kernel<T, ACC>                     | test_maxpool_backward (d3f_maxpool3x3s2_backward)                    |
| nchw_to_nhwc_kernel<T>, one store per pixel    | test_layout (d3f_nchw_to_nhwc), Cpad = one vector, aligned           |
| nchw_to_nhwc_kernel<T>, element stores         | test_layout, Cpad = two vectors / an output that is not 16-B aligned |
| bn_finalize_kernel (column_sum2)               | test_bn_split_forms (d3f_bn_layer_forward), test_bn_finalize_rows    |
| bn_apply_kernel<T, RES>                        | test_bn_split_forms, test_bn_one_row, test_bn_older_entries          |
| bn_bwd_reduce_kernel<T>                        | test_bn_split_forms (partials from the reduce), test_bn_one_row      |
| bn_bwd_finalize_kernel (column_sum2)           | test_bn_split_forms (1024 reduce rows / 3333 supplied rows)          |
| bn_bwd_apply_kernel<T, MASK, DRES>             | test_bn_split_forms, test_bn_one_row, test_bn_older_entries          |
| pack_all_kernel<T, false>                      | test_pack_weights (d3f_conv_pack_weights), both layouts              |
| ssim_fwd_kernel, ssim_mse_bwd_kernel,          | test_mse_ssim_loss (d3f_mse_ssim_loss): 12 x 12 = one partial tile,  |
|   loss_finalize_kernel                         |   43 x 45 = ragged tiles in both directions                          |

Bounds.  Every kernel here does a fixed number n of fp32 roundings per output element, so |out - ref| <= n * 2^-24 * (sum
of the absolute values of the terms), ref = the same expression in float64; bf16 storage adds one rounding of the result.
The BatchNorm expressions and their counts are the ones tests/test_gpu_batchnorm.py states (A_ROUNDINGS, DY_ROUNDINGS,
run_case); this file drives them, in the split form (allow_fused = 0), over C = 16 / 64 / 128, 1 / 33 / 1000 rows and one
row count just above a whole unrolled trip of the streaming kernels, all three masks, both residual forms, both storage
types.  A trip of bn_apply_kernel / bn_bwd_apply_kernel is U * 2048 * 256 vectors (U = 4 for fp32, 2 for bf16): below that
only their tails run, so BIG_ROWS is what it takes to enter the unrolled loop at all.
max-pool backward: an input pixel collects at most four windows; the first add to 0 is exact, so n = (terms - 1) + 1 for
the accumulated base.  The layout kernel copies: exact (bf16: torch's own round-to-nearest-even).
The criterion's bound is carried through its expression operation by operation (class E below).
pack_all_kernel (d3f_conv_pack_weights) copies: the packed buffers, zero padding included, equal the layouts restated here.

The tests without the gpu mark evaluate the same expressions with torch in fp32 on the CPU and hold them to the same
bounds: the bounds admit an honest fp32 evaluation (and the check functions are exercised without a GPU).
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import test_gpu_batchnorm as bn
from util import SENTINEL, Guarded, to_nhwc

gpu = pytest.mark.gpu
F32, BF16 = 0, 1
U24 = 2.0 ** -24
DEV = "cuda"
TRIP_VECTORS = 2048 * 256  # vectors one grid-stride step of the streaming kernels covers (vec16.h, grid_for)
BIG_ROWS = {16: 4 * TRIP_VECTORS * 4 // 16 + 33, 128: 4 * TRIP_VECTORS * 4 // 128 + 33}  # fp32: four whole steps + a tail
MORE_ROWS = 6 * TRIP_VECTORS * 4 // 16 + 33  # C = 16: six whole steps + a tail (fp32), three + a tail (bf16)


@pytest.fixture(scope="module")
def ops():
    from denoising_diffusion_deep_fake_amd import ops as m
    return m


def tdt(dt):
    return torch.bfloat16 if dt == BF16 else torch.float32


def within(out, ref, bound, dt, what):
    bn.check_elementwise(out, ref, bound, dt, what)


# ------------------------------------------------------------------------------------------
# max-pool backward
# ------------------------------------------------------------------------------------------
POOL_SHAPES = [(2, 6, 6, 8), (2, 6, 6, 64), (2, 10, 14, 8), (2, 10, 14, 64), (2, 14, 10, 64), (2, 10, 14, 96), (2, 10, 14, 160)]
# 6 and 10 rows: 3 and 5 row pairs per image against 2 pairs per workgroup (a workgroup straddles two images, the last
# one holds one pair); W * C / N = 12 ... 560 vectors per row in fp32, 6 ... 280 in bf16 (fewer and more than the 256 of a
# workgroup in both storage types, never a multiple: a second workgroup per row, part of it past the row's end)


def pool_case(B, H, W, Cn, dt, seed, acc):
    """idx as ATen's max_pool2d picks it, dout / base in storage precision; float64 result, its bound"""
    g = torch.Generator().manual_seed(seed)
    x = F.relu(torch.randn(B, Cn, H, W, generator=g))
    _, ind = F.max_pool2d(x, 3, 2, 1, return_indices=True)
    Ho, Wo = H // 2, W // 2
    oy = torch.arange(Ho).view(1, 1, Ho, 1)
    ox = torch.arange(Wo).view(1, 1, 1, Wo)
    tap = (ind // W - (2 * oy - 1)) * 3 + (ind % W - (2 * ox - 1))
    assert int(tap.min()) >= 0 and int(tap.max()) <= 8
    dout = bn.stored(torch.randn(B, Cn, Ho, Wo, generator=g, dtype=torch.float64), dt)
    base = bn.stored(torch.randn(B, Cn, H, W, generator=g, dtype=torch.float64), dt) if acc else torch.zeros(B, Cn, H, W,
                                                                                                            dtype=torch.float64)
    flat = ind.view(B, Cn, -1)

    def scatter(v, dtype=torch.float64):
        return torch.zeros(B, Cn, H * W, dtype=dtype).scatter_add_(2, flat, v.reshape(B, Cn, -1).to(dtype)).view(B, Cn, H, W)

    ref = scatter(dout) + base
    terms = scatter(torch.ones_like(dout)) + (1.0 if acc else 0.0)
    bound = (terms - 1).clamp_min(0) * U24 * (scatter(dout.abs()) + base.abs()) * (1 + 1e-6)
    return tap.to(torch.uint8), dout, base, ref, bound, scatter


@gpu
@pytest.mark.parametrize("acc", [False, True])
@pytest.mark.parametrize("dt", [F32, BF16])
@pytest.mark.parametrize("B,H,W,Cn", POOL_SHAPES)
def test_maxpool_backward(ops, B, H, W, Cn, dt, acc):
    from denoising_diffusion_deep_fake_amd import _lib
    tap, dout, base, ref, bound, _ = pool_case(B, H, W, Cn, dt, 31 + H + W + Cn, acc)
    din = Guarded(B * H * W * Cn, 64 * Cn, tdt(dt))
    if acc:
        din.t.copy_(to_nhwc(base).to(tdt(dt)).reshape(-1))
    d_dev, i_dev = to_nhwc(dout).to(tdt(dt)).to(DEV), to_nhwc(tap).to(DEV)
    _lib.check(_lib.lib().d3f_maxpool3x3s2_backward(dt, _lib.ptr(d_dev), _lib.ptr(i_dev), _lib.ptr(din.t), int(acc), B, H, W,
                                                    Cn, _lib.stream_ptr()))
    torch.cuda.synchronize()
    assert din.intact(), "guard band overwritten"
    out = din.t.cpu().view(B, H, W, Cn).permute(0, 3, 1, 2)
    within(out, ref, bound, dt, f"maxpool backward {B}x{H}x{W}x{Cn} acc{int(acc)}")
    assert bool((ref != 0).any()) and bool((out[ref == 0] == 0).all())


@pytest.mark.parametrize("acc", [False, True])
def test_maxpool_bound_admits_torch_fp32(acc):
    for (B, H, W, Cn) in POOL_SHAPES[:4]:
        _, dout, base, ref, bound, scatter = pool_case(B, H, W, Cn, F32, 31 + H + W + Cn, acc)
        out = scatter(dout, torch.float32) + base.float()
        within(out, ref, bound, F32, "torch fp32")


# ------------------------------------------------------------------------------------------
# layout at the NCHW boundary
# ------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("dt", [F32, BF16])
@pytest.mark.parametrize("Cn,vectors,shift", [(3, 1, 0), (3, 1, 1), (5, 2, 0), (4, 1, 0)])
def test_layout(ops, dt, Cn, vectors, shift):
    """B = 2, 5 x 7 pixels, 3 channels padded to one vector (fp32: 4, bf16: 8 elements): one store per pixel; the same
    into an output one element off 16-byte alignment, and 5 channels padded to two vectors: element stores"""
    from denoising_diffusion_deep_fake_amd import _lib
    B, H, W = 2, 5, 7
    cpad = vectors * (4 if dt == F32 else 8)
    g = torch.Generator().manual_seed(5)
    x = torch.randn(B, Cn, H, W, generator=g)
    n = B * H * W * cpad
    out = Guarded(n + shift, 64, tdt(dt))
    dst = out.t[shift:]
    _lib.check(_lib.lib().d3f_nchw_to_nhwc(dt, _lib.ptr(x.to(DEV)), _lib.ptr(dst), B, Cn, H, W, cpad, _lib.stream_ptr()))
    torch.cuda.synchronize()
    assert out.intact() and bool((out.t[:shift] == SENTINEL).all())
    expect = to_nhwc(x, cpad).to(tdt(dt))
    assert torch.equal(dst.cpu().view(B, H, W, cpad), expect)


# ------------------------------------------------------------------------------------------
# BatchNorm, split form: finalize -> apply, reduce -> finalize -> apply
# ------------------------------------------------------------------------------------------
FORMS = [(0, 1, False), (1, 0, True), (2, 1, True), (2, 2, True), (0, 2, False)]  # (mask, residual form, ReLU)


@gpu
@pytest.mark.parametrize("dt", [F32, BF16])
@pytest.mark.parametrize("mask,res,relu", FORMS)
@pytest.mark.parametrize("rows", [33, 1000])
@pytest.mark.parametrize("Cn", [16, 64, 128])
def test_bn_split_forms(ops, Cn, rows, mask, res, relu, dt):
    dres_mode = 0 if res == 0 else (2 if rows == 33 else 1)
    bn.run_case(ops, Cn, rows, min(rows, 37), dt, False, res=res, relu=relu, mask=mask, fused_rows=0, dres_mode=dres_mode,
                seed=rows + Cn, expect_fused=(False, False), tag=f"helper {Cn}x{rows} mask{mask} res{res} dt{dt}")


@gpu
@pytest.mark.parametrize("dt", [F32, BF16])
@pytest.mark.parametrize("Cn,mask,res,relu", [(16,) + f for f in FORMS] + [(128, 2, 1, True)])
def test_bn_split_forms_above_an_unrolled_trip(ops, Cn, mask, res, relu, dt):
    """four whole grid-stride steps and 33 rows in fp32 (two and 66 vectors in bf16): one trip of the unrolled loop of
    both streaming kernels and one partly filled pass of their remainder loop; 3333 forward partial rows: the eight-, four- and one-row loops of bn_finalize_kernel; the backward rows
    from bn_bwd_reduce (fp32: 1024 of them) or supplied (bf16: 3333, bn_bwd_finalize_kernel's three loops)"""
    dres_mode = 0 if res == 0 else (2 if mask == 2 else 1)
    bn.run_case(ops, Cn, BIG_ROWS[Cn], 3333, dt, False, res=res, relu=relu, mask=mask, fused_rows=3333 if dt == BF16 else 0,
                dres_mode=dres_mode, seed=77 + mask + res, expect_fused=(False, False),
                tag=f"helper big {Cn} mask{mask} res{res} dt{dt}")


@gpu
@pytest.mark.parametrize("dt", [F32, BF16])
def test_bn_split_forms_whole_strides_in_the_remainder_loop(ops, dt):
    """six grid-stride steps and 33 rows in fp32: one unrolled trip of four, then the remainder loop twice in full and
    once partly filled; bf16 (three steps and 66 vectors): one trip of two, the remainder loop once in full and once partly"""
    bn.run_case(ops, 16, MORE_ROWS, 37, dt, False, res=1, relu=True, mask=2, fused_rows=0, dres_mode=2, seed=91,
                expect_fused=(False, False), tag=f"helper more dt{dt}")


def one_row_data(Cn, dt, seed, res):
    g = torch.Generator().manual_seed(seed)
    y = bn.stored(torch.randn(1, Cn, generator=g, dtype=torch.float64), dt)
    r = bn.stored(torch.randn(1, Cn, generator=g, dtype=torch.float64), dt) if res else None
    dA = bn.stored(torch.randn(1, Cn, generator=g, dtype=torch.float64), dt)
    dA[dA == 0] = 1.0
    gamma = (0.5 + torch.rand(Cn, generator=g)) * torch.where(torch.rand(Cn, generator=g) < 0.25, -1.0, 1.0)
    return y, r, dA, gamma.float(), (torch.rand(Cn, generator=g) - 0.5).float()


@gpu
@pytest.mark.parametrize("dt", [F32, BF16])
@pytest.mark.parametrize("mask,res,relu", FORMS)
@pytest.mark.parametrize("Cn", [16, 64, 128])
def test_bn_one_row(ops, Cn, mask, res, relu, dt):
    """one row: every streaming kernel runs one partly filled workgroup, the reduce one row of one pass.  (No torch
    reference: batch_norm refuses one value per channel; the kernels' formulas in float64 stand.)"""
    rng = np.random.default_rng(Cn)
    y, r, dA, gamma, beta = one_row_data(Cn, dt, Cn + mask, res)
    res_coef_dev = res_coef = None
    if res == 2:
        _, _, _, gamma_d, beta_d = one_row_data(Cn, dt, Cn + 500, 0)
        D = bn.Layer(ops, Cn, 1, dt, fwd_rows=1, apply=False, relu=False, allow_fused=False)
        res_coef = D.forward(bn.make_stats(r, 1, Cn, rng), r, gamma_d, beta_d)
        res_coef_dev = D.coef.t
    L = bn.Layer(ops, Cn, 1, dt, 1, Cn, True, relu, res, mask, 0, False)
    assert not L.plan.fwd_fused and not L.plan.bwd_fused
    stats = bn.make_stats(y, 1, Cn, rng)
    coef = L.forward(stats, y, gamma, beta, r, res_coef_dev)
    bn.check_fwd_coef(coef, stats, Cn, 1, gamma, beta)
    a = L.act()
    ref_a, bound = bn.a_formula(coef, y, relu, res, r, res_coef)
    within(a, ref_a, bound, dt, "a")
    keep = (a > 0) if mask else torch.ones_like(a, dtype=torch.bool)
    dz = dA * keep
    dy, dres, dgamma, dbeta, k = L.backward(dA, None, 2 if res else 0, base64=r)
    xh = (y - coef[0].double()) * coef[1].double()
    assert torch.equal(dbeta.double(), dz[0])  # one term: 0 + dz is exact
    within(dgamma.double(), (dz * xh)[0], 3 * U24 * (dz * xh)[0].abs() * (1 + 1e-6), F32, "dgamma")
    k0, k1, k2 = k[0].double(), k[1].double(), k[2].double()
    within(dy, k0 * (dz - k1 - xh * k2), bn.DY_ROUNDINGS * U24 * k0.abs() * (dz.abs() + k1.abs() + (xh * k2).abs()) * (1 + 1e-6),
           dt, "dy")
    if res:
        assert torch.equal(dres, (r.float() + dz.float()).to(tdt(dt)))


@gpu
@pytest.mark.parametrize("tiles", [255, 257, 1024, 1279, 2048, 2049, 3333, 4096])
def test_bn_finalize_rows(ops, tiles):
    """d3f_bn_finalize at C = 16 over the row counts where column_sum2 changes loops (a thread's share: 1 ... 16 rows)"""
    Cn, rows = 16, 5000
    rng = np.random.default_rng(tiles)
    y, _, _, gamma, beta = bn.make_data(Cn, rows, F32, tiles)
    stats = bn.make_stats(y, tiles, Cn, rng)
    g0 = torch.Generator().manual_seed(tiles + 7)
    rm0, rv0 = torch.randn(Cn, generator=g0), 0.5 + torch.rand(Cn, generator=g0)
    rm, rv = rm0.to(DEV), rv0.to(DEV)
    coef = ops.bn_finalize(stats.to(DEV), tiles, Cn, rows, gamma.to(DEV), beta.to(DEV), rm, rv).cpu().reshape(4, Cn)
    bn.check_fwd_coef(coef, stats, Cn, rows, gamma, beta, rm0, rv0, rm.cpu(), rv.cpu())


@gpu
@pytest.mark.parametrize("dt", [F32, BF16])
@pytest.mark.parametrize("Cn,rows", [(16, 1000), (64, 33), (128, 1)])
def test_bn_older_entries(ops, Cn, rows, dt):
    """d3f_bn_apply and d3f_bn_backward (residual tensor, mask from a, dres written) under the same bounds"""
    g = torch.Generator().manual_seed(rows)
    y = bn.stored(torch.randn(rows, Cn, generator=g, dtype=torch.float64) * 1.5 + 0.25, dt)
    r = bn.stored(torch.randn(rows, Cn, generator=g, dtype=torch.float64), dt)
    dA = bn.stored(torch.randn(rows, Cn, generator=g, dtype=torch.float64), dt)
    coef = torch.stack([torch.randn(Cn, generator=g) * 0.1, 0.5 + torch.rand(Cn, generator=g), torch.randn(Cn, generator=g),
                        torch.randn(Cn, generator=g) * 0.2])  # mean, invstd, scale, shift
    gamma = torch.randn(Cn, generator=g)
    dev = lambda t: t.to(tdt(dt)).to(DEV)
    a = ops.bn_apply(dev(y), coef.reshape(-1).to(DEV), residual=dev(r), relu=True, dtype=dt)
    ref_a, bound = bn.a_formula(coef, y, True, 1, r)
    within(a.cpu(), ref_a, bound, dt, "a")
    dy, dres, dgamma, dbeta = ops.bn_backward(dev(dA), a, dev(y), coef.reshape(-1).to(DEV), gamma.to(DEV), want_dres=True,
                                              dtype=dt)
    dz = dA * (a.cpu() > 0)
    assert torch.equal(dres.cpu().double(), dz)
    xh = (y - coef[0].double()) * coef[1].double()
    # the sums the device reports: fp32 sums of `rows` terms in an order not fixed here -- at most rows - 1 roundings
    # of partial sums that never exceed the sum of the absolute terms (second order: the factor behind); a term of
    # dgamma carries three roundings of its own (the difference and the product of xhat, the product with dz); the f64
    # total of the partial rows is rounded once more to fp32
    s1, s2 = dbeta.cpu().double(), dgamma.cpu().double()
    slack = 1 + rows * U24
    assert bool(((s1 - dz.sum(0)).abs() <= rows * U24 * dz.abs().sum(0) * slack).all())
    assert bool(((s2 - (dz * xh).sum(0)).abs() <= (rows + 3) * U24 * (dz * xh).abs().sum(0) * slack).all())
    k0 = (gamma * coef[1]).double()                      # fp32 product, as bn_bwd_coef forms it
    k1, k2 = (s1 / rows).float().double(), (s2 / rows).float().double()
    within(dy.cpu(), k0 * (dz - k1 - xh * k2), bn.DY_ROUNDINGS * U24 * k0.abs() * (dz.abs() + k1.abs() + (xh * k2).abs()) * (1 + 1e-6),
           dt, "dy")


# ------------------------------------------------------------------------------------------
# weight packing: torch layout -> the forward and the data-gradient operand (pack_all_kernel)
# ------------------------------------------------------------------------------------------
# forward   wf[n][(kh * KW + kw) * Cin + c]  = w[n][c][kh][kw]       CoutPad rows of Kpad elements
# gradient  wd[c][slot * CoutD + n]          = w[n][c][taps - 1 - f] CinRows rows of KpadD elements, f = slot -- but for
#           the stride-2 layers whose data gradient runs as output-parity classes (no second source, 3x3 pad 1 or 1x1 pad 0,
#           CoutD whole k-tiles) slot 0 .. 8 holds f = 0, 2, 6, 8, 1, 7, 3, 5, 4
# Cin = C0 padded, CoutPad / CinRows: multiples of 16, CoutD: Cout in whole vectors, Kpad / KpadD: whole k-tiles of 32 (fp32)
# or 64 (bf16) elements; everything outside the real filter is zero.  A workgroup loads a tile of 32 filters x CT
# channels x taps (CT * taps <= 288) eight elements per thread at a time: 2048 per trip.
PACK_CASES = [  # (C0, CinReal, Cout, K, stride, pad): tile elements, what the case is for
    (64, 64, 40, 3, 1, 1),     # 9216 = 4.5 trips; Cout no multiple of 32 (and of 16): zero filters inside a tile
    (64, 64, 128, 3, 2, 1),    # the parity order of the flipped taps
    (64, 64, 128, 1, 2, 0),    # 1024: less than one trip
    (16, 13, 24, 3, 1, 1),     # 4608 = 2.25 trips; CinReal < Cin: zero channels inside a tile; one half-empty filter tile
    (8, 3, 64, 7, 2, 3),       # the stem: 49 taps, CT = 4, 6272 = 3.06 trips; fp32 packs it with C0 = 4
]


def round_up(a, b):
    return (a + b - 1) // b * b


def packed_reference(w, C0, Cout, K, stride, pad, dt):
    ve, bke = (4, 32) if dt == F32 else (8, 64)
    CinReal, taps, Cin = w.shape[1], K * K, C0
    CoutPad, CinRows, CoutD = round_up(Cout, 16), round_up(Cin, 16), round_up(Cout, ve)
    Kpad, KpadD = round_up(taps * Cin, bke), round_up(taps * CoutD, bke)
    wf = torch.zeros(CoutPad, Kpad)
    body = torch.zeros(CoutPad, taps, Cin)
    body[:Cout, :, :CinReal] = w.permute(0, 2, 3, 1).reshape(Cout, taps, CinReal)
    wf[:, :taps * Cin] = body.reshape(CoutPad, -1)
    parity = stride == 2 and CoutD % bke == 0 and ((K == 3 and pad == 1) or (K == 1 and pad == 0))
    flipped = [0, 2, 6, 8, 1, 7, 3, 5, 4] if (parity and taps == 9) else list(range(taps))
    wd = torch.zeros(CinRows, KpadD)
    body = torch.zeros(CinRows, taps, CoutD)
    flat = w.reshape(Cout, CinReal, taps)
    for slot, f in enumerate(flipped):
        body[:CinReal, slot, :Cout] = flat[:, :, taps - 1 - f].t()
    wd[:, :taps * CoutD] = body.reshape(CinRows, -1)
    return wf.to(tdt(dt)), wd.to(tdt(dt))


@gpu
@pytest.mark.parametrize("dt", [F32, BF16])
@pytest.mark.parametrize("C0,CinReal,Cout,K,stride,pad", PACK_CASES)
def test_pack_weights(ops, C0, CinReal, Cout, K, stride, pad, dt):
    import ctypes as C
    from denoising_diffusion_deep_fake_amd import _lib
    if dt == F32 and C0 == 8 and CinReal == 3:
        C0 = 4
    d = ops.make_desc(1, 16, 16, C0, 0, Cout, K, stride, pad, cin_real=CinReal)
    g = torch.Generator().manual_seed(C0 + Cout + K)
    w = torch.randn(Cout, CinReal, K, K, generator=g)
    wf_ref, wd_ref = packed_reference(w, C0, Cout, K, stride, pad, dt)
    L = _lib.lib()
    esz = 4 if dt == F32 else 2
    assert L.d3f_conv_packed_bytes(dt, C.byref(d), 0) == wf_ref.numel() * esz
    assert L.d3f_conv_packed_bytes(dt, C.byref(d), 1) == wd_ref.numel() * esz
    wf, wd = Guarded(wf_ref.numel(), 64, tdt(dt), fill=float("nan")), Guarded(wd_ref.numel(), 64, tdt(dt), fill=float("nan"))
    _lib.check(L.d3f_conv_pack_weights(dt, C.byref(d), _lib.ptr(w.to(DEV)), _lib.ptr(wf.t), _lib.ptr(wd.t), _lib.stream_ptr()))
    torch.cuda.synchronize()
    assert wf.intact() and wd.intact(), "guard band overwritten"
    assert torch.equal(wf.t.cpu().view(wf_ref.shape), wf_ref), "forward layout"
    assert torch.equal(wd.t.cpu().view(wd_ref.shape), wd_ref), "data-gradient layout"
    # ... and each layout packed on its own (one launch each) gives the same bytes
    only = Guarded(wd_ref.numel(), 64, tdt(dt), fill=float("nan"))
    _lib.check(L.d3f_conv_pack_weights(dt, C.byref(d), _lib.ptr(w.to(DEV)), None, _lib.ptr(only.t), _lib.stream_ptr()))
    torch.cuda.synchronize()
    assert only.intact() and torch.equal(only.t.cpu().view(wd_ref.shape), wd_ref)


# ------------------------------------------------------------------------------------------
# the bounds against torch's own fp32 arithmetic (no GPU)
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", [F32, BF16])
@pytest.mark.parametrize("res", [0, 1, 2])
def test_bn_bounds_admit_torch_fp32(dt, res):
    Cn, rows = 64, 1000
    g = torch.Generator().manual_seed(res)
    y = bn.stored(torch.randn(rows, Cn, generator=g, dtype=torch.float64) * 1.5 + 0.25, dt)
    r = bn.stored(torch.randn(rows, Cn, generator=g, dtype=torch.float64), dt)
    dA = bn.stored(torch.randn(rows, Cn, generator=g, dtype=torch.float64), dt)
    coef = torch.stack([torch.randn(Cn, generator=g) * 0.1, 0.5 + torch.rand(Cn, generator=g), torch.randn(Cn, generator=g),
                        torch.randn(Cn, generator=g) * 0.2])
    rc = torch.stack([coef[0], coef[1], torch.randn(Cn, generator=g), torch.randn(Cn, generator=g)])
    k = torch.randn(3, Cn, generator=g)
    a32 = y.float() * coef[2] + coef[3]
    if res == 1:
        a32 = a32 + r.float()
    elif res == 2:
        a32 = a32 + (r.float() * rc[2] + rc[3])
    a32 = a32.clamp_min(0.0).to(tdt(dt))
    ref_a, bound = bn.a_formula(coef, y, True, res, r, rc)
    within(a32, ref_a, bound, dt, "a")
    dz = dA * (a32 > 0)
    xh32 = (y.float() - coef[0]) * coef[1]
    dy32 = (k[0] * (dz.float() - k[1] - xh32 * k[2])).to(tdt(dt))
    xh = (y - coef[0].double()) * coef[1].double()
    k0, k1, k2 = k[0].double(), k[1].double(), k[2].double()
    within(dy32, k0 * (dz - k1 - xh * k2), bn.DY_ROUNDINGS * U24 * k0.abs() * (dz.abs() + k1.abs() + (xh * k2).abs()) * (1 + 1e-6),
           dt, "dy")


# ------------------------------------------------------------------------------------------
# (MSE + 1 - SSIM) / 2 and its gradient: ssim_fwd_kernel, ssim_mse_bwd_kernel, loss_finalize_kernel
# ------------------------------------------------------------------------------------------
# The criterion is no single expression with one magnitude: variances are differences of filtered moments and four
# quotients follow.  The bound is therefore carried THROUGH the expression: E is a float64 value with a bound on the
# distance of the fp32 evaluation from it, and every operation adds its own rounding, 2^-24 of its result, to what its
# operands bring (first order plus the product of the operands' errors) -- per element the operation count times 2^-24
# of the magnitude, weighted by what each operation's result is multiplied by afterwards.
class E:
    def __init__(self, val, err=None):
        self.val = val
        self.err = torch.zeros_like(val) if err is None else err

    @staticmethod
    def lift(x):
        return x if isinstance(x, E) else E(torch.as_tensor(x, dtype=torch.float64))

    def _rounded(self, val, err):
        return E(val, err + U24 * (val.abs() + err))

    def __add__(self, o):
        o = E.lift(o)
        return self._rounded(self.val + o.val, self.err + o.err)

    def __sub__(self, o):
        o = E.lift(o)
        return self._rounded(self.val - o.val, self.err + o.err)

    def __mul__(self, o):
        o = E.lift(o)
        return self._rounded(self.val * o.val, self.val.abs() * o.err + o.val.abs() * self.err + self.err * o.err)

    def __truediv__(self, o):
        o = E.lift(o)
        q = self.val / o.val
        assert bool((o.val.abs() > 2 * o.err).all()), "a divisor the bound cannot separate from 0"
        return self._rounded(q, (self.err + q.abs() * o.err) / (o.val.abs() - o.err))

    def twice(self):  # exact in binary floating point
        return E(2 * self.val, 2 * self.err)

    def neg(self):
        return E(-self.val, self.err)

    def clip01(self):  # 1-Lipschitz
        return E(self.val.clamp(0.0, 1.0), self.err)


def gauss_window():
    """the 11 fp32 weights as make_gauss forms them (libm's expf and numpy's may differ in the last place: FILTER_OPS)"""
    d = np.arange(11, dtype=np.float32) - np.float32(5.0)
    g = np.exp(-(d * d) / np.float32(2.0 * 1.5 * 1.5)).astype(np.float32)
    s = np.float32(0.0)
    for v in g:
        s = np.float32(s + v)
    return torch.from_numpy((g / s).astype(np.float32)).double()


FILTER_OPS = 11 + 10 + 2  # products, sums, and a weight that may sit one place off (2^-23 relative)


def filter1d(x, dim, adjoint):
    """x: E [planes, H, W]; valid filtering, or its adjoint (the full correlation with the flipped window)"""
    g = gauss_window()
    w = g.flip(0) if adjoint else g
    shape = [1, 1, 11, 1] if dim == 1 else [1, 1, 1, 11]
    pad = (0, 0, 10, 10) if dim == 1 else (10, 10, 0, 0)

    def run(t):
        t = t.unsqueeze(1)
        if adjoint:
            t = F.pad(t, pad)
        return F.conv2d(t, w.view(shape)).squeeze(1)

    val = run(x.val)
    # every partial sum is at most the sum of the absolute products (the weights are positive)
    return E(val, run(x.err) + FILTER_OPS * U24 * run(x.val.abs() + x.err) * (1 + 1e-6))


def loss_reference(p, t, lo=-1.0, hi=1.0):
    """the kernels' formulas on [planes, H, W] float64 inputs holding fp32 values: loss, mse, ssim and the gradient as E"""
    f32 = lambda v: float(np.float32(v))
    planes, H, W = p.shape
    rng_ = f32(np.float32(hi) - np.float32(lo))
    rawx = (E(p) - lo) / rng_
    xh, yh = rawx.clip01(), ((E(t) - lo) / rng_).clip01()
    both = lambda q: filter1d(filter1d(q, 1, False), 2, False)
    mux, muy, m2, m3, m4 = both(xh), both(yh), both(xh * xh), both(yh * yh), both(xh * yh)
    c1, c2 = f32(np.float32(0.01) * np.float32(0.01)), f32(np.float32(0.03) * np.float32(0.03))
    sxx, syy, sxy = m2 - mux * mux, m3 - muy * muy, m4 - mux * muy
    a1, b1 = (mux.twice() * muy) + c1, (mux * mux + muy * muy) + c1
    a2, b2 = sxy.twice() + c2, (sxx + syy) + c2
    l, cs = a1 / b1, a2 / b2
    ss = l * cs
    dl = (muy - l * mux).twice() / b1
    dcs = (mux.twice() * cs - muy.twice()) / b2
    dA, dB, dC = cs * dl + l * dcs, (l.neg() * cs) / b2, l.twice() / b2
    back = lambda q: filter1d(filter1d(q, 1, True), 2, True)
    ga, gb, gc = back(dA), back(dB), back(dC)
    gx = (ga + xh.twice() * gb) + yh * gc
    inv_range = E(torch.tensor(1.0, dtype=torch.float64)) / rng_
    gx = gx * inv_range
    inside = (rawx.val >= 0) & (rawx.val <= 1)
    margin = torch.minimum(rawx.val.abs(), (rawx.val - 1).abs())
    assert bool((margin[margin > 0] > 4 * rawx.err[margin > 0]).all()), "an input the bound cannot place against the clip"
    gx = E(torch.where(inside, gx.val, torch.zeros_like(gx.val)), torch.where(inside, gx.err, torch.zeros_like(gx.err)))
    n_ssim, n = float(ss.val.numel()), float(p.numel())
    diff = E(p) - E(t)
    grad = gx * f32(-0.5 / n_ssim) + diff * f32(1.0 / n)
    # a tile's partial sum: at most 1024 terms through a few adds per thread, six shuffle steps and a tree of four: 13
    # roundings of sums that are at most the sum of the absolute terms; the f64 total, one division, one rounding to fp32
    def mean(q, count):
        tot = q.val.sum() / count
        return E(tot, (q.err.sum() + 13 * U24 * (q.val.abs() + q.err).sum()) / count * (1 + 1e-6) + U24 * tot.abs())

    ssim, mse = mean(ss, n_ssim), mean(diff * diff, n)
    loss = (mse + (E.lift(1.0) - ssim))
    return E(loss.val / 2, loss.err / 2), mse, ssim, grad


def loss_inputs(B, H, W, seed):
    g = torch.Generator().manual_seed(seed)
    yy, xx = torch.meshgrid(torch.linspace(0, 3, H), torch.linspace(0, 3, W), indexing="ij")
    t = (0.6 * torch.sin(yy * 2.1 + 0.3) * torch.cos(xx * 1.7) + 0.1 * torch.randn(B, 3, H, W, generator=g)).clamp(-0.95, 0.95)
    p = (t + 0.3 * torch.randn(B, 3, H, W, generator=g)).clamp(-0.95, 0.95)
    p[0, 0, :3, :3] = 1.7    # outside the range on both sides: the clip and its zero gradient
    p[0, 1, 4, 5] = -1.4
    return p.float().contiguous(), t.float().contiguous()


def hold(name, got, ref):
    err = (torch.as_tensor(got).double() - ref.val).abs()
    bad = err > ref.err * (1 + 1e-3)
    assert not bool(bad.any()), (name, int(bad.sum()), float((err / ref.err.clamp_min(1e-300)).max()))


LOSS_SHAPES = [(2, 12, 12), (2, 43, 45)]  # one partial tile; ragged tiles in both directions (valid maps 33 x 35)


@gpu
@pytest.mark.parametrize("B,H,W", LOSS_SHAPES)
def test_mse_ssim_loss(ops, B, H, W):
    p, t = loss_inputs(B, H, W, H)
    loss, mse, ssim, grad = loss_reference(p.double().view(-1, H, W), t.double().view(-1, H, W))
    out, g = ops.mse_ssim_loss(p.to(DEV), t.to(DEV))
    out, g = out.cpu(), g.cpu()
    hold("gradient", g.view(-1, H, W), grad)
    hold("loss", out[0], loss)
    hold("mse", out[1], mse)
    hold("ssim", out[2], ssim)
    assert bool((g[0, 0, :3, :3] == (p - t)[0, 0, :3, :3] * np.float32(1.0 / p.numel())).all())  # clipped: the MSE term alone


@pytest.mark.parametrize("B,H,W", LOSS_SHAPES)
def test_loss_bound_admits_torch_fp32(B, H, W):
    """the same formulas in torch fp32 (conv2d's own summation order) stay inside the carried bound, and the float64
    values agree with autograd through the plain float64 criterion"""
    p, t = loss_inputs(B, H, W, H)
    loss, mse, ssim, grad = loss_reference(p.double().view(-1, H, W), t.double().view(-1, H, W))
    g32 = gauss_window().float()

    def criterion(pp, tt, g):
        x, y = ((pp + 1) / 2).clamp(0, 1).view(-1, 1, H, W), ((tt + 1) / 2).clamp(0, 1).view(-1, 1, H, W)
        f = lambda q: F.conv2d(F.conv2d(q, g.view(1, 1, 11, 1)), g.view(1, 1, 1, 11))
        mux, muy = f(x), f(y)
        sxx, syy, sxy = f(x * x) - mux * mux, f(y * y) - muy * muy, f(x * y) - mux * muy
        ss = ((2 * mux * muy + 0.01 ** 2) / (mux * mux + muy * muy + 0.01 ** 2)) * ((2 * sxy + 0.03 ** 2) / (sxx + syy + 0.03 ** 2))
        m = ((pp - tt) ** 2).mean()
        return (m + (1 - ss.mean())) / 2, m, ss.mean()

    for dtype, g in ((torch.float32, g32), (torch.float64, gauss_window())):
        pp = p.detach().clone().to(dtype).requires_grad_(True)
        lo, m, s = criterion(pp, t.to(dtype), g)
        lo.backward()
        if dtype == torch.float32:
            hold("gradient", pp.grad.view(-1, H, W), grad)
            hold("loss", lo.detach(), loss)
            hold("mse", m.detach(), mse)
            hold("ssim", s.detach(), ssim)
        else:  # float64 autograd against the float64 values of the kernels' formulas: the formulas are the criterion's
            # (up to the kernels' constants, which are fp32 numbers: 0.01f * 0.01f, (float)(-0.5 / n), ...: 2^-23 each)
            d = float((pp.grad.view(-1, H, W) - grad.val).abs().max())
            print("formula against float64 autograd:", d / float(grad.val.abs().max()), abs(float(lo.detach()) - float(loss.val)))
            assert d < 1e-6 * float(grad.val.abs().max())
            assert abs(float(lo.detach()) - float(loss.val)) < 1e-7
