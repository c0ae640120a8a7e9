"""GPU: every convolution kernel form at operator level against float64, element by element.

The cases, the float64 reference and the derived bounds are tests/conv_cases.py (its docstring states the bounds and
counts every rounding); tests/test_cpu_conv_forms.py holds the table to the planner.  Here every case runs through the
C ABI directly -- d3f_conv_pack_weights, d3f_conv_forward, d3f_conv_backward_data (+ d3f_upsample2x_backward where the
route needs it), d3f_conv_backward_weight, d3f_conv_winograd_* -- and each call is checked five ways:

* every element: |got - ref| <= bound, no exempt share; the aggregate gates of the older operator tests stay beside it
  (rel-L2 1e-5 in fp32, 4e-3 in bf16 storage, 1e-5 for the fp32 weight gradient of either);
* statistics: rows [0, stat_rows) x [0, Cout) finite and inside their bounds, every row behind them still NaN;
* guards: y, dx0, dx1, the full-resolution scratch, dw, the statistics, the split-K workspace, the weight-gradient
  slabs and the packed weights each sit between sentinel bands of at least 64 rows that must survive; outputs start as
  the sentinel, statistics as NaN, packed weights and both workspaces as NaN bytes, the pad channels of an input with
  cin_real < C0 as finite garbage (dY pad channels stay zero: d3f_head_activation_backward's contract);
* every call runs twice from the same poisoned state and must give the same bits (no result path has an atomic);
* acc0 / acc1: a second data-gradient call accumulates into a random base and is held to base + gradient under the one
  counted extra addition;
* exact operands: every case runs a second time (test_conv_case_exact) on conv_cases.make_exact_data -- operands in
  {-1, 0, 1}, on which fp32 arithmetic makes no rounding error in any order -- through the same guards, poison, garbage pad
  channels and repeat, and every result must EQUAL the float64 one passed through the route's storage roundings
  (conv_cases.py lists them); a failure reports how many elements differ and the first index.

Winograd F(2x2, 3x3) goes through d3f_conv_winograd_pack / d3f_conv_winograd_forward: the raw output under its own
per-element bound gamma_(C + 10) * Ymag (conv_cases.py has the analysis), both statistics sums under the bounds derived
from it, and the eval epilogue of the same kernel -- relu?(conv * scale + shift + residual?), all four variants, the
residual behind guard bands -- under |scale| * E_o + k * 2^-24 * (|o scale| + |shift| + |res|).

What launches what (python tests/conv_cases.py prints it from the plan structs; kernel instantiation, its form tuple --
(dtype 0 f32 / 1 bf16 / 2 f32x3, launch, patch, tile_bm, tile_bn, par, nz, small_c, fast_addr, sum2, splitk > 1) or
(dtype, "wgrad", part, cls, patch variant, tile) -- and the cases that reach it):

conv_igemm_kernel<float, 128, 64, FAST 1>
    (0, 'dgrad', 0, 128, 64, 0, 1, 0, 1, 0, 0)
    <- f32-16x16x128-8+64to32-k3s1-up0-ws0
conv_igemm_kernel<float, 128, 64, FAST 1> par 1
    (0, 'dgrad', 0, 128, 64, 1, 4, 0, 1, 0, 0)
    <- f32-16x16x128-96+0to32-k3s2-up0-ws0
conv_igemm_kernel<float, 256, 16, SMALLC>
    (0, 'dgrad', 0, 256, 16, 0, 1, 1, 0, 0, 0)
    <- f32-2x16x16-16+0to16-k3s1-up2-ws0, f32-2x24x40-16+0to3-k3s1-up0-ws0
conv_igemm_kernel<float, 256, 32, FAST 1>
    (0, 'dgrad', 0, 256, 32, 0, 1, 0, 1, 0, 0)
    <- f32-3x10x10-32+0to64-k3s1-up0-ws0, f32-1x4x4-32+32to32-k3s1-up2-ws1, f32-1x4x4-32+32to64-k3s1-up2-ws0
conv_igemm_kernel<float, 256, 32, FAST 1> par 2
    (0, 'dgrad', 0, 256, 32, 2, 1, 0, 1, 0, 0)
    <- f32-12x64x64-32+0to96-k1s2-up0-ws0
conv_igemm_kernel<float, 32, 32, FAST 1>
    (0, 'dgrad', 0, 32, 32, 0, 1, 0, 1, 0, 0)
    <- f32-1x24x40-64+64to32-k3s1-up2-ws0
conv_igemm_kernel<float, 32, 32, FAST 1> + conv_splitk_reduce_kernel
    (0, 'dgrad', 0, 32, 32, 0, 1, 0, 1, 0, 1)
    <- f32-3x12x20-128+64to128-k3s1-up2-ws1
conv_igemm_kernel<float, 32, 32, FAST 1> par 1
    (0, 'dgrad', 0, 32, 32, 1, 4, 0, 1, 0, 0)
    <- f32-1x4x4-64+0to32-k3s2-up0-ws0
conv_igemm_kernel<float, 32, 32, FAST 1> par 2
    (0, 'dgrad', 0, 32, 32, 2, 1, 0, 1, 0, 0)
    <- f32-1x4x4-512+0to64-k1s2-up0-ws1
conv_igemm_kernel<float, 64, 64, FAST 1>
    (0, 'dgrad', 0, 64, 64, 0, 1, 0, 1, 0, 0)
    <- f32-1x4x4-8+32to32-k3s1-up0-ws0
conv_igemm_kernel<float, 64, 64, FAST 1> par 1
    (0, 'dgrad', 0, 64, 64, 1, 4, 0, 1, 0, 0)
    <- f32-3x56x72-96+0to32-k3s2-up0-ws0
conv_patch_kernel<float, 16 | 4, 16>
    (0, 'dgrad', 1, 0, 0, 0, 1, 0, 0, 0, 0)
    <- f32-5x128x128-16+0to16-k3s1-up0-ws0, f32-2x8x64-16+0to3-k3s1-up0-ws0
conv_igemm_kernel<float, 128, 64, FAST 1>
    (0, 'dgrad_lo', 0, 128, 64, 0, 1, 0, 1, 0, 0)
    <- f32-8x128x128-96+0to32-k3s1-up2-ws0
conv_igemm_kernel<float, 256, 32, FAST 1>
    (0, 'dgrad_lo', 0, 256, 32, 0, 1, 0, 1, 0, 0)
    <- f32-1x4x4-32+32to64-k3s1-up2-ws0
conv_igemm_kernel<float, 256, 32, FAST 1> + conv_splitk_reduce_kernel
    (0, 'dgrad_lo', 0, 256, 32, 0, 1, 0, 1, 0, 1)
    <- f32-1x4x4-32+32to32-k3s1-up2-ws1
conv_igemm_kernel<float, 256, 32, SMALLC>
    (0, 'dgrad_lo', 0, 256, 32, 0, 1, 1, 0, 0, 0)
    <- f32-1x4x4-32+0to8-k3s1-up2-ws0
conv_igemm_kernel<float, 32, 32, FAST 1>
    (0, 'dgrad_lo', 0, 32, 32, 0, 1, 0, 1, 0, 0)
    <- f32-1x24x40-64+64to32-k3s1-up2-ws0
conv_igemm_kernel<float, 32, 32, FAST 1> + conv_splitk_reduce_kernel
    (0, 'dgrad_lo', 0, 32, 32, 0, 1, 0, 1, 0, 1)
    <- f32-3x12x20-128+64to128-k3s1-up2-ws1
conv_igemm_kernel<float, 64, 64, FAST 1>
    (0, 'dgrad_lo', 0, 64, 64, 0, 1, 0, 1, 0, 0)
    <- f32-12x64x64-96+0to32-k3s1-up2-ws0
conv_winograd_kernel
    (0, 'fwd', 'wino')
    <- f32-1x16x16-16+0to64-k3s1-up0-ws0-wino, f32-1x16x16-32+0to64-k3s1-up0-ws0-wino, f32-2x32x48-48+0to128-k3s1-up0-ws0-wino
    (1, 2 and 3 chunks of 16 channels: the last chunk contracted from V[0], V[1], V[0]; raw output + statistics rows,
    and the eval epilogue {no residual, residual} x {no ReLU, ReLU})
conv_igemm_kernel<float, 128, 64, FAST 2 (up-folded)>
    (0, 'fwd', 0, 128, 64, 3, 4, 0, 0, 0, 0)
    <- f32-16x16x128-32+32to96-k3s1-up2-ws0
conv_igemm_kernel<float, 256, 16, SMALLC>
    (0, 'fwd', 0, 256, 16, 0, 1, 1, 0, 0, 0)
    <- f32-2x16x16-16+0to16-k3s1-up2-ws0
conv_igemm_kernel<float, 256, 16, FAST 2 (up-folded)>
    (0, 'fwd', 0, 256, 16, 3, 4, 0, 1, 0, 0)
    <- f32-1x4x4-32+0to8-k3s1-up2-ws0
conv_igemm_kernel<float, 256, 32, FAST 1>
    (0, 'fwd', 0, 256, 32, 0, 1, 0, 1, 0, 0)
    <- f32-1x4x4-64+0to32-k3s2-up0-ws0, f32-3x56x72-96+0to32-k3s2-up0-ws0, f32-16x16x128-96+0to32-k3s2-up0-ws0
conv_igemm_kernel<float, 256, 32, FAST 2 (up-folded)>
    (0, 'fwd', 0, 256, 32, 3, 4, 0, 0, 0, 0)
    <- f32-1x24x40-64+64to32-k3s1-up2-ws0
conv_igemm_kernel<float, 256, 32, FAST 2 (up-folded)> + conv_splitk_reduce_kernel
    (0, 'fwd', 0, 256, 32, 3, 4, 0, 0, 0, 1)
    <- f32-1x4x4-32+32to32-k3s1-up2-ws1
conv_igemm_kernel<float, 32, 32, FAST 1>
    (0, 'fwd', 0, 32, 32, 0, 1, 0, 1, 0, 0)
    <- f32-3x10x10-32+0to64-k3s1-up0-ws0
conv_igemm_kernel<float, 32, 32, FAST 1> + conv_splitk_reduce_kernel
    (0, 'fwd', 0, 32, 32, 0, 1, 0, 1, 0, 1)
    <- f32-1x4x4-512+0to64-k1s2-up0-ws1
conv_igemm_kernel<float, 32, 32, FAST 2 (up-folded)>
    (0, 'fwd', 0, 32, 32, 3, 4, 0, 0, 0, 0)
    <- f32-1x4x4-32+32to64-k3s1-up2-ws0
conv_igemm_kernel<float, 32, 32, FAST 2 (up-folded)> + conv_splitk_reduce_kernel
    (0, 'fwd', 0, 32, 32, 3, 4, 0, 0, 0, 1)
    <- f32-3x12x20-128+64to128-k3s1-up2-ws1
conv_igemm_kernel<float, 64, 64, FAST 1>
    (0, 'fwd', 0, 64, 64, 0, 1, 0, 1, 0, 0)
    <- f32-12x64x64-32+0to96-k1s2-up0-ws0
conv_igemm_kernel<float, 64, 64, FAST 2 (up-folded)>
    (0, 'fwd', 0, 64, 64, 3, 4, 0, 0, 0, 0)
    <- f32-3x56x72-32+32to96-k3s1-up2-ws0
conv_patch_kernel<float, 16 | 4, 16>
    (0, 'fwd', 1, 0, 0, 0, 1, 0, 0, 0, 0)
    <- f32-5x128x128-16+0to16-k3s1-up0-ws0
conv_stem_kernel
    (0, 'fwd', 2, 0, 0, 0, 1, 0, 0, 0, 0)
    <- f32-2x32x64-4+0to64-k7s2-up0-ws0
conv_wgrad_kernel<float, 32, 32, 1, 1, 4> + wgrad_reduce_batch_kernel
    (0, 'wgrad', 0, 0, 0, 32)
    <- f32-3x10x10-32+0to64-k3s1-up0-ws0, f32-1x4x4-64+0to32-k3s2-up0-ws0, f32-12x64x64-32+0to96-k1s2-up0-ws0, f32-3x56x72-96+0to32-k3s2-up0-ws0, f32-16x16x128-96+0to32-k3s2-up0-ws0
conv_wgrad_kernel<float, 64, 64, 2, 2, 1> + wgrad_reduce_batch_kernel
    (0, 'wgrad', 0, 0, 0, 64)
    <- f32-1x4x4-512+0to64-k1s2-up0-ws1
conv_wgrad_patch_kernel<float, 16, 32, 3, 1, 16> + wgrad_reduce_batch_kernel
    (0, 'wgrad', 0, 0, 1, 0)
    <- f32-5x128x128-32+0to16-k3s1-up0-ws0
conv_wgrad_patch_kernel<float, 16, 16, 3, 1, 16> + wgrad_reduce_batch_kernel
    (0, 'wgrad', 0, 0, 2, 0)
    <- f32-5x128x128-16+0to16-k3s1-up0-ws0, f32-2x16x16-16+0to16-k3s1-up2-ws0, f32-2x24x40-16+0to3-k3s1-up0-ws0, f32-2x8x64-16+0to3-k3s1-up0-ws0
conv_wgrad_patch_kernel<float, 32, 32, 3, 1, 16> + wgrad_reduce_batch_kernel
    (0, 'wgrad', 0, 0, 3, 0)
    <- f32-5x128x128-32+0to32-k3s1-up0-ws0
conv_wgrad_patch_kernel<float, 32, 4, 7, 2, 16, 3> + wgrad_reduce_batch_kernel
    (0, 'wgrad', 0, 0, 4, 0)
    <- f32-5x256x256-4+0to32-k7s2-up0-ws0, f32-2x32x64-4+0to64-k7s2-up0-ws0
conv_wgrad_kernel<float, 64, 64, 2, 2, 1, CLS> + wgrad_reduce_batch_kernel
    (0, 'wgrad', 1, 1, 0, 64)
    <- f32-3x12x20-128+64to128-k3s1-up2-ws1
conv_wgrad_patch_cls_kernel<float, 16, 32, 16> + wgrad_reduce_batch_kernel
    (0, 'wgrad', 1, 1, 1, 0)
    <- f32-5x128x128-32+0to16-k3s1-up2-ws0, f32-1x4x4-32+0to8-k3s1-up2-ws0
conv_wgrad_patch_cls_kernel<float, 32, 32, 16> + wgrad_reduce_batch_kernel
    (0, 'wgrad', 1, 1, 3, 0)
    <- f32-1x24x40-64+64to32-k3s1-up2-ws0, f32-1x4x4-32+32to32-k3s1-up2-ws1
conv_wgrad_kernel<float, 64, 64, 2, 2, 1> + wgrad_reduce_batch_kernel
    (0, 'wgrad', 2, 0, 0, 64)
    <- f32-3x12x20-128+64to128-k3s1-up2-ws1
conv_wgrad_patch_kernel<float, 32, 32, 3, 1, 16> + wgrad_reduce_batch_kernel
    (0, 'wgrad', 2, 0, 3, 0)
    <- f32-1x24x40-64+64to32-k3s1-up2-ws0, f32-1x4x4-32+32to32-k3s1-up2-ws1
conv_igemm_kernel<bf16_t, 128, 64, SMALLC>
    (1, 'dgrad', 0, 128, 64, 0, 1, 1, 0, 0, 0)
    <- bf16-16x16x128-128+0to32-k3s1-up0-ws0
conv_igemm_kernel<bf16_t, 128, 64, FAST 1> par 1
    (1, 'dgrad', 0, 128, 64, 1, 4, 0, 1, 0, 0)
    <- bf16-16x16x128-96+0to64-k3s2-up0-ws0
conv_igemm_kernel<bf16_t, 256, 32, SMALLC>
    (1, 'dgrad', 0, 256, 32, 0, 1, 1, 0, 0, 0)
    <- bf16-2x8x64-32+0to16-k3s1-up1-ws0, bf16-1x12x128-32+0to8-k3s1-up2-ws0, bf16-3x4x64-32+0to24-k3s1-up0-ws0
conv_igemm_kernel<bf16_t, 32, 32, FAST 1>
    (1, 'dgrad', 0, 32, 32, 0, 1, 0, 1, 0, 0)
    <- bf16-1x4x4-64+64to256-k3s1-up2-ws0
conv_igemm_kernel<bf16_t, 32, 32, FAST 1> + conv_splitk_reduce_kernel
    (1, 'dgrad', 0, 32, 32, 0, 1, 0, 1, 0, 1)
    <- bf16-3x12x20-128+64to128-k3s1-up2-ws1
conv_igemm_kernel<bf16_t, 32, 32, SMALLC>
    (1, 'dgrad', 0, 32, 32, 0, 1, 1, 0, 0, 0)
    <- bf16-1x4x4-64+64to32-k3s1-up2-ws0, bf16-1x4x4-64+64to32-k3s1-up2-ws1
conv_igemm_kernel<bf16_t, 32, 32, FAST 1> par 1
    (1, 'dgrad', 0, 32, 32, 1, 4, 0, 1, 0, 0)
    <- bf16-1x4x4-128+0to64-k3s2-up0-ws1
conv_igemm_kernel<bf16_t, 32, 32, FAST 1> par 2
    (1, 'dgrad', 0, 32, 32, 2, 1, 0, 1, 0, 0)
    <- bf16-1x4x4-64+0to64-k1s2-up0-ws0
conv_igemm_kernel<bf16_t, 64, 32, FAST 1>
    (1, 'dgrad', 0, 64, 32, 0, 1, 0, 1, 0, 0)
    <- bf16-12x8x64-32+64to64-k3s1-up0-ws0
conv_igemm_kernel<bf16_t, 64, 32, FAST 1> par 1
    (1, 'dgrad', 0, 64, 32, 1, 4, 0, 1, 0, 0)
    <- bf16-12x8x64-96+0to64-k3s2-up0-ws0
conv_igemm_kernel<bf16_t, 64, 32, FAST 1> par 2
    (1, 'dgrad', 0, 64, 32, 2, 1, 0, 1, 0, 0)
    <- bf16-16x12x128-96+0to64-k1s2-up0-ws0
conv_igemm_kernel<bf16_t, 64, 64, FAST 1>
    (1, 'dgrad', 0, 64, 64, 0, 1, 0, 1, 0, 0)
    <- bf16-1x4x4-8+32to64-k3s1-up0-ws0
conv_igemm_kernel<bf16_t, 64, 64, SMALLC>
    (1, 'dgrad', 0, 64, 64, 0, 1, 1, 0, 0, 0)
    <- bf16-16x12x128-64+0to96-k1s2-up0-ws0, bf16-12x64x64-64+0to96-k1s2-up0-ws0
conv_igemm_kernel<bf16_t, 64, 64, FAST 1> par 1
    (1, 'dgrad', 0, 64, 64, 1, 4, 0, 1, 0, 0)
    <- bf16-3x56x72-96+0to64-k3s2-up0-ws0
conv_pres_kernel<128, 32, 4, 1, 1, 1> (one weight stage)
    (1, 'dgrad', 10, 0, 0, 0, 1, 0, 0, 0, 0)
    <- bf16-16x16x128-32+0to128-k3s1-up0-ws0
conv_pres_kernel<256, 16, 2, 1, 2, 1> (one weight stage)
    (1, 'dgrad', 11, 0, 0, 0, 1, 0, 0, 0, 0)
    <- bf16-16x32x32-32+0to256-k3s1-up0-ws0
conv_pres_kernel<512, 8, 1, 1, 4, 2> (one weight stage)
    (1, 'dgrad', 12, 0, 0, 0, 1, 0, 0, 0, 0)
    <- bf16-8x32x32-32+0to512-k3s1-up0-ws0
conv_patch_kernel<bf16_t, 16, 16>
    (1, 'dgrad', 3, 0, 0, 0, 1, 0, 0, 0, 0)
    <- bf16-3x128x128-16+0to16-k3s1-up0-ws0
conv_patch_kernel<bf16_t, 32, 32>
    (1, 'dgrad', 4, 0, 0, 0, 1, 0, 0, 0, 0)
    <- bf16-1x12x128-48+0to32-k3s1-up0-ws0
conv_patch_kernel<bf16_t, 16, 16, false, 8>
    (1, 'dgrad', 6, 0, 0, 0, 1, 0, 0, 0, 0)
    <- bf16-1x12x128-16+0to3-k3s1-up0-ws0
conv_patch_kernel<bf16_t, 16, 32, false, 16, SUM2>
    (1, 'dgrad', 7, 0, 0, 0, 1, 0, 0, 1, 0)
    <- bf16-1x4x64-32+0to16-k3s1-up2-ws0
conv_pres_kernel<64, 64, 2, 2, 1, 2> (one weight stage)
    (1, 'dgrad', 9, 0, 0, 0, 1, 0, 0, 0, 0)
    <- bf16-12x64x64-64+0to64-k3s1-up0-ws0
conv_igemm_kernel<bf16_t, 128, 64, SMALLC>
    (1, 'dgrad_lo', 0, 128, 64, 0, 1, 1, 0, 0, 0)
    <- bf16-16x128x128-64+0to3-k3s1-up2-ws0
conv_igemm_kernel<bf16_t, 32, 32, FAST 1>
    (1, 'dgrad_lo', 0, 32, 32, 0, 1, 0, 1, 0, 0)
    <- bf16-1x4x4-64+64to256-k3s1-up2-ws0
conv_igemm_kernel<bf16_t, 32, 32, FAST 1> + conv_splitk_reduce_kernel
    (1, 'dgrad_lo', 0, 32, 32, 0, 1, 0, 1, 0, 1)
    <- bf16-3x12x20-128+64to128-k3s1-up2-ws1
conv_igemm_kernel<bf16_t, 32, 32, SMALLC>
    (1, 'dgrad_lo', 0, 32, 32, 0, 1, 1, 0, 0, 0)
    <- bf16-1x4x4-64+64to32-k3s1-up2-ws0, bf16-1x4x4-64+64to32-k3s1-up2-ws1
conv_igemm_kernel<bf16_t, 64, 32, FAST 1>
    (1, 'dgrad_lo', 0, 64, 32, 0, 1, 0, 1, 0, 0)
    <- bf16-3x56x72-256+0to64-k3s1-up2-ws0
conv_igemm_kernel<bf16_t, 64, 32, SMALLC>
    (1, 'dgrad_lo', 0, 64, 32, 0, 1, 1, 0, 0, 0)
    <- bf16-3x56x72-256+0to3-k3s1-up2-ws0
conv_igemm_kernel<bf16_t, 64, 64, FAST 1>
    (1, 'dgrad_lo', 0, 64, 64, 0, 1, 0, 1, 0, 0)
    <- bf16-3x56x72-512+0to64-k3s1-up2-ws0
conv_igemm_kernel<bf16_t, 64, 64, SMALLC>
    (1, 'dgrad_lo', 0, 64, 64, 0, 1, 1, 0, 0, 0)
    <- bf16-3x56x72-512+0to3-k3s1-up2-ws0
conv_igemm_kernel<bf16_t, 128, 64, FAST 2 (up-folded)>
    (1, 'fwd', 0, 128, 64, 3, 4, 0, 0, 0, 0)
    <- bf16-16x16x128-64+64to96-k3s1-up2-ws0
conv_igemm_kernel<bf16_t, 256, 32, SMALLC>
    (1, 'fwd', 0, 256, 32, 0, 1, 1, 0, 0, 0)
    <- bf16-1x12x128-48+0to32-k3s1-up0-ws0
conv_igemm_kernel<bf16_t, 256, 32, FAST 2 (up-folded)>
    (1, 'fwd', 0, 256, 32, 3, 4, 0, 0, 0, 0)
    <- bf16-1x4x4-64+64to32-k3s1-up2-ws0
conv_igemm_kernel<bf16_t, 256, 32, FAST 2 (up-folded)> + conv_splitk_reduce_kernel
    (1, 'fwd', 0, 256, 32, 3, 4, 0, 0, 0, 1)
    <- bf16-1x4x4-64+64to32-k3s1-up2-ws1
conv_igemm_kernel<bf16_t, 32, 32, FAST 1>
    (1, 'fwd', 0, 32, 32, 0, 1, 0, 1, 0, 0)
    <- bf16-1x4x4-64+0to64-k1s2-up0-ws0
conv_igemm_kernel<bf16_t, 32, 32, FAST 1> + conv_splitk_reduce_kernel
    (1, 'fwd', 0, 32, 32, 0, 1, 0, 1, 0, 1)
    <- bf16-1x4x4-128+0to64-k3s2-up0-ws1
conv_igemm_kernel<bf16_t, 32, 32, SMALLC>
    (1, 'fwd', 0, 32, 32, 0, 1, 1, 0, 0, 0)
    <- bf16-16x12x128-96+0to64-k1s2-up0-ws0, bf16-12x8x64-96+0to64-k3s2-up0-ws0, bf16-3x56x72-96+0to64-k3s2-up0-ws0
conv_igemm_kernel<bf16_t, 32, 32, FAST 2 (up-folded)>
    (1, 'fwd', 0, 32, 32, 3, 4, 0, 0, 0, 0)
    <- bf16-1x4x4-64+64to256-k3s1-up2-ws0
conv_igemm_kernel<bf16_t, 32, 32, FAST 2 (up-folded)> + conv_splitk_reduce_kernel
    (1, 'fwd', 0, 32, 32, 3, 4, 0, 0, 0, 1)
    <- bf16-3x12x20-128+64to128-k3s1-up2-ws1
conv_igemm_kernel<bf16_t, 64, 32, FAST 1>
    (1, 'fwd', 0, 64, 32, 0, 1, 0, 1, 0, 0)
    <- bf16-16x12x128-64+0to96-k1s2-up0-ws0
conv_igemm_kernel<bf16_t, 64, 32, FAST 2 (up-folded)>
    (1, 'fwd', 0, 64, 32, 3, 4, 0, 0, 0, 0)
    <- bf16-12x8x64-64+64to96-k3s1-up2-ws0
conv_igemm_kernel<bf16_t, 64, 64, FAST 1>
    (1, 'fwd', 0, 64, 64, 0, 1, 0, 1, 0, 0)
    <- bf16-12x64x64-64+0to96-k1s2-up0-ws0
conv_igemm_kernel<bf16_t, 64, 64, FAST 2 (up-folded)>
    (1, 'fwd', 0, 64, 64, 3, 4, 0, 0, 0, 0)
    <- bf16-3x56x72-64+64to96-k3s1-up2-ws0
conv_pres_kernel<128, 32, 4, 1, 1, 1>
    (1, 'fwd', 10, 0, 0, 0, 1, 0, 0, 0, 0)
    <- bf16-16x16x128-128+0to32-k3s1-up0-ws0
conv_pres_kernel<256, 16, 2, 1, 2, 1>
    (1, 'fwd', 11, 0, 0, 0, 1, 0, 0, 0, 0)
    <- bf16-16x32x32-256+0to32-k3s1-up0-ws0
conv_pres_kernel<512, 8, 1, 1, 4, 2>
    (1, 'fwd', 12, 0, 0, 0, 1, 0, 0, 0, 0)
    <- bf16-8x32x32-512+0to32-k3s1-up0-ws0
conv_patch_kernel<bf16_t, 16, 16>
    (1, 'fwd', 3, 0, 0, 0, 1, 0, 0, 0, 0)
    <- bf16-3x128x128-16+0to16-k3s1-up0-ws0
conv_patch_kernel<bf16_t, 32, 32>
    (1, 'fwd', 4, 0, 0, 0, 1, 0, 0, 0, 0)
    <- bf16-3x4x64-32+0to24-k3s1-up0-ws0
conv_patch_kernel<bf16_t, 32, 16, UP>
    (1, 'fwd', 5, 0, 0, 0, 1, 0, 0, 0, 0)
    <- bf16-2x8x64-32+0to16-k3s1-up1-ws0, bf16-1x12x128-32+0to8-k3s1-up2-ws0, bf16-1x4x64-32+0to16-k3s1-up2-ws0
conv_stem_bf16_kernel
    (1, 'fwd', 8, 0, 0, 0, 1, 0, 0, 0, 0)
    <- bf16-1x48x128-8+0to64-k7s2-up0-ws0
conv_pres_kernel<64, 64, 2, 2, 1, 2>
    (1, 'fwd', 9, 0, 0, 0, 1, 0, 0, 0, 0)
    <- bf16-12x64x64-64+0to64-k3s1-up0-ws0
conv_wgrad_kernel<bf16_t, 32, 32, 1, 1, 4> + wgrad_reduce_batch_kernel
    (1, 'wgrad', 0, 0, 0, 32)
    <- bf16-1x12x128-48+0to32-k3s1-up0-ws0, bf16-3x56x72-512+0to3-k3s1-up2-ws0
conv_wgrad_kernel<bf16_t, 64, 64, 2, 2, 1, bf16 MFMA> + wgrad_reduce_batch_kernel
    (1, 'wgrad', 0, 0, 0, 64)
    <- bf16-1x4x4-64+0to64-k1s2-up0-ws0, bf16-1x4x4-128+0to64-k3s2-up0-ws1, bf16-16x12x128-64+0to96-k1s2-up0-ws0, bf16-16x12x128-96+0to64-k1s2-up0-ws0, bf16-12x64x64-64+0to96-k1s2-up0-ws0, bf16-12x8x64-96+0to64-k3s2-up0-ws0, bf16-3x56x72-96+0to64-k3s2-up0-ws0
conv_wgrad_patch_kernel<bf16_t, 32, 8, 7, 2, 16> + wgrad_reduce_batch_kernel
    (1, 'wgrad', 0, 0, 5, 0)
    <- bf16-2x64x96-8+0to64-k7s2-up0-ws0
conv_wgrad_patch_kernel<bf16_t, 32, 4, 7, 2, 16, 3> + wgrad_reduce_batch_kernel
    (1, 'wgrad', 0, 0, 6, 0)
    <- bf16-5x256x256-8+0to32-k7s2-up0-ws0, bf16-1x48x128-8+0to64-k7s2-up0-ws0
conv_wgrad_patch_bf16_kernel + wgrad_reduce_batch_kernel
    (1, 'wgrad', 0, 0, 7, 0)
    <- bf16-12x64x64-64+0to64-k3s1-up0-ws0, bf16-3x128x128-16+0to16-k3s1-up0-ws0, bf16-2x8x64-32+0to16-k3s1-up1-ws0, bf16-1x12x128-32+0to8-k3s1-up2-ws0, bf16-1x12x128-16+0to3-k3s1-up0-ws0, bf16-3x12x20-128+64to128-k3s1-up2-ws1, bf16-3x4x64-32+0to24-k3s1-up0-ws0, bf16-1x4x4-64+64to32-k3s1-up2-ws0, bf16-1x4x4-64+64to32-k3s1-up2-ws1, bf16-1x4x64-32+0to16-k3s1-up2-ws0, bf16-3x56x72-256+0to3-k3s1-up2-ws0
conv_wgrad_kernel<bf16_t, 64, 64, 2, 2, 1, bf16 MFMA, CLS> + wgrad_reduce_batch_kernel
    (1, 'wgrad', 1, 1, 0, 64)
    <- bf16-1x4x4-64+64to256-k3s1-up2-ws0
conv_wgrad_kernel<bf16_t, 64, 64, 2, 2, 1, bf16 MFMA> + wgrad_reduce_batch_kernel
    (1, 'wgrad', 2, 0, 0, 64)
    <- bf16-1x4x4-64+64to256-k3s1-up2-ws0
conv_igemm_kernel<float, 128, 64, FAST 1, X3>
    (2, 'dgrad', 0, 128, 64, 0, 1, 0, 1, 0, 0)
    <- f32x3-16x16x128-8+64to32-k3s1-up0-ws0
conv_igemm_kernel<float, 128, 64, FAST 1, X3> par 1
    (2, 'dgrad', 0, 128, 64, 1, 4, 0, 1, 0, 0)
    <- f32x3-16x16x128-96+0to32-k3s2-up0-ws0
conv_igemm_kernel<float, 256, 16, SMALLC, X3>
    (2, 'dgrad', 0, 256, 16, 0, 1, 1, 0, 0, 0)
    <- f32x3-1x4x4-8+0to8-k1s2-up0-ws0, f32x3-1x4x4-16+0to3-k3s1-up0-ws0
conv_igemm_kernel<float, 256, 16, FAST 1, X3> par 2
    (2, 'dgrad', 0, 256, 16, 2, 1, 0, 1, 0, 0)
    <- f32x3-8x128x128-8+0to96-k1s2-up0-ws0
conv_igemm_kernel<float, 256, 32, FAST 1, X3>
    (2, 'dgrad', 0, 256, 32, 0, 1, 0, 1, 0, 0)
    <- f32x3-1x4x4-32+32to32-k3s1-up2-ws0, f32x3-1x4x4-32+0to32-k3s1-up0-ws0
conv_igemm_kernel<float, 256, 32, FAST 1, X3> + conv_splitk_reduce_kernel
    (2, 'dgrad', 0, 256, 32, 0, 1, 0, 1, 0, 1)
    <- f32x3-1x4x4-32+32to64-k3s1-up2-ws1
conv_igemm_kernel<float, 256, 32, FAST 1, X3> par 2
    (2, 'dgrad', 0, 256, 32, 2, 1, 0, 1, 0, 0)
    <- f32x3-8x128x128-32+0to96-k1s2-up0-ws0
conv_igemm_kernel<float, 64, 64, FAST 1, X3>
    (2, 'dgrad', 0, 64, 64, 0, 1, 0, 1, 0, 0)
    <- f32x3-3x12x20-128+64to128-k3s1-up2-ws0
conv_igemm_kernel<float, 64, 64, FAST 1, X3> + conv_splitk_reduce_kernel
    (2, 'dgrad', 0, 64, 64, 0, 1, 0, 1, 0, 1)
    <- f32x3-1x4x4-32+32to64-k3s1-up0-ws1
conv_igemm_kernel<float, 64, 64, FAST 1, X3> par 1
    (2, 'dgrad', 0, 64, 64, 1, 4, 0, 1, 0, 0)
    <- f32x3-1x4x4-64+0to32-k3s2-up0-ws0
conv_igemm_kernel<float, 64, 64, FAST 1, X3> par 2
    (2, 'dgrad', 0, 64, 64, 2, 1, 0, 1, 0, 0)
    <- f32x3-1x4x4-64+0to64-k1s2-up0-ws0, f32x3-1x4x4-512+0to64-k1s2-up0-ws1
conv_igemm_kernel<float, 128, 64, FAST 1, X3>
    (2, 'dgrad_lo', 0, 128, 64, 0, 1, 0, 1, 0, 0)
    <- f32x3-8x128x128-96+0to32-k3s1-up2-ws0
conv_igemm_kernel<float, 256, 32, FAST 1, X3>
    (2, 'dgrad_lo', 0, 256, 32, 0, 1, 0, 1, 0, 0)
    <- f32x3-1x4x4-32+32to32-k3s1-up2-ws0
conv_igemm_kernel<float, 256, 32, FAST 1, X3> + conv_splitk_reduce_kernel
    (2, 'dgrad_lo', 0, 256, 32, 0, 1, 0, 1, 0, 1)
    <- f32x3-1x4x4-32+32to64-k3s1-up2-ws1
conv_igemm_kernel<float, 256, 32, SMALLC, X3>
    (2, 'dgrad_lo', 0, 256, 32, 0, 1, 1, 0, 0, 0)
    <- f32x3-1x4x4-32+0to8-k3s1-up2-ws0
conv_igemm_kernel<float, 64, 64, FAST 1, X3>
    (2, 'dgrad_lo', 0, 64, 64, 0, 1, 0, 1, 0, 0)
    <- f32x3-3x12x20-128+64to128-k3s1-up2-ws0
conv_igemm_kernel<float, 64, 64, FAST 1, X3> + conv_splitk_reduce_kernel
    (2, 'dgrad_lo', 0, 64, 64, 0, 1, 0, 1, 0, 1)
    <- f32x3-1x4x4-64+0to32-k3s1-up2-ws1
conv_igemm_kernel<float, 128, 64, FAST 1, X3>
    (2, 'fwd', 0, 128, 64, 0, 1, 0, 1, 0, 0)
    <- f32x3-8x128x128-32+0to96-k1s2-up0-ws0
conv_igemm_kernel<float, 128, 64, SMALLC, X3>
    (2, 'fwd', 0, 128, 64, 0, 1, 1, 0, 0, 0)
    <- f32x3-8x128x128-8+0to96-k1s2-up0-ws0
conv_igemm_kernel<float, 128, 64, FAST 2 (up-folded), X3>
    (2, 'fwd', 0, 128, 64, 3, 4, 0, 0, 0, 0)
    <- f32x3-16x16x128-32+32to96-k3s1-up2-ws0
conv_igemm_kernel<float, 256, 16, SMALLC, X3>
    (2, 'fwd', 0, 256, 16, 0, 1, 1, 0, 0, 0)
    <- f32x3-1x4x4-8+0to8-k1s2-up0-ws0
conv_igemm_kernel<float, 256, 16, FAST 2 (up-folded), X3>
    (2, 'fwd', 0, 256, 16, 3, 4, 0, 1, 0, 0)
    <- f32x3-1x4x4-32+0to8-k3s1-up2-ws0
conv_igemm_kernel<float, 256, 32, FAST 1, X3>
    (2, 'fwd', 0, 256, 32, 0, 1, 0, 1, 0, 0)
    <- f32x3-1x4x4-64+0to32-k3s2-up0-ws0, f32x3-1x4x4-32+0to32-k3s1-up0-ws0, f32x3-16x16x128-96+0to32-k3s2-up0-ws0
conv_igemm_kernel<float, 256, 32, FAST 2 (up-folded), X3>
    (2, 'fwd', 0, 256, 32, 3, 4, 0, 0, 0, 0)
    <- f32x3-1x4x4-32+32to32-k3s1-up2-ws0
conv_igemm_kernel<float, 256, 32, FAST 2 (up-folded), X3>
    (2, 'fwd', 0, 256, 32, 3, 4, 0, 1, 0, 0)
    <- f32x3-1x4x4-64+0to32-k3s1-up2-ws1
conv_igemm_kernel<float, 64, 64, FAST 0, X3> + conv_splitk_reduce_kernel
    (2, 'fwd', 0, 64, 64, 0, 1, 0, 0, 0, 1)
    <- f32x3-1x4x4-32+32to64-k3s1-up0-ws1
conv_igemm_kernel<float, 64, 64, FAST 1, X3>
    (2, 'fwd', 0, 64, 64, 0, 1, 0, 1, 0, 0)
    <- f32x3-1x4x4-64+0to64-k1s2-up0-ws0
conv_igemm_kernel<float, 64, 64, FAST 1, X3> + conv_splitk_reduce_kernel
    (2, 'fwd', 0, 64, 64, 0, 1, 0, 1, 0, 1)
    <- f32x3-1x4x4-512+0to64-k1s2-up0-ws1
conv_igemm_kernel<float, 64, 64, SMALLC, X3>
    (2, 'fwd', 0, 64, 64, 0, 1, 1, 0, 0, 0)
    <- f32x3-2x32x32-4+0to64-k7s2-up0-ws0
conv_igemm_kernel<float, 64, 64, FAST 2 (up-folded), X3>
    (2, 'fwd', 0, 64, 64, 3, 4, 0, 0, 0, 0)
    <- f32x3-3x12x20-128+64to128-k3s1-up2-ws0
conv_igemm_kernel<float, 64, 64, FAST 2 (up-folded), X3> + conv_splitk_reduce_kernel
    (2, 'fwd', 0, 64, 64, 3, 4, 0, 0, 0, 1)
    <- f32x3-1x4x4-32+32to64-k3s1-up2-ws1
conv_wgrad_kernel<float, 32, 32, 1, 1, 4> + wgrad_reduce_batch_kernel
    (2, 'wgrad', 0, 0, 0, 32)
    <- f32x3-1x4x4-8+0to8-k1s2-up0-ws0, f32x3-1x4x4-64+0to32-k3s2-up0-ws0, f32x3-8x128x128-8+0to96-k1s2-up0-ws0, f32x3-8x128x128-32+0to96-k1s2-up0-ws0, f32x3-16x16x128-96+0to32-k3s2-up0-ws0
conv_wgrad_kernel<float, 64, 64, 2, 2, 1, bf16 MFMA> + wgrad_reduce_batch_kernel
    (2, 'wgrad', 0, 0, 0, 64)
    <- f32x3-1x4x4-64+0to64-k1s2-up0-ws0, f32x3-1x4x4-512+0to64-k1s2-up0-ws1
conv_wgrad_patch_kernel<float, 16, 16, 3, 1, 16> + wgrad_reduce_batch_kernel
    (2, 'wgrad', 0, 0, 2, 0)
    <- f32x3-1x4x4-16+0to3-k3s1-up0-ws0
conv_wgrad_patch_kernel<float, 32, 32, 3, 1, 16> + wgrad_reduce_batch_kernel
    (2, 'wgrad', 0, 0, 3, 0)
    <- f32x3-1x4x4-32+0to32-k3s1-up0-ws0
conv_wgrad_patch_kernel<float, 32, 4, 7, 2, 16, 3> + wgrad_reduce_batch_kernel
    (2, 'wgrad', 0, 0, 4, 0)
    <- f32x3-2x32x32-4+0to64-k7s2-up0-ws0
conv_wgrad_kernel<float, 64, 64, 2, 2, 1, bf16 MFMA, CLS> + wgrad_reduce_batch_kernel
    (2, 'wgrad', 1, 1, 0, 64)
    <- f32x3-3x12x20-128+64to128-k3s1-up2-ws0
conv_wgrad_patch_cls_kernel<float, 16, 32, 16> + wgrad_reduce_batch_kernel
    (2, 'wgrad', 1, 1, 1, 0)
    <- f32x3-1x4x4-32+0to8-k3s1-up2-ws0
conv_wgrad_patch_cls_kernel<float, 32, 32, 16> + wgrad_reduce_batch_kernel
    (2, 'wgrad', 1, 1, 3, 0)
    <- f32x3-1x4x4-32+32to32-k3s1-up2-ws0, f32x3-1x4x4-64+0to32-k3s1-up2-ws1
conv_wgrad_kernel<float, 64, 64, 2, 2, 1, bf16 MFMA> + wgrad_reduce_batch_kernel
    (2, 'wgrad', 2, 0, 0, 64)
    <- f32x3-3x12x20-128+64to128-k3s1-up2-ws0
conv_wgrad_patch_kernel<float, 32, 32, 3, 1, 16> + wgrad_reduce_batch_kernel
    (2, 'wgrad', 2, 0, 3, 0)
    <- f32x3-1x4x4-32+32to32-k3s1-up2-ws0

Reachable only through the whole network (run-time paths of the instantiations above, no instantiation of their own):
the eval-fused epilogue of d3f_conv_forward's kernels (CONV_EVAL_FUSED; conv_winograd_kernel's own is run here, through
d3f_conv_winograd_forward's scale / shift / residual arguments) and the head's bias + NCHW epilogue
(CONV_HEAD_NCHW), BatchNorm partial sums riding in a data-gradient epilogue (ConvParams::bn_partial), and two networks
in one launch (grid.z = nets): tests/test_gpu_unet.py, test_gpu_bf16.py, test_gpu_parity_layers.py, test_gpu_pair.py.
"""
import ctypes as C

import pytest
import torch

import conv_cases as cc
from conv_cases import BF16, CASES
from denoising_diffusion_deep_fake_amd import _lib
from util import SENTINEL, Guarded

pytestmark = pytest.mark.gpu

GUARD_ROWS = 64
GUARD_BYTES = 4096      # byte buffers (packed weights, workspaces): 64 rows of 64 bytes
NAN_BYTE, BAND_BYTE = 0xFF, 0xA5   # 0xFFFF / 0xFFFFFFFF are NaN in bf16 / fp32
SPARE_STAT_ROWS = 4     # NaN rows behind the last statistics row the plan names
NAN = float("nan")
RATIOS = {}             # (direction, dtype name) -> worst |got - ref| / bound seen in this run (information only)


def note(direction, c, ratio):
    key = (direction, cc.DTYPE_NAMES[c.dtype])
    RATIOS[key] = max(RATIOS.get(key, 0.0), ratio)
    print(f"error/bound {direction:10s} {cc.case_id(c)}: {ratio:.3f}")


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def ptr(g):
    if g is None:
        return None
    return C.c_void_p((g.t if isinstance(g, Guarded) else g).data_ptr())


def byte_buffer(n):
    return Guarded(max(int(n), 16), GUARD_BYTES, torch.uint8, fill=NAN_BYTE, band=BAND_BYTE)


def bits(t):
    return t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32 if t.dtype == torch.float32 else t.dtype).clone()


def run_twice(call, outputs, poison):
    """call() from the same poisoned state twice: the outputs must agree bit for bit; returns nothing (the second
    run's results stay in the buffers)"""
    poison()
    call()
    torch.cuda.synchronize()
    first = [bits(o.buf) for o in outputs]
    poison()
    call()
    torch.cuda.synchronize()
    for k, (a, o) in enumerate(zip(first, outputs)):
        assert torch.equal(a, bits(o.buf)), f"output {k} differs between two runs"
        assert o.intact(), f"guard band of output {k} overwritten"


def check(direction, c, got_nchw, ref, bound, gate):
    bad, ratio = cc.violations(got_nchw, ref, bound)
    note(direction, c, ratio)
    assert bad == 0, (direction, cc.case_id(c), bad, ratio)
    e = cc.rel_l2(got_nchw, ref)
    assert e < gate, (direction, cc.case_id(c), "rel-L2", e)


def same(direction, c, got, want):
    """the exact pass: equality with the float64 result (after the route's storage roundings), no tolerance"""
    got = got.double()
    diff = got != want   # (NaN differs from everything)
    n = int(diff.sum())
    first = tuple(diff.nonzero()[0].tolist()) if n else None
    assert got.shape == want.shape and torch.equal(got, want), \
        (direction, cc.case_id(c), f"{n} of {want.numel()} elements differ, first at {first}",
         None if first is None else (float(got[first]), float(want[first])))


def gate_of(c):
    return cc.REL_L2_BF16 if c.dtype == BF16 else cc.REL_L2_F32


def device_input(x64, cpad, dtype, gen):
    """NCHW float64 -> NHWC storage tensor on the device; pad channels hold finite garbage"""
    t = cc.to_nhwc(x64, cpad)
    if cpad > x64.shape[1]:
        t[..., x64.shape[1]:] = torch.randn(t[..., x64.shape[1]:].shape, generator=gen, dtype=torch.float64) * 3.0
    return t.to(cc.tdt(dtype)).cuda().contiguous()


class Run:
    def __init__(self, c, exact=False):
        self.c, self.L, self.exact = c, _lib.lib(), exact
        self.d = cc.desc_of(c)
        self.plan = cc.plan_of(c)
        assert cc.case_forms(c, self.plan) == c.forms, "the planner moved this case: tests/test_cpu_conv_forms.py"
        self.data = cc.make_exact_data(c) if exact else cc.make_data(c)
        self.ref = cc.reference(c, self.data, mags=not exact)
        if exact:   # what makes equality the right demand (tests/test_cpu_conv_forms.py asserts the same without a GPU)
            cond = cc.exact_conditions(c, self.plan, self.data, self.ref.get("y"))
            assert all(v < 2 ** 24 for v in cond.values()), cond
        self.gen = torch.Generator().manual_seed(99)
        x0, x1, w, dy = self.data
        self.tt = cc.tdt(c.dtype)
        self.s0 = device_input(x0, c.C0, c.dtype, self.gen)
        self.s1 = cc.to_nhwc(x1).to(self.tt).cuda() if x1 is not None else None
        self.w = w.float().cuda().contiguous()
        coutd = (c.Cout + cc.ve(c.dtype) - 1) // cc.ve(c.dtype) * cc.ve(c.dtype)
        self.dy = cc.to_nhwc(dy, coutd).to(self.tt).cuda()  # pad channels zero
        self.ho, self.wo = cc.out_hw(c)

    def ok(self, rc):
        assert rc == 0, self.L.d3f_last_error().decode()

    def stored(self, x64):
        return cc.stored(x64, self.c.dtype)

    def base(self, *shape):
        """an existing gradient to accumulate into: storage-type N(0, 1), or {-1, 0, 1} in the exact pass"""
        if self.exact:
            return torch.randint(-1, 2, shape, generator=self.gen).double()
        return self.stored(torch.randn(*shape, generator=self.gen, dtype=torch.float64))

    # ---- packed weights: NaN bytes before the pack ----
    def pack(self):
        c, L, d = self.c, self.L, self.d
        # (an up-folded layer's pack kernel writes the forward matrices whichever layout is asked for)
        self.wf = byte_buffer(L.d3f_conv_packed_bytes(c.dtype, C.byref(d), 0)) if "fwd" in c.dirs or self.plan.upfold else None
        self.wd = byte_buffer(L.d3f_conv_packed_bytes(c.dtype, C.byref(d), 1)) if "dgrad" in c.dirs else None
        outs = [b for b in (self.wf, self.wd) if b is not None]
        if not outs:
            return
        run_twice(lambda: self.ok(L.d3f_conv_pack_weights(c.dtype, C.byref(d), ptr(self.w), ptr(self.wf), ptr(self.wd), stream())),
                  outs, lambda: [b.t.fill_(NAN_BYTE) for b in outs])

    def forward(self):
        c, L, d, plan = self.c, self.L, self.d, self.plan
        tiles = C.c_int()
        nst = L.d3f_conv_stats_floats(c.dtype, C.byref(d), c.ws, C.byref(tiles))
        rows = tiles.value
        assert rows == plan.fwd.stat_rows and nst % (2 * rows) == 0
        cpad = nst // (2 * rows)
        y = Guarded(c.B * self.ho * self.wo * c.Cout, GUARD_ROWS * c.Cout, self.tt)
        stats = Guarded((rows + SPARE_STAT_ROWS) * cpad * 2, GUARD_ROWS * cpad * 2, torch.float32, fill=NAN, band=NAN)
        ws = byte_buffer(L.d3f_conv_workspace_bytes(c.dtype, C.byref(d), 0)) if c.ws else None
        outs = [y, stats] + ([ws] if ws else [])

        def poison():
            y.t.fill_(SENTINEL)
            stats.t.fill_(NAN)
            if ws:
                ws.t.fill_(NAN_BYTE)
        run_twice(lambda: self.ok(L.d3f_conv_forward(c.dtype, C.byref(d), ptr(self.s0), ptr(self.s1), ptr(self.wf), ptr(y),
                                                     ptr(stats), ptr(ws), stream())), outs, poison)
        assert self.wf.intact()
        got = cc.to_nchw(y.t.cpu().view(c.B, self.ho, self.wo, c.Cout))
        ref_y = self.ref["y"]
        st = stats.t.cpu().view(rows + SPARE_STAT_ROWS, cpad, 2)
        assert bool(torch.isfinite(st[:rows, :c.Cout]).all()), "statistics rows not written"
        assert bool(torch.isnan(st[rows:]).all()), "statistics written behind the last row the plan names"
        sums = st[:rows, :c.Cout].double().sum(0)
        if self.exact:
            same("fwd", c, got, self.stored(ref_y))
            same("stats sum", c, sums[:, 0], ref_y.sum((0, 2, 3)))
            same("stats sumsq", c, sums[:, 1], (ref_y * ref_y).sum((0, 2, 3)))
            return
        mag = self.ref["y_mag"]
        check("fwd", c, got, ref_y, cc.fwd_bound(c, plan, ref_y, mag), gate_of(c))
        s1, s2, b1, b2 = cc.stats_reference(c, plan, ref_y, mag)
        for name, got_s, ref_s, bnd in (("sum", sums[:, 0], s1, b1), ("sumsq", sums[:, 1], s2, b2)):
            bad, ratio = cc.violations(got_s, ref_s, bnd)
            note("stats " + name, c, ratio)
            assert bad == 0, ("statistics", name, cc.case_id(c), bad, ratio)

    def backward_data(self):
        c, L, d, plan = self.c, self.L, self.d, self.plan
        route = cc.dgrad_route(c, plan)
        low = route in ("folded", "summed")
        h0, w0 = (c.H // 2, c.W // 2) if low else (c.H, c.W)
        dx0 = Guarded(c.B * h0 * w0 * c.C0, GUARD_ROWS * c.C0, self.tt)
        dx1 = Guarded(c.B * c.H * c.W * c.C1, GUARD_ROWS * c.C1, self.tt) if c.C1 else None
        ws = byte_buffer(L.d3f_conv_workspace_bytes(c.dtype, C.byref(d), 1)) if c.ws else None
        outs = [dx0] + ([dx1] if dx1 else []) + ([ws] if ws else [])
        ref_dx, mag = self.ref["dx"], self.ref.get("dx_mag")
        r0, m0 = ref_dx[:, :c.C0], None if mag is None else mag[:, :c.C0]
        r1, m1 = ref_dx[:, c.C0:], None if mag is None else mag[:, c.C0:]
        base0 = self.base(c.B, c.C0, h0, w0)
        base1 = self.base(c.B, c.C1, c.H, c.W) if c.C1 else None

        def call(acc):
            return lambda: self.ok(L.d3f_conv_backward_data(c.dtype, C.byref(d), ptr(self.dy), ptr(self.wd), ptr(dx0), ptr(dx1),
                                                            acc, acc, ptr(ws), stream()))

        def poison(acc):
            def f():
                if acc:
                    dx0.t.copy_(cc.to_nhwc(base0).to(self.tt).reshape(-1))
                    if dx1:
                        dx1.t.copy_(cc.to_nhwc(base1).to(self.tt).reshape(-1))
                else:
                    dx0.t.fill_(SENTINEL)
                    if dx1:
                        dx1.t.fill_(SENTINEL)
                if ws:
                    ws.t.fill_(NAN_BYTE)
            return f

        def read0():
            return cc.to_nchw(dx0.t.cpu().view(c.B, h0, w0, c.C0))

        def read1():
            return cc.to_nchw(dx1.t.cpu().view(c.B, c.H, c.W, c.C1))

        run_twice(call(0), outs, poison(0))
        assert self.wd.intact()
        want0 = cc.sum2x2(r0) if low else r0
        if self.exact:
            same("dgrad " + route, c, read0(), self.stored(want0))
            if dx1:
                same("dgrad skip", c, read1(), self.stored(r1))
        else:
            err0 = cc.dgrad_low_err(c, plan, r0, m0) if low else cc.dgrad_full_err(c, m0)
            check("dgrad " + route, c, read0(), want0, cc.store_rounding(c.dtype, want0, err0), gate_of(c))
            if dx1:
                check("dgrad skip", c, read1(), r1, cc.dgrad_full_bound(c, r1, m1), gate_of(c))
        if route == "fullres":  # the caller reduces the full-resolution gradient itself
            lowg = Guarded(c.B * (c.H // 2) * (c.W // 2) * c.C0, GUARD_ROWS * c.C0, self.tt)
            run_twice(lambda: self.ok(L.d3f_upsample2x_backward(c.dtype, ptr(dx0), ptr(lowg), c.B, c.H // 2, c.W // 2, c.C0, stream())),
                      [lowg], lambda: lowg.t.fill_(SENTINEL))
            assert dx0.intact()
            got = cc.to_nchw(lowg.t.cpu().view(c.B, c.H // 2, c.W // 2, c.C0))
            if self.exact:   # two storage roundings: the full-resolution gradient, then its 2 x 2 sums
                same("dgrad 2x2", c, got, self.stored(cc.sum2x2(self.stored(r0))))
            else:
                check("dgrad 2x2", c, got, cc.sum2x2(r0), cc.dgrad_low_bound(c, plan, r0, m0), gate_of(c))
        # accumulate into an existing gradient
        run_twice(call(1), outs, poison(1))
        if self.exact:
            same("dgrad acc", c, read0(), self.stored(base0 + want0))
            if dx1:
                same("dgrad acc skip", c, read1(), self.stored(base1 + r1))
            return
        total, bound = cc.acc_bound(c, base0, want0, err0)
        bad, ratio = cc.violations(read0(), total, bound)
        note("dgrad acc", c, ratio)
        assert bad == 0, ("acc0", cc.case_id(c), bad, ratio)
        if dx1:
            total, bound = cc.acc_bound(c, base1, r1, cc.dgrad_full_err(c, m1))
            bad, ratio = cc.violations(read1(), total, bound)
            note("dgrad acc", c, ratio)
            assert bad == 0, ("acc1", cc.case_id(c), bad, ratio)

    def backward_weight(self):
        c, L, d, plan = self.c, self.L, self.d, self.plan
        per_filter = c.cin_real * c.k * c.k
        dw = Guarded(c.Cout * per_filter, GUARD_ROWS * per_filter, torch.float32)
        ws = byte_buffer(L.d3f_conv_backward_weight_workspace_bytes(c.dtype, C.byref(d)))

        def poison():
            dw.t.fill_(SENTINEL)
            ws.t.fill_(NAN_BYTE)
        run_twice(lambda: self.ok(L.d3f_conv_backward_weight(c.dtype, C.byref(d), ptr(self.dy), ptr(self.s0), ptr(self.s1), ptr(ws),
                                                             ptr(dw), stream())), [dw, ws], poison)
        got = dw.t.cpu().view(c.Cout, c.cin_real, c.k, c.k)
        if self.exact:
            same("wgrad", c, got, self.ref["dw"])
            return
        check("wgrad", c, got, self.ref["dw"], cc.wgrad_bound(c, plan, self.ref["dw_mag"]), cc.REL_L2_WGRAD)

    def winograd(self):
        """conv_winograd_kernel through its own entry: guards, poison, repeat; the aggregate gates of
        tests/test_gpu_ops.py, and beside them the per-element bound of conv_cases.py on y, the bounds derived from it on
        both statistics sums, and the four eval-epilogue variants under theirs"""
        c, L, d = self.c, self.L, self.d
        u = byte_buffer(L.d3f_conv_winograd_filter_bytes(C.byref(d)))
        run_twice(lambda: self.ok(L.d3f_conv_winograd_pack(C.byref(d), ptr(self.w), ptr(u), stream())), [u],
                  lambda: u.t.fill_(NAN_BYTE))
        tiles = C.c_int()
        nst = L.d3f_conv_winograd_stats_floats(C.byref(d), C.byref(tiles))
        rows = tiles.value
        assert rows == self.plan.wino_rows == c.B * (c.H // 16) * (c.W // 16)
        cpad = nst // (2 * rows)
        y = Guarded(c.B * c.H * c.W * c.Cout, GUARD_ROWS * c.Cout, self.tt)
        stats = Guarded((rows + SPARE_STAT_ROWS) * cpad * 2, GUARD_ROWS * cpad * 2, torch.float32, fill=NAN, band=NAN)

        def poison():
            y.t.fill_(SENTINEL)
            stats.t.fill_(NAN)
        run_twice(lambda: self.ok(L.d3f_conv_winograd_forward(C.byref(d), ptr(self.s0), ptr(u), ptr(y), ptr(stats), None, None,
                                                              None, 0, stream())), [y, stats], poison)
        assert u.intact()
        ref_y = self.ref["y"]
        got = cc.to_nchw(y.t.cpu().view(c.B, c.H, c.W, c.Cout))
        assert cc.rel_l2(got, ref_y) < cc.REL_L2_F32
        st = stats.t.cpu().view(rows + SPARE_STAT_ROWS, cpad, 2)
        assert bool(torch.isfinite(st[:rows, :c.Cout]).all()) and bool(torch.isnan(st[rows:]).all())
        sums = st[:rows, :c.Cout].double().sum(0)
        s1, s2 = ref_y.sum((0, 2, 3)), (ref_y * ref_y).sum((0, 2, 3))
        assert float(((sums[:, 1] - s2).abs().max() / s2.abs().max())) < 1e-5
        assert float((sums[:, 0] - s1).abs().max()) < 1e-3 * (1 + float(s2.sqrt().max()))
        # every element and both sums under the Winograd bound (exact pass: equal)
        x0, w = self.data[0], self.data[2]
        if self.exact:
            same("wino", c, got, ref_y)
            same("wino stats sum", c, sums[:, 0], s1)
            same("wino stats sumsq", c, sums[:, 1], s2)
            acc = None
        else:
            acc = cc.wino_acc_bound(c, cc.winograd_eval(x0, w, absolute=True))
            check("wino", c, got, ref_y, acc, cc.REL_L2_F32)
            _, _, b1, b2 = cc.stats_reference(c, self.plan, ref_y, None, wino=True, acc=acc)
            for name, got_s, ref_s, bnd in (("sum", sums[:, 0], s1, b1), ("sumsq", sums[:, 1], s2, b2)):
                bad, ratio = cc.violations(got_s, ref_s, bnd)
                note("wino stats " + name, c, ratio)
                assert bad == 0, ("winograd statistics", name, cc.case_id(c), bad, ratio)
        # the eval epilogue of the same kernel: relu?(o * scale + shift + residual?)
        if self.exact:
            scale = torch.tensor([-2.0, -1.0, 1.0, 2.0])[torch.randint(0, 4, (c.Cout,), generator=self.gen)]
            shift = torch.randint(-1, 2, (c.Cout,), generator=self.gen).float()
            res64 = torch.randint(-1, 2, ref_y.shape, generator=self.gen).double()
        else:
            scale = torch.rand(c.Cout, generator=self.gen) + 0.5
            scale[::3] = -scale[::3]
            shift = torch.randn(c.Cout, generator=self.gen) * 0.3
            res64 = torch.randn(ref_y.shape, generator=self.gen).double()
        sc_d, sf_d = scale.cuda(), shift.cuda()
        res = Guarded(res64.numel(), GUARD_ROWS * c.Cout, self.tt)
        res_nhwc = cc.to_nhwc(res64).float().reshape(-1)
        res.t.copy_(res_nhwc)
        for with_res in (False, True):
            for relu in (0, 1):
                run_twice(lambda: self.ok(L.d3f_conv_winograd_forward(C.byref(d), ptr(self.s0), ptr(u), ptr(y), None, ptr(sc_d),
                                                                      ptr(sf_d), ptr(res) if with_res else None, relu, stream())),
                          [y], lambda: y.t.fill_(SENTINEL))
                assert u.intact() and res.intact() and torch.equal(res.t.cpu(), res_nhwc), "the epilogue wrote into an input"
                out = cc.to_nchw(y.t.cpu().view(c.B, c.H, c.W, c.Cout))
                name = "wino eval" + ("+res" if with_res else "") + ("+relu" if relu else "")
                want, bound = cc.wino_eval_reference(ref_y, acc if acc is not None else torch.zeros_like(ref_y), scale, shift,
                                                     res64 if with_res else None, bool(relu))
                if self.exact:
                    same(name, c, out, want)
                else:
                    check(name, c, out, want, bound, cc.REL_L2_F32)
                assert not relu or bool((out >= 0).all())


def run_case(case, exact):
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    r = Run(case, exact)
    if case.entry == "winograd":
        r.winograd()
        return
    r.pack()
    if "fwd" in case.dirs:
        r.forward()
    if "dgrad" in case.dirs:
        r.backward_data()
    if "wgrad" in case.dirs:
        r.backward_weight()


@pytest.mark.parametrize("case", CASES, ids=cc.case_id)
def test_conv_case(case):
    run_case(case, exact=False)


@pytest.mark.parametrize("case", CASES, ids=cc.case_id)
def test_conv_case_exact(case):
    """the same case on operands in {-1, 0, 1}: every result equals float64 (conv_cases.py, "Exact operands")"""
    run_case(case, exact=True)


def test_report_worst_ratios():
    """information only: the worst error / bound per direction and dtype seen by the cases above"""
    for key in sorted(RATIOS):
        print(f"worst error/bound {key[0]:12s} {key[1]:6s} {RATIOS[key]:.3f}")
