"""The convolution operator cases, their float64 reference and their derived per-element bounds -- shared by
tests/test_cpu_conv_forms.py (host only) and tests/test_gpu_conv_forms.py.  Nothing here touches the GPU.

Case table.  A case is (dtype, B, H, W, C0, C1, Cout, k, stride, pad, up, cin_real, with_workspace) -- the d3f_conv_desc
fields in the order the older operator tests use, `up` being d3f_conv_desc::upsample0 (0, 1, or 2 = the 2x2-summed data
gradient where a launch offers it) -- together with the directions it runs, the kernel forms d3f_conv_layer_plan must
report for them, and what it is there for.  A FORM is the tuple of the kernel-selecting plan fields:

    forward / data gradient   (dtype, launch, patch, tile_bm, tile_bn, par, nz, small_c, fast_addr, sum2, splitk > 1)
                              launch: "fwd", "dgrad", or "dgrad_lo" (the up-folded layer's low-resolution source)
    Winograd forward          (dtype, "fwd", "wino")
    weight gradient, per part (dtype, "wgrad", part, cls, patch variant, tile)

Counts (tiles_m, tiles_n, splitk's value, splits, chunks_per_split, stat_rows) are not part of a form.

Float64 reference.  The operands are the values as STORED (rounded to bf16 first in bf16 storage, so the fp32 master
weights handed to the pack routine are exact in bf16 too); forward, both data gradients (for an up-sampled source also
the gradient at the source's own low resolution), weight gradient and the per-channel sums of y and y * y come from
torch's float64 convolutions on the CPU.

Per-element bound.  fp32 accumulation of n products in any order obeys |fl(sum) - sum| <= n * 2^-24 * sum |a_i| |b_i|
(every term passes through at most n roundings; the partial sums of waves, k-groups, split-K slabs, weight-gradient
slabs and the four parity classes are nodes of that same tree, so they cost no rounding of their own as long as no
chain is longer than n).  The magnitude term is the same contraction on the absolute values, in float64.

    forward          n = k * k * Cin
    data gradient    n = k * k * CoutD, times 4 where 2 x 2 blocks are summed into the low-resolution gradient
    weight gradient  n = B * Ho * Wo
    bf16 storage     one round-to-nearest-even of the fp32 result: + 2^-8 * (|ref| + accumulation term).  bf16 has 8
                     significand bits, so its unit roundoff is 2^-8 (torch's fp32 convolution rounded once to bf16 sits
                     at 0.97 of this bound, and at 1.9 of the same bound written with 2^-9).

Roundings a route adds are counted next to the route, at the named constants below (UPFOLD_*, ACC_*, FULLRES_*,
WGRAD_CLASS_ADDS, SLAB_REDUCE_ADDS).

D3F_F32X3.  conv_igemm.hip / conv_wgrad.hip split every fp32 operand exactly into three bf16 terms by TRUNCATION,
x = h + m + l with |m| < 2^-7 |x|, |l| < 2^-15 |x|, and keep six of the nine products, ah bh + ah bm + am bh + am bm +
ah bl + al bh; each is exact in fp32 (8 x 8 significand bits).  Dropped: am bl + al bm + al bl, below
(2 * 2^-22 + 2^-30) |a b| = X3_DROPPED * 2^-24 |a b|.  The six bf16 MFMAs of a k-step contract 16 (32 x 32 x 16) or 32
(16 x 16 x 32) indices each and round the accumulator once per instruction: 6 * ceil(n / 16) roundings instead of n.
The term is therefore (6 * ceil(n / 16) + X3_DROPPED) * 2^-24 * sum |a| |b|, capped at the fp32 bound with n + 4 (the
cap binds below n = 16 only; test_cpu_conv_forms.py asserts it for every case).

Winograd F(2x2, 3x3), fp32 (conv_winograd.hip): Y = A^T [ sum_c (G g G^T) (.) (B^T d B) ] A per 2 x 2 output tile, d the
4 x 4 input tile at stride 2 on the zero-padded input.  Every term of that sum passes through the roundings of four
stages, read off the kernel (the library is compiled with -ffp-contract=off: no fused multiply-add outside the MFMAs):

    input transform    tr_col, then tr_row: one addition or subtraction per stage                     2  WINO_INPUT_ROUNDINGS
    filter transform   winograd_pack_kernel: 0.5f * ((g0 +- g1) + g2) down the columns and again along
                       the rows -- two additions per stage, the halving exact                         4  WINO_FILTER_ROUNDINGS
    contraction        C channels per position through v_mfma_f32_32x32x2f32, the accumulator carried
                       from chunk to chunk: at most one rounding per channel, as for every fp32 MFMA
                       of this table                                                                  C
    output transform   (a + b) + c over the rows of positions, then over the columns                  4  WINO_OUTPUT_ROUNDINGS

A stage's error is relative to that stage on absolute values -- |B^T| |d| |B|, |G| |g| |G^T|, the sum of absolute products,
|A^T| |M| |A| -- so the bound is gamma_n * Ymag with n = C + 10, gamma_n = n * 2^-24 / (1 - n * 2^-24) (the first-order
n * 2^-24 does not cover the products of the stages' errors) and

    Ymag = |A^T| [ sum_c (|G| |g| |G^T|) (.) (|B^T| |d| |B|) ] |A|

the Winograd algorithm itself in float64 on absolute values with the absolute-value matrices (winograd_eval(...,
absolute=True)).  It is NOT the direct convolution's magnitude: the transforms add and subtract what the direct form
never combines (on N(0, 1) data Ymag is about 7 times sum |x| |w|; on inputs with a common offset, where B^T d B cancels,
far more), and a gate built from sum |x| |w| would be violated by a faultless kernel.  The kernel's eval epilogue
v = o * sc + sf (+ res), then ReLU: |sc| * E_o + k * 2^-24 * (|o sc| + |sf| + |res|), k = 2 without a residual (the product,
the addition) and 3 with one; ReLU is 1-Lipschitz and adds nothing.  tests/test_cpu_conv_forms.py restates the whole path
in torch fp32 in the kernel's operation order, holds it to this bound on N(0, 1) inputs and on the same inputs shifted
by + 8, and shows that the same path with V rounded to bf16 violates it.

Exact operands (make_exact_data).  x0, x1, w and dy drawn from {-1, 0, 1}: every product is -1, 0 or 1, every partial sum
of every contraction an integer below 2^24 (exact_conditions, asserted for every case by tests/test_cpu_conv_forms.py),
every pre-summed up-fold weight an integer of at most 4 (exact in bf16 and in the first plane of f32x3), every Winograd
transform a quarter-integer: fp32 arithmetic makes no rounding error in any order, and the only acceptable difference
from float64 is zero.  Every case of the table runs a second time on them and is compared with torch.equal against the
float64 result passed through the route's STORAGE roundings only (bf16 storage rounds integers above 256):

    forward, a data gradient written at its own resolution   stored(ref)
    "fullres" route                                          stored(sum2x2(stored(ref_full)))
    "summed" and "folded" routes                             stored(sum2x2(ref))
    accumulation into an existing gradient                   stored(base + grad), base in {-1, 0, 1}
    weight gradient, all parts, class form and slab reduce   ref
    statistics                                               the float64 total of the partial rows == sum y, sum y^2
    Winograd eval epilogue                                   scale in {-2, -1, 1, 2}, shift and residual in {-1, 0, 1}:
                                                             relu?(ref * scale + shift + res), exact as well

Statistics.  In every storage type they are sums of the fp32 accumulators, `rows` of them per partial row in fp32
(stat_row_pixels), the partial rows added here in float64: bound = the propagated per-element accumulation bound
+ rows * 2^-24 * sum |y| for the sum, + rows * 2^-24 * sum y^2 for the sum of squares (rows - 1 additions and the one
rounding of the square).
"""
import ctypes as C
import math
from collections import namedtuple

import torch
import torch.nn.functional as F

from denoising_diffusion_deep_fake_amd import _lib

F32, BF16, F32X3 = _lib.F32, _lib.BF16, _lib.F32X3
DTYPE_NAMES = {F32: "f32", BF16: "bf16", F32X3: "f32x3"}
U24 = 2.0 ** -24  # unit roundoff of fp32
U8 = 2.0 ** -8    # unit roundoff of bf16 (8 significand bits)

# The aggregate gates of tests/test_gpu_ops.py and tests/test_gpu_bf16.py, kept beside the per-element bound, unchanged.
REL_L2_F32 = 1e-5
REL_L2_BF16 = 4e-3
REL_L2_WGRAD = 1e-5  # the fp32 weight gradient, of fp32 and of bf16 storage

# ---- roundings a route adds to the plain accumulation --------------------------------------------------------------
# Up-sampling folded into pre-summed weights (pack_up_kernel, pointwise.hip): a folded tap is the sum of up to four
# master weights -- three fp32 additions -- and in bf16 storage that sum is rounded to bf16 once more.  Relative to
# sum |x| |w1 + .. + w4| <= the magnitude term.
UPFOLD_F32_ADDS = 3
UPFOLD_BF16_ROUNDINGS = 1
# acc0 / acc1 (conv_igemm.hip CONV_DGRAD epilogue `v.x += o.x`, conv_splitk_reduce_kernel `x += to_f32<T>(dst[k])`,
# conv_patch.hip / conv_pres.hip `if (p.acc0)`): the existing gradient is added to the fp32 accumulator, one fp32
# addition; the result is stored with the storage type's one rounding.
ACC_ADDS = 1
# Full-resolution data gradient + d3f_upsample2x_backward (sum2x2_kernel, pointwise.hip): the full-resolution gradient
# is stored (bf16: first rounding), its 2 x 2 blocks are added in fp32 (three additions) and stored (bf16: second
# rounding).
FULLRES_SUM_ADDS = 3
FULLRES_BF16_ROUNDINGS = 2
# Class-form weight gradient (WG_CLASS, wgrad_reduce_batch_kernel with fold): every 3 x 3 tap is the sum of the four
# folded taps (one per output-parity class) it belongs to: three fp32 additions on top of the B * Ho * Wo products.
WGRAD_CLASS_ADDS = 3
# Slab reduce (wgrad_reduce_batch_kernel, conv_splitk_reduce_kernel): `splits` partial sums of n / splits products are
# added in a fixed order -- nodes of the accumulation tree, no chain longer than n: nothing to add.
SLAB_REDUCE_ADDS = 0
# D3F_F32X3: dropped products of the truncation split, in units of 2^-24 |a b| (2 * 2^-22 + 2^-30), and the cap
X3_DROPPED = 8.0 + 2.0 ** -6
X3_CAP = 4
# Winograd F(2x2, 3x3) (conv_winograd.hip): roundings of the three transforms (the contraction adds one per channel), and
# the eval epilogue's v = o * sc + sf (+ res)
WINO_INPUT_ROUNDINGS = 2
WINO_FILTER_ROUNDINGS = 4
WINO_OUTPUT_ROUNDINGS = 4
WINO_EVAL_ROUNDINGS = 2
WINO_EVAL_RES_ROUNDINGS = 3
WINO_BT = ((1, 0, -1, 0), (0, 1, 1, 0), (0, -1, 1, 0), (0, 1, 0, -1))
WINO_G = ((1, 0, 0), (.5, .5, .5), (.5, -.5, .5), (0, 0, 1))
WINO_AT = ((1, 1, 1, 0), (0, 1, -1, -1))

Case = namedtuple("Case", "dtype B H W C0 C1 Cout k stride pad up cin_real ws dirs forms why ragged entry",
                  defaults=(None, "conv"))


def case_id(c):
    return f"{DTYPE_NAMES[c.dtype]}-{c.B}x{c.H}x{c.W}-{c.C0}+{c.C1}to{c.Cout}-k{c.k}s{c.stride}-up{c.up}-ws{c.ws}" + \
        ("-wino" if c.entry == "winograd" else "")


def ve(dtype):
    return 8 if dtype == BF16 else 4


def desc_of(c):
    return _lib.ConvDesc(c.B, c.H, c.W, c.C0, c.C1, c.up, c.Cout, c.k, c.k, c.stride, c.pad, c.cin_real)


def out_hw(c):
    return (c.H + 2 * c.pad - c.k) // c.stride + 1, (c.W + 2 * c.pad - c.k) // c.stride + 1


def macs(c):
    ho, wo = out_hw(c)
    return c.B * ho * wo * c.Cout * c.k * c.k * (c.C0 + c.C1)


def plan_of(c):
    p = _lib.ConvPlan()
    d = desc_of(c)
    _lib.check(_lib.lib().d3f_conv_layer_plan(c.dtype, C.byref(d), c.ws, C.byref(p)))
    return p


# ---- forms -----------------------------------------------------------------------------------------------------------
def launch_form(dtype, name, p, wino=False):
    if wino:
        return (dtype, name, "wino")
    return (dtype, name, p.patch, p.tile_bm, p.tile_bn, p.par, p.nz, p.small_c, p.fast_addr, p.sum2, int(p.splitk > 1))


def wgrad_form(dtype, w):
    return (dtype, "wgrad", w.part, w.cls, w.patch, w.tile)


def plan_forms(dtype, plan, wino_entry=None):
    """{direction: [forms]} of a d3f_conv_plan.  wino_entry None: the forward is Winograd where the plan says so (a
    network layer); True / False: the case runs d3f_conv_winograd_forward / d3f_conv_forward whatever the plan prefers"""
    out = {"fwd": [], "dgrad": [], "wgrad": []}
    if plan.fwd.planned:
        wino = bool(plan.wino) if wino_entry is None else wino_entry
        out["fwd"].append(launch_form(dtype, "fwd", plan.fwd, wino))
    for name in ("dgrad", "dgrad_lo"):
        p = getattr(plan, name)
        if p.planned:
            out["dgrad"].append(launch_form(dtype, name, p))
    for i in range(plan.wgrad_parts):
        out["wgrad"].append(wgrad_form(dtype, plan.wgrad[i]))
    return out


def case_forms(c, plan=None):
    """the forms the case's own directions reach, in direction order"""
    f = plan_forms(c.dtype, plan_of(c) if plan is None else plan, wino_entry=c.entry == "winograd")
    return [x for d in ("fwd", "dgrad", "wgrad") if d in c.dirs for x in f[d]]


def stat_row_pixels(launch, wino=False):
    """output pixels one statistics partial row sums in fp32: the tile of the kernel that writes it"""
    if wino:
        return 256                       # conv_winograd_kernel: 16 x 16 pixels per workgroup
    if launch.splitk > 1:
        return 8                         # conv_splitk_reduce_kernel: SK_ROWS
    if launch.patch == 0:
        return launch.tile_bm            # conv_igemm_kernel: BM rows
    if launch.patch <= 8:
        return 256                       # conv_patch_kernel 4 x 64, conv_stem[_bf16]_kernel 8 x 32
    return 128 if launch.patch <= 10 else 64  # conv_pres_kernel: BM 128 / 128 / 64 / 64


# ---- data and float64 reference -----------------------------------------------------------------------------------------
def tdt(dtype):
    return torch.bfloat16 if dtype == BF16 else torch.float32


def stored(x64, dtype):
    """what the storage type keeps of a float64 tensor, as float64"""
    return x64.to(tdt(dtype)).double()


def make_data(c, seed=0):
    """x0 [B, C0 real, h0, w0], x1 [B, C1, H, W] or None, w [Cout, cin_real, k, k], dy [B, Cout, Ho, Wo]: float64 tensors
    holding storage-type values"""
    g = torch.Generator().manual_seed(1000 * seed + c.B + 7 * c.H + 13 * c.Cout)
    c0 = c.cin_real if c.C1 == 0 else c.C0
    h0, w0 = (c.H // 2, c.W // 2) if c.up else (c.H, c.W)
    ho, wo = out_hw(c)
    rn = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)  # noqa: E731
    x0 = stored(rn(c.B, c0, h0, w0), c.dtype)
    x1 = stored(rn(c.B, c.C1, c.H, c.W), c.dtype) if c.C1 else None
    w = stored(rn(c.Cout, c.cin_real, c.k, c.k) / math.sqrt(c.cin_real * c.k * c.k), c.dtype)
    dy = stored(rn(c.B, c.Cout, ho, wo), c.dtype)
    return x0, x1, w, dy


def conv_input(c, x0, x1):
    xin = x0.repeat_interleave(2, 2).repeat_interleave(2, 3) if c.up else x0
    return torch.cat([xin, x1], 1) if x1 is not None else xin


def sum2x2(t):
    return t[:, :, 0::2, 0::2] + t[:, :, 0::2, 1::2] + t[:, :, 1::2, 0::2] + t[:, :, 1::2, 1::2]


def make_exact_data(c, seed=0):
    """make_data's tensors drawn uniformly from {-1, 0, 1}: the operands on which fp32 arithmetic is exact (docstring);
    a case that broke one of exact_conditions would get more zeros here, not leave the table"""
    g = torch.Generator().manual_seed(1000 * seed + 17 + c.B + 7 * c.H + 13 * c.Cout)
    c0 = c.cin_real if c.C1 == 0 else c.C0
    h0, w0 = (c.H // 2, c.W // 2) if c.up else (c.H, c.W)
    ho, wo = out_hw(c)
    tri = lambda *s: torch.randint(-1, 2, s, generator=g).double()  # noqa: E731
    x0 = tri(c.B, c0, h0, w0)
    x1 = tri(c.B, c.C1, c.H, c.W) if c.C1 else None
    return x0, x1, tri(c.Cout, c.cin_real, c.k, c.k), tri(c.B, c.Cout, ho, wo)


def exact_conditions(c, plan, data, y=None):
    """{name: the largest magnitude an fp32 partial sum of that contraction can reach}: each must stay below 2^24 for the
    exact pass to be exact in any summation order.  y: the float64 forward result (statistics rows)"""
    x0, x1, w, dy = data
    mx = max(float(x0.abs().max()), float(x1.abs().max()) if x1 is not None else 0.0)
    mw, mdy = float(w.abs().max()), float(dy.abs().max())
    ho, wo = out_hw(c)
    wino = c.entry == "winograd"
    out = {}
    if "fwd" in c.dirs:
        # (pre-summed up-fold weights: |w1 + .. + w4| <= |w1| + .. + |w4|, the same total; Winograd: |B^T| |d| |B| <= 4 max|x|,
        # |G| |g| |G^T| <= 2.25 max|w| per position, |A^T| |M| |A| sums 9 positions, all in quarter-integers: x 4)
        out["forward contraction"] = c.k * c.k * (c.C0 + c.C1) * mx * mw * (4 * 9 * 4 * 2.25 if wino else 1)
        if y is not None:
            out["statistics row"] = stat_row_pixels(plan.fwd, wino) * float((y * y).max())
    if "dgrad" in c.dirs:
        out["data-gradient contraction"] = (4 if c.up else 1) * dgrad_n(c) * mdy * mw + 1   # + the base of acc0 / acc1
    if "wgrad" in c.dirs:
        out["weight-gradient contraction"] = c.B * ho * wo * mx * mdy * (4 if c.up else 1)  # (class form: four taps)
    return out


def reference(c, data, dirs=None, mags=True):
    """float64 results and (mags) magnitude terms (the same contractions on absolute values) of the directions asked for,
    NCHW: y, y_mag; dx (gradient of the conv input, all channels, full resolution), dx_mag; dw, dw_mag"""
    x0, x1, w, dy = data
    dirs = c.dirs if dirs is None else dirs
    xin = conv_input(c, x0, x1)
    r = {}
    if "fwd" in dirs:
        r["y"] = F.conv2d(xin, w, None, c.stride, c.pad)
        if mags:
            r["y_mag"] = F.conv2d(xin.abs(), w.abs(), None, c.stride, c.pad)
    if "dgrad" in dirs:
        r["dx"] = torch.nn.grad.conv2d_input(xin.shape, w, dy, c.stride, c.pad)
        if mags:
            r["dx_mag"] = torch.nn.grad.conv2d_input(xin.shape, w.abs(), dy.abs(), c.stride, c.pad)
    if "wgrad" in dirs:
        r["dw"] = torch.nn.grad.conv2d_weight(xin, w.shape, dy, c.stride, c.pad)
        if mags:
            r["dw_mag"] = torch.nn.grad.conv2d_weight(xin.abs(), w.shape, dy.abs(), c.stride, c.pad)
    return r


# ---- Winograd F(2x2, 3x3) in float64 ---------------------------------------------------------------------------------------
def winograd_tiles(x):
    """[B, C, H, W] -> the 4 x 4 input tiles at stride 2 on the zero-padded input, [B, C, 4, 4, H / 2, W / 2]"""
    H, W = x.shape[2:]
    xp = F.pad(x, (1, 1, 1, 1))
    return torch.stack([torch.stack([xp[:, :, a:a + H:2, b:b + W:2] for b in range(4)], 2) for a in range(4)], 2)


def winograd_eval(x, w, absolute=False):
    """A^T [ sum_c (G g G^T) (.) (B^T d B) ] A in float64, [B, K, H, W]; absolute: on |x|, |w| with |B^T|, |G|, |A^T| -- the
    magnitude term Ymag of the Winograd bound"""
    bt, g, at = (torch.tensor(m, dtype=torch.float64) for m in (WINO_BT, WINO_G, WINO_AT))
    x, w = x.double(), w.double()
    if absolute:
        x, w, bt, g, at = x.abs(), w.abs(), bt.abs(), g.abs(), at.abs()
    v = torch.einsum("ia,bcaets,je->bcijts", bt, winograd_tiles(x), bt)
    u = torch.einsum("ia,kcae,je->kcij", g, w, g)
    m = torch.einsum("kcij,bcijts->bkijts", u, v)
    y = torch.einsum("pi,bkijts,qj->bktpsq", at, m, at)
    return y.reshape(x.shape[0], w.shape[0], x.shape[2], x.shape[3])


# ---- bounds --------------------------------------------------------------------------------------------------------------
def acc_roundings(dtype, n):
    """roundings (in units of 2^-24 of the magnitude term) of an n-term contraction in the compute type"""
    if dtype == F32X3:
        return min(6 * math.ceil(n / 16) + X3_DROPPED, n + X3_CAP)
    return n


def store_rounding(dtype, ref, err):
    """the bound after the result is stored: bf16 storage rounds the fp32 value once"""
    return err + U8 * (ref.abs() + err) if dtype == BF16 else err


def upfold_terms(dtype, mag):
    """pre-summed weights of a folded layer, relative to the magnitude term"""
    t = UPFOLD_F32_ADDS * U24 * mag
    if dtype == BF16:
        t = t + UPFOLD_BF16_ROUNDINGS * U8 * mag
    return t


def fwd_acc_bound(c, plan, y_mag):
    """the fp32 accumulator of the forward pass (what the statistics sum): before the storage rounding"""
    n = c.k * c.k * (c.C0 + c.C1)
    b = acc_roundings(c.dtype, n) * U24 * y_mag
    return b + upfold_terms(c.dtype, y_mag) if plan.upfold else b


def fwd_bound(c, plan, y, y_mag):
    return store_rounding(c.dtype, y, fwd_acc_bound(c, plan, y_mag))


def dgrad_route(c, plan):
    """how dx0 of an up-sampled source comes back: "plain" (no up-sampling), "folded" (dgrad_lo), "summed" (2 x 2 sums in
    the launch's epilogue) or "fullres" (full-resolution gradient, then d3f_upsample2x_backward)"""
    if not c.up:
        return "plain"
    if plan.upfold:
        return "folded"
    return "summed" if plan.dgrad.sum2 else "fullres"


def dgrad_n(c):
    coutd = (c.Cout + ve(c.dtype) - 1) // ve(c.dtype) * ve(c.dtype)
    return c.k * c.k * coutd


def dgrad_full_err(c, dx_mag):
    """the fp32 accumulator of a gradient written at the conv input's own resolution by one launch (dx1, dx0 without
    up-sampling, the full-resolution scratch): before the storage rounding"""
    return acc_roundings(c.dtype, dgrad_n(c)) * U24 * dx_mag


def dgrad_full_bound(c, dx, dx_mag):
    return store_rounding(c.dtype, dx, dgrad_full_err(c, dx_mag))


def dgrad_low_err(c, plan, dx0, dx0_mag):
    """dx0 of an up-sampled source at its own low resolution, before the last storage rounding; dx0 / dx0_mag: the
    FULL-resolution reference and magnitude"""
    route = dgrad_route(c, plan)
    if route == "fullres":
        full_err = dgrad_full_bound(c, dx0, dx0_mag)               # bf16: the first of FULLRES_BF16_ROUNDINGS
        return sum2x2(full_err) + FULLRES_SUM_ADDS * U24 * sum2x2(dx0.abs() + full_err)
    mag = sum2x2(dx0_mag)
    err = acc_roundings(c.dtype, 4 * dgrad_n(c)) * U24 * mag       # 2 x 2 blocks summed: n x 4
    return err + upfold_terms(c.dtype, mag) if route == "folded" else err


def dgrad_low_bound(c, plan, dx0, dx0_mag):
    return store_rounding(c.dtype, sum2x2(dx0), dgrad_low_err(c, plan, dx0, dx0_mag))  # bf16: the second rounding


def acc_bound(c, base, grad, grad_err):
    """destination = base + gradient: ACC_ADDS fp32 addition to the accumulator (error grad_err), then the storage
    rounding.  Returns (base + gradient, bound)."""
    total = base + grad
    err = grad_err + ACC_ADDS * U24 * (base.abs() + grad.abs() + grad_err)
    return total, store_rounding(c.dtype, total, err)


def wgrad_bound(c, plan, dw_mag):
    ho, wo = out_hw(c)
    n = c.B * ho * wo
    extra = SLAB_REDUCE_ADDS + (WGRAD_CLASS_ADDS if any(plan.wgrad[i].cls for i in range(plan.wgrad_parts)) else 0)
    return (acc_roundings(c.dtype, n) + extra) * U24 * dw_mag  # the gradient is fp32 in every storage type


def stats_reference(c, plan, y, y_mag, wino=False, acc=None):
    """per-channel (sum y, sum y^2) in float64 and their bounds; acc: the accumulator bound where it is not the plain
    contraction's (Winograd: wino_acc_bound)"""
    acc = fwd_acc_bound(c, plan, y_mag) if acc is None else acc
    rows = stat_row_pixels(plan.fwd, wino)
    s1, s2 = y.sum((0, 2, 3)), (y * y).sum((0, 2, 3))
    b1 = acc.sum((0, 2, 3)) + rows * U24 * y.abs().sum((0, 2, 3))
    b2 = (2 * y.abs() * acc + acc * acc).sum((0, 2, 3)) + rows * U24 * s2
    return s1, s2, b1, b2


def gamma(n):
    """n roundings compounded: (1 + 2^-24)^n - 1 <= n * 2^-24 / (1 - n * 2^-24)"""
    return n * U24 / (1.0 - n * U24)


def wino_roundings(c):
    return c.C0 + WINO_INPUT_ROUNDINGS + WINO_FILTER_ROUNDINGS + WINO_OUTPUT_ROUNDINGS


def wino_acc_bound(c, wino_mag):
    """conv_winograd_kernel's output before the epilogue; wino_mag = winograd_eval(x, w, absolute=True)"""
    return gamma(wino_roundings(c)) * wino_mag


def wino_eval_reference(o, o_err, scale, shift, res, relu):
    """the eval epilogue relu?(o * scale + shift + res?) in float64 and its bound.  o, o_err: the float64 convolution
    and the bound of the kernel's own o; scale, shift [K]; res like o or None"""
    sc, sf = scale.double().view(1, -1, 1, 1), shift.double().view(1, -1, 1, 1)
    ref = o * sc + sf
    terms = (o * sc).abs() + sf.abs()
    k = WINO_EVAL_ROUNDINGS
    if res is not None:
        ref, terms, k = ref + res, terms + res.abs(), WINO_EVAL_RES_ROUNDINGS
    return (ref.clamp_min(0.0) if relu else ref), sc.abs() * o_err + k * U24 * terms


def violations(got, ref, bound):
    """(elements with |got - ref| > bound, worst |got - ref| / bound); NaN counts as a violation"""
    err = (got.double() - ref).abs()
    bad = ~(err <= bound)
    ratio = (err / bound.clamp_min(1e-300))
    ratio = torch.where(torch.isnan(ratio), torch.full_like(ratio, float("inf")), ratio)
    return int(bad.sum()), float(ratio.max()) if ratio.numel() else 0.0


def rel_l2(a, b):
    a, b = a.double(), b.double()
    return ((a - b).norm() / b.norm().clamp_min(1e-30)).item()


def to_nhwc(x, cpad=None):
    x = x.permute(0, 2, 3, 1)
    if cpad is not None and cpad > x.shape[-1]:
        x = F.pad(x, (0, cpad - x.shape[-1]))
    return x.contiguous()


def to_nchw(x, c=None):
    x = x.permute(0, 3, 1, 2)
    return (x if c is None else x[:, :c]).contiguous()


# ---- the whole-network plans the coverage test reads ------------------------------------------------------------------
# (dtype, B, H, W, nets): tests/test_cpu_lib.py and BASELINE.json name them
NETWORK_PLANS = [(F32, 16, 256, 256, 1), (BF16, 16, 256, 256, 1), (F32, 16, 128, 128, 1), (BF16, 16, 128, 128, 1),
                 (F32, 2, 448, 448, 1), (BF16, 2, 448, 448, 1), (F32, 8, 256, 256, 2), (BF16, 8, 256, 256, 2),
                 (F32X3, 16, 256, 256, 1)]


def network_layers(dtype, B, H, W, nets):
    """[(conv desc fields, d3f_conv_plan)] of Unet(resnet34) as the engine planned it (host only)"""
    L = _lib.lib()
    h = C.c_void_p()
    _lib.check(L.d3f_unet_create_nets(b"resnet34", 3, 3, B, H, W, dtype, nets, nets, C.byref(h)))
    try:
        out = []
        for i in range(L.d3f_unet_num_conv_layers(h)):
            d, p = _lib.ConvDesc(), _lib.ConvPlan()
            _lib.check(L.d3f_unet_conv_layer(h, i, C.byref(d), C.byref(p)))
            out.append((tuple(getattr(d, k) for k, _ in _lib.ConvDesc._fields_), p))
        return out
    finally:
        L.d3f_unet_destroy(h)


ALL = ("fwd", "dgrad", "wgrad")

# The table: the 13 description fields, the directions the case runs, the forms d3f_conv_layer_plan must report for
# those directions (test_cpu_conv_forms.py asserts them, so a planner change that moves a case fails there), what the
# case is there for, and optionally `ragged` ("patch" / "tap": the weight gradient's workgroups take unequal shares) and
# `entry` ("winograd": through d3f_conv_winograd_forward).  The first block carries over the shapes of the older operator
# tests and adds the ragged persistent weight gradients; the "smallest extent found" cases come from a search over
# B in 1..16, 27 extents, channel counts 8..512 and both workspace settings for the fewest multiply-adds whose plan
# shows a form some whole-network plan takes and no earlier case reaches.  A case above 3e8 multiply-adds runs only
# the directions it is there for (the float64 reference of the others would be most of its time).
CASES = [
    Case(BF16, 12, 64, 64, 64, 0, 64, 3, 1, 1, 0, 64, 0, ('fwd', 'dgrad', 'wgrad'),
         [(BF16, 'fwd', 9, 0, 0, 0, 1, 0, 0, 0, 0), (BF16, 'dgrad', 9, 0, 0, 0, 1, 0, 0, 0, 0), (BF16, 'wgrad', 0, 0, 7, 0)],
         'conv_pres_kernel layer1 form at 384 workgroups: 3.1 M outputs, the case the rel-L2 gate cannot guard'),
    Case(F32, 5, 128, 128, 16, 0, 16, 3, 1, 1, 0, 16, 0, ('fwd', 'dgrad', 'wgrad'),
         [(F32, 'fwd', 1, 0, 0, 0, 1, 0, 0, 0, 0), (F32, 'dgrad', 1, 0, 0, 0, 1, 0, 0, 0, 0), (F32, 'wgrad', 0, 0, 2, 0)],
         'persistent patch weight gradient variant 2: 640 tiles over 512 workgroups', 'patch', 'conv'),
    Case(F32, 5, 128, 128, 32, 0, 16, 3, 1, 1, 0, 32, 0, ('wgrad',),
         [(F32, 'wgrad', 0, 0, 1, 0)],
         'whole-layer (non-class) patch weight gradient variant 1: 640 tiles over 512 workgroups', 'patch', 'conv'),
    Case(F32, 5, 128, 128, 32, 0, 32, 3, 1, 1, 0, 32, 0, ('wgrad',),
         [(F32, 'wgrad', 0, 0, 3, 0)],
         'whole-layer patch weight gradient variant 3: 640 tiles over 512 workgroups', 'patch', 'conv'),
    Case(F32, 5, 128, 128, 32, 0, 16, 3, 1, 1, 2, 32, 0, ('wgrad',),
         [(F32, 'wgrad', 1, 1, 1, 0)],
         'class-form patch weight gradient variant 1: 640 tiles over 256 workgroups per row parity', 'patch', 'conv'),
    Case(F32, 5, 256, 256, 4, 0, 32, 7, 2, 3, 0, 3, 0, ('wgrad',),
         [(F32, 'wgrad', 0, 0, 4, 0)],
         'stem weight gradient variant 4: 640 tiles over 512 workgroups', 'patch', 'conv'),
    Case(BF16, 5, 256, 256, 8, 0, 32, 7, 2, 3, 0, 3, 0, ('wgrad',),
         [(BF16, 'wgrad', 0, 0, 6, 0)],
         'bf16 stem weight gradient variant 6 (half vectors): 640 tiles over 512 workgroups', 'patch', 'conv'),
    Case(BF16, 2, 64, 96, 8, 0, 64, 7, 2, 3, 0, 8, 0, ('wgrad',),
         [(BF16, 'wgrad', 0, 0, 5, 0)],
         'bf16 stem weight gradient variant 5 (eight staged channels)'),
    Case(BF16, 3, 128, 128, 16, 0, 16, 3, 1, 1, 0, 16, 0, ('fwd', 'dgrad', 'wgrad'),
         [(BF16, 'fwd', 3, 0, 0, 0, 1, 0, 0, 0, 0), (BF16, 'dgrad', 3, 0, 0, 0, 1, 0, 0, 0, 0), (BF16, 'wgrad', 0, 0, 7, 0)],
         'native-bf16 patch weight gradient variant 7: 384 tiles over 256 workgroups', 'patch', 'conv'),
    Case(F32, 3, 10, 10, 32, 0, 64, 3, 1, 1, 0, 32, 0, ('fwd', 'dgrad', 'wgrad'),
         [(F32, 'fwd', 0, 32, 32, 0, 1, 0, 1, 0, 0), (F32, 'dgrad', 0, 256, 32, 0, 1, 0, 1, 0, 0), (F32, 'wgrad', 0, 0, 0, 32)],
         'ragged M (300 rows); tap-parallel weight gradient with a short last slab', 'tap', 'conv'),
    Case(F32, 1, 16, 16, 16, 0, 64, 3, 1, 1, 0, 16, 0, ('fwd',),
         [(F32, 'fwd', 'wino')],
         'conv_winograd_kernel: one workgroup, every image border inside one patch', None, 'winograd'),
    Case(F32, 1, 16, 16, 32, 0, 64, 3, 1, 1, 0, 32, 0, ('fwd',),
         [(F32, 'fwd', 'wino')],
         'conv_winograd_kernel: two chunks, the last one contracted from V[1] (1 and 3 chunks both end in V[0])', None, 'winograd'),
    Case(F32, 2, 32, 48, 48, 0, 128, 3, 1, 1, 0, 48, 0, ('fwd',),
         [(F32, 'fwd', 'wino')],
         'conv_winograd_kernel: odd chunk count, two filter blocks, non-square', None, 'winograd'),
    Case(BF16, 2, 8, 64, 32, 0, 16, 3, 1, 1, 1, 32, 0, ('fwd', 'dgrad', 'wgrad'),
         [(BF16, 'fwd', 5, 0, 0, 0, 1, 0, 0, 0, 0), (BF16, 'dgrad', 0, 256, 32, 0, 1, 1, 0, 0, 0), (BF16, 'wgrad', 0, 0, 7, 0)],
         'up-sampled source on the full-resolution contract: two bf16 roundings (d3f_upsample2x_backward)'),
    Case(BF16, 1, 12, 128, 32, 0, 8, 3, 1, 1, 2, 32, 0, ('fwd', 'dgrad', 'wgrad'),
         [(BF16, 'fwd', 5, 0, 0, 0, 1, 0, 0, 0, 0), (BF16, 'dgrad', 0, 256, 32, 0, 1, 1, 0, 0, 0), (BF16, 'wgrad', 0, 0, 7, 0)],
         'up-sampled bf16 patch forward, two tiles per row, 8 of 16 filter columns real'),
    Case(F32, 2, 16, 16, 16, 0, 16, 3, 1, 1, 2, 16, 0, ('fwd', 'dgrad', 'wgrad'),
         [(F32, 'fwd', 0, 256, 16, 0, 1, 1, 0, 0, 0), (F32, 'dgrad', 0, 256, 16, 0, 1, 1, 0, 0, 0), (F32, 'wgrad', 0, 0, 2, 0)],
         'fp32 up-sampled source that is not folded: full-resolution gradient + 2x2 sum'),
    Case(F32, 2, 24, 40, 16, 0, 3, 3, 1, 1, 0, 16, 0, ('dgrad', 'wgrad'),
         [(F32, 'dgrad', 0, 256, 16, 0, 1, 1, 0, 0, 0), (F32, 'wgrad', 0, 0, 2, 0)],
         'head shape (3 outputs), extent ragged against the 4 x 64 patch tile'),
    Case(F32, 2, 8, 64, 16, 0, 3, 3, 1, 1, 0, 16, 0, ('dgrad', 'wgrad'),
         [(F32, 'dgrad', 1, 0, 0, 0, 1, 0, 0, 0, 0), (F32, 'wgrad', 0, 0, 2, 0)],
         'head data gradient through conv_patch_kernel<float, 4, 16>'),
    Case(BF16, 1, 12, 128, 16, 0, 3, 3, 1, 1, 0, 16, 0, ('dgrad', 'wgrad'),
         [(BF16, 'dgrad', 6, 0, 0, 0, 1, 0, 0, 0, 0), (BF16, 'wgrad', 0, 0, 7, 0)],
         'bf16 head data gradient (dY 3 -> 8 channels staged as 16), two tiles per row'),
    Case(F32, 1, 24, 40, 64, 64, 32, 3, 1, 1, 2, 128, 0, ('fwd', 'dgrad', 'wgrad'),
         [(F32, 'fwd', 0, 256, 32, 3, 4, 0, 0, 0, 0), (F32, 'dgrad', 0, 32, 32, 0, 1, 0, 1, 0, 0), (F32, 'dgrad_lo', 0, 32, 32, 0, 1, 0, 1, 0, 0), (F32, 'wgrad', 1, 1, 3, 0), (F32, 'wgrad', 2, 0, 3, 0)],
         'folded decoder layer, ragged 256-row tiles'),
    Case(F32, 3, 12, 20, 128, 64, 128, 3, 1, 1, 2, 192, 1, ('fwd', 'dgrad', 'wgrad'),
         [(F32, 'fwd', 0, 32, 32, 3, 4, 0, 0, 0, 1), (F32, 'dgrad', 0, 32, 32, 0, 1, 0, 1, 0, 1), (F32, 'dgrad_lo', 0, 32, 32, 0, 1, 0, 1, 0, 1), (F32, 'wgrad', 1, 1, 0, 64), (F32, 'wgrad', 2, 0, 0, 64)],
         'class-form weight gradient on a ragged class grid (3 x 6 x 10 low-resolution pixels)'),
    Case(BF16, 3, 12, 20, 128, 64, 128, 3, 1, 1, 2, 192, 1, ('fwd', 'dgrad', 'wgrad'),
         [(BF16, 'fwd', 0, 32, 32, 3, 4, 0, 0, 0, 1), (BF16, 'dgrad', 0, 32, 32, 0, 1, 0, 1, 0, 1), (BF16, 'dgrad_lo', 0, 32, 32, 0, 1, 0, 1, 0, 1), (BF16, 'wgrad', 0, 0, 7, 0)],
         '... in bf16 storage'),
    Case(F32X3, 3, 12, 20, 128, 64, 128, 3, 1, 1, 2, 192, 0, ('fwd', 'dgrad', 'wgrad'),
         [(F32X3, 'fwd', 0, 64, 64, 3, 4, 0, 0, 0, 0), (F32X3, 'dgrad', 0, 64, 64, 0, 1, 0, 1, 0, 0), (F32X3, 'dgrad_lo', 0, 64, 64, 0, 1, 0, 1, 0, 0), (F32X3, 'wgrad', 1, 1, 0, 64), (F32X3, 'wgrad', 2, 0, 0, 64)],
         '... on the f32x3 contraction'),
    Case(BF16, 3, 4, 64, 32, 0, 24, 3, 1, 1, 0, 32, 0, ('fwd', 'dgrad', 'wgrad'),
         [(BF16, 'fwd', 4, 0, 0, 0, 1, 0, 0, 0, 0), (BF16, 'dgrad', 0, 256, 32, 0, 1, 1, 0, 0, 0), (BF16, 'wgrad', 0, 0, 7, 0)],
         'bf16 32-channel patch kernel, ragged filter count, one tile row per image'),
    Case(BF16, 1, 12, 128, 48, 0, 32, 3, 1, 1, 0, 48, 0, ('fwd', 'dgrad', 'wgrad'),
         [(BF16, 'fwd', 0, 256, 32, 0, 1, 1, 0, 0, 0), (BF16, 'dgrad', 4, 0, 0, 0, 1, 0, 0, 0, 0), (BF16, 'wgrad', 0, 0, 0, 32)],
         'bf16 data gradient 32 -> 48 channels: the second filter half is half empty'),
    Case(F32, 2, 32, 64, 4, 0, 64, 7, 2, 3, 0, 3, 0, ('fwd', 'wgrad'),
         [(F32, 'fwd', 2, 0, 0, 0, 1, 0, 0, 0, 0), (F32, 'wgrad', 0, 0, 4, 0)],
         'conv_stem_kernel: image borders on all four sides, garbage in the pad channel'),
    Case(BF16, 1, 48, 128, 8, 0, 64, 7, 2, 3, 0, 3, 0, ('fwd', 'wgrad'),
         [(BF16, 'fwd', 8, 0, 0, 0, 1, 0, 0, 0, 0), (BF16, 'wgrad', 0, 0, 6, 0)],
         'conv_stem_bf16_kernel: garbage in pad channels 3..7'),
    Case(F32X3, 2, 32, 32, 4, 0, 64, 7, 2, 3, 0, 3, 0, ('fwd', 'wgrad'),
         [(F32X3, 'fwd', 0, 64, 64, 0, 1, 1, 0, 0, 0), (F32X3, 'wgrad', 0, 0, 4, 0)],
         'f32x3 stem through the small-channel loader'),
    Case(BF16, 1, 4, 4, 64, 64, 256, 3, 1, 1, 2, 128, 0, ('fwd', 'dgrad', 'wgrad'),
         [(BF16, 'fwd', 0, 32, 32, 3, 4, 0, 0, 0, 0), (BF16, 'dgrad', 0, 32, 32, 0, 1, 0, 1, 0, 0), (BF16, 'dgrad_lo', 0, 32, 32, 0, 1, 0, 1, 0, 0), (BF16, 'wgrad', 1, 1, 0, 64), (BF16, 'wgrad', 2, 0, 0, 64)],
         'smallest extent found for conv_igemm_kernel<bf16_t, 32, 32, FAST 1> (dgrad); conv_igemm_kernel<bf16_t, 32, 32, FAST 1> (dgrad_lo); conv_igemm_kernel<bf16_t, 32, 32, FAST 2 (up-folded)> (fwd); conv_wgrad_kernel<bf16_t, 64, 64, 2, 2, 1, bf16 MFMA, CLS> + wgrad_reduce_batch_kernel (wgrad); conv_wgrad_kernel<bf16_t, 64, 64, 2, 2, 1, bf16 MFMA> + wgrad_reduce_batch_kernel (wgrad)'),
    Case(F32X3, 1, 4, 4, 32, 32, 32, 3, 1, 1, 2, 64, 0, ('fwd', 'dgrad', 'wgrad'),
         [(F32X3, 'fwd', 0, 256, 32, 3, 4, 0, 0, 0, 0), (F32X3, 'dgrad', 0, 256, 32, 0, 1, 0, 1, 0, 0), (F32X3, 'dgrad_lo', 0, 256, 32, 0, 1, 0, 1, 0, 0), (F32X3, 'wgrad', 1, 1, 3, 0), (F32X3, 'wgrad', 2, 0, 3, 0)],
         'smallest extent found for conv_igemm_kernel<float, 256, 32, FAST 1, X3> (dgrad); conv_igemm_kernel<float, 256, 32, FAST 2 (up-folded), X3> (fwd); conv_wgrad_patch_cls_kernel<float, 32, 32, 16> + wgrad_reduce_batch_kernel (wgrad); conv_wgrad_patch_kernel<float, 32, 32, 3, 1, 16> + wgrad_reduce_batch_kernel (wgrad)'),
    Case(BF16, 1, 4, 4, 64, 0, 64, 1, 2, 0, 0, 64, 0, ('fwd', 'dgrad', 'wgrad'),
         [(BF16, 'fwd', 0, 32, 32, 0, 1, 0, 1, 0, 0), (BF16, 'dgrad', 0, 32, 32, 2, 1, 0, 1, 0, 0), (BF16, 'wgrad', 0, 0, 0, 64)],
         'smallest extent found for conv_igemm_kernel<bf16_t, 32, 32, FAST 1> (fwd); conv_igemm_kernel<bf16_t, 32, 32, FAST 1> par 2 (dgrad); conv_wgrad_kernel<bf16_t, 64, 64, 2, 2, 1, bf16 MFMA> + wgrad_reduce_batch_kernel (wgrad)'),
    Case(F32X3, 1, 4, 4, 64, 0, 64, 1, 2, 0, 0, 64, 0, ('fwd', 'dgrad', 'wgrad'),
         [(F32X3, 'fwd', 0, 64, 64, 0, 1, 0, 1, 0, 0), (F32X3, 'dgrad', 0, 64, 64, 2, 1, 0, 1, 0, 0), (F32X3, 'wgrad', 0, 0, 0, 64)],
         'smallest extent found for conv_igemm_kernel<float, 64, 64, FAST 1, X3> (fwd); conv_igemm_kernel<float, 64, 64, FAST 1, X3> par 2 (dgrad); conv_wgrad_kernel<float, 64, 64, 2, 2, 1, bf16 MFMA> + wgrad_reduce_batch_kernel (wgrad)'),
    Case(F32X3, 1, 4, 4, 32, 0, 8, 3, 1, 1, 2, 32, 0, ('fwd', 'dgrad', 'wgrad'),
         [(F32X3, 'fwd', 0, 256, 16, 3, 4, 0, 1, 0, 0), (F32X3, 'dgrad_lo', 0, 256, 32, 0, 1, 1, 0, 0, 0), (F32X3, 'wgrad', 1, 1, 1, 0)],
         'smallest extent found for conv_igemm_kernel<float, 256, 16, FAST 2 (up-folded), X3> (fwd); conv_igemm_kernel<float, 256, 32, SMALLC, X3> (dgrad_lo); conv_wgrad_patch_cls_kernel<float, 16, 32, 16> + wgrad_reduce_batch_kernel (wgrad)'),
    Case(F32, 1, 4, 4, 512, 0, 64, 1, 2, 0, 0, 512, 1, ('fwd', 'dgrad', 'wgrad'),
         [(F32, 'fwd', 0, 32, 32, 0, 1, 0, 1, 0, 1), (F32, 'dgrad', 0, 32, 32, 2, 1, 0, 1, 0, 0), (F32, 'wgrad', 0, 0, 0, 64)],
         'smallest extent found for conv_igemm_kernel<float, 32, 32, FAST 1> + conv_splitk_reduce_kernel (fwd); conv_igemm_kernel<float, 32, 32, FAST 1> par 2 (dgrad); conv_wgrad_kernel<float, 64, 64, 2, 2, 1> + wgrad_reduce_batch_kernel (wgrad)'),
    Case(F32X3, 1, 4, 4, 8, 0, 8, 1, 2, 0, 0, 8, 0, ('fwd', 'dgrad', 'wgrad'),
         [(F32X3, 'fwd', 0, 256, 16, 0, 1, 1, 0, 0, 0), (F32X3, 'dgrad', 0, 256, 16, 0, 1, 1, 0, 0, 0), (F32X3, 'wgrad', 0, 0, 0, 32)],
         'smallest extent found for conv_igemm_kernel<float, 256, 16, SMALLC, X3> (dgrad); conv_igemm_kernel<float, 256, 16, SMALLC, X3> (fwd)'),
    Case(F32, 1, 4, 4, 32, 0, 8, 3, 1, 1, 2, 32, 0, ('fwd', 'dgrad', 'wgrad'),
         [(F32, 'fwd', 0, 256, 16, 3, 4, 0, 1, 0, 0), (F32, 'dgrad_lo', 0, 256, 32, 0, 1, 1, 0, 0, 0), (F32, 'wgrad', 1, 1, 1, 0)],
         'smallest extent found for conv_igemm_kernel<float, 256, 16, FAST 2 (up-folded)> (fwd); conv_igemm_kernel<float, 256, 32, SMALLC> (dgrad_lo)'),
    Case(F32, 1, 4, 4, 64, 0, 32, 3, 2, 1, 0, 64, 0, ('fwd', 'dgrad', 'wgrad'),
         [(F32, 'fwd', 0, 256, 32, 0, 1, 0, 1, 0, 0), (F32, 'dgrad', 0, 32, 32, 1, 4, 0, 1, 0, 0), (F32, 'wgrad', 0, 0, 0, 32)],
         'smallest extent found for conv_igemm_kernel<float, 256, 32, FAST 1> (fwd); conv_igemm_kernel<float, 32, 32, FAST 1> par 1 (dgrad)'),
    Case(F32X3, 1, 4, 4, 64, 0, 32, 3, 2, 1, 0, 64, 0, ('fwd', 'dgrad', 'wgrad'),
         [(F32X3, 'fwd', 0, 256, 32, 0, 1, 0, 1, 0, 0), (F32X3, 'dgrad', 0, 64, 64, 1, 4, 0, 1, 0, 0), (F32X3, 'wgrad', 0, 0, 0, 32)],
         'smallest extent found for conv_igemm_kernel<float, 256, 32, FAST 1, X3> (fwd); conv_igemm_kernel<float, 64, 64, FAST 1, X3> par 1 (dgrad)'),
    Case(BF16, 1, 4, 4, 128, 0, 64, 3, 2, 1, 0, 128, 1, ('fwd', 'dgrad', 'wgrad'),
         [(BF16, 'fwd', 0, 32, 32, 0, 1, 0, 1, 0, 1), (BF16, 'dgrad', 0, 32, 32, 1, 4, 0, 1, 0, 0), (BF16, 'wgrad', 0, 0, 0, 64)],
         'smallest extent found for conv_igemm_kernel<bf16_t, 32, 32, FAST 1> + conv_splitk_reduce_kernel (fwd); conv_igemm_kernel<bf16_t, 32, 32, FAST 1> par 1 (dgrad)'),
    Case(BF16, 16, 16, 128, 128, 0, 32, 3, 1, 1, 0, 128, 0, ('fwd', 'dgrad'),
         [(BF16, 'fwd', 10, 0, 0, 0, 1, 0, 0, 0, 0), (BF16, 'dgrad', 0, 128, 64, 0, 1, 1, 0, 0, 0)],
         'smallest extent found for conv_igemm_kernel<bf16_t, 128, 64, SMALLC> (dgrad); conv_pres_kernel<128, 32, 4, 1, 1, 1> (fwd)'),
    Case(F32X3, 1, 4, 4, 16, 0, 3, 3, 1, 1, 0, 16, 0, ('dgrad', 'wgrad'),
         [(F32X3, 'dgrad', 0, 256, 16, 0, 1, 1, 0, 0, 0), (F32X3, 'wgrad', 0, 0, 2, 0)],
         'smallest extent found for conv_wgrad_patch_kernel<float, 16, 16, 3, 1, 16> + wgrad_reduce_batch_kernel (wgrad)'),
    Case(F32X3, 1, 4, 4, 512, 0, 64, 1, 2, 0, 0, 512, 1, ('fwd', 'dgrad', 'wgrad'),
         [(F32X3, 'fwd', 0, 64, 64, 0, 1, 0, 1, 0, 1), (F32X3, 'dgrad', 0, 64, 64, 2, 1, 0, 1, 0, 0), (F32X3, 'wgrad', 0, 0, 0, 64)],
         'smallest extent found for conv_igemm_kernel<float, 64, 64, FAST 1, X3> + conv_splitk_reduce_kernel (fwd)'),
    Case(F32X3, 1, 4, 4, 32, 0, 32, 3, 1, 1, 0, 32, 0, ('fwd', 'dgrad', 'wgrad'),
         [(F32X3, 'fwd', 0, 256, 32, 0, 1, 0, 1, 0, 0), (F32X3, 'dgrad', 0, 256, 32, 0, 1, 0, 1, 0, 0), (F32X3, 'wgrad', 0, 0, 3, 0)],
         'smallest extent found for conv_wgrad_patch_kernel<float, 32, 32, 3, 1, 16> + wgrad_reduce_batch_kernel (wgrad)'),
    Case(F32, 1, 4, 4, 8, 32, 32, 3, 1, 1, 0, 40, 0, ('dgrad',),
         [(F32, 'dgrad', 0, 64, 64, 0, 1, 0, 1, 0, 0)],
         'smallest extent found for conv_igemm_kernel<float, 64, 64, FAST 1> (dgrad)'),
    Case(F32, 1, 4, 4, 32, 32, 32, 3, 1, 1, 2, 64, 1, ('fwd', 'dgrad', 'wgrad'),
         [(F32, 'fwd', 0, 256, 32, 3, 4, 0, 0, 0, 1), (F32, 'dgrad', 0, 256, 32, 0, 1, 0, 1, 0, 0), (F32, 'dgrad_lo', 0, 256, 32, 0, 1, 0, 1, 0, 1), (F32, 'wgrad', 1, 1, 3, 0), (F32, 'wgrad', 2, 0, 3, 0)],
         'smallest extent found for conv_igemm_kernel<float, 256, 32, FAST 2 (up-folded)> + conv_splitk_reduce_kernel (fwd)'),
    Case(F32X3, 1, 4, 4, 64, 0, 32, 3, 1, 1, 2, 64, 1, ('fwd', 'dgrad', 'wgrad'),
         [(F32X3, 'fwd', 0, 256, 32, 3, 4, 0, 1, 0, 0), (F32X3, 'dgrad_lo', 0, 64, 64, 0, 1, 0, 1, 0, 1), (F32X3, 'wgrad', 1, 1, 3, 0)],
         'smallest extent found for conv_igemm_kernel<float, 64, 64, FAST 1, X3> + conv_splitk_reduce_kernel (dgrad_lo)'),
    Case(BF16, 1, 4, 4, 8, 32, 64, 3, 1, 1, 0, 40, 0, ('dgrad',),
         [(BF16, 'dgrad', 0, 64, 64, 0, 1, 0, 1, 0, 0)],
         'smallest extent found for conv_igemm_kernel<bf16_t, 64, 64, FAST 1> (dgrad)'),
    Case(F32, 1, 4, 4, 32, 32, 64, 3, 1, 1, 2, 64, 0, ('fwd', 'dgrad'),
         [(F32, 'fwd', 0, 32, 32, 3, 4, 0, 0, 0, 0), (F32, 'dgrad', 0, 256, 32, 0, 1, 0, 1, 0, 0), (F32, 'dgrad_lo', 0, 256, 32, 0, 1, 0, 1, 0, 0)],
         'smallest extent found for conv_igemm_kernel<float, 32, 32, FAST 2 (up-folded)> (fwd)'),
    Case(BF16, 1, 4, 4, 64, 64, 32, 3, 1, 1, 2, 128, 0, ('fwd', 'dgrad', 'wgrad'),
         [(BF16, 'fwd', 0, 256, 32, 3, 4, 0, 0, 0, 0), (BF16, 'dgrad', 0, 32, 32, 0, 1, 1, 0, 0, 0), (BF16, 'dgrad_lo', 0, 32, 32, 0, 1, 1, 0, 0, 0), (BF16, 'wgrad', 0, 0, 7, 0)],
         'smallest extent found for conv_igemm_kernel<bf16_t, 256, 32, FAST 2 (up-folded)> (fwd)'),
    Case(BF16, 1, 4, 4, 64, 64, 32, 3, 1, 1, 2, 128, 1, ('fwd', 'dgrad', 'wgrad'),
         [(BF16, 'fwd', 0, 256, 32, 3, 4, 0, 0, 0, 1), (BF16, 'dgrad', 0, 32, 32, 0, 1, 1, 0, 0, 0), (BF16, 'dgrad_lo', 0, 32, 32, 0, 1, 1, 0, 0, 0), (BF16, 'wgrad', 0, 0, 7, 0)],
         'smallest extent found for conv_igemm_kernel<bf16_t, 256, 32, FAST 2 (up-folded)> + conv_splitk_reduce_kernel (fwd)'),
    Case(F32X3, 1, 4, 4, 32, 32, 64, 3, 1, 1, 0, 64, 1, ('fwd', 'dgrad'),
         [(F32X3, 'fwd', 0, 64, 64, 0, 1, 0, 0, 0, 1), (F32X3, 'dgrad', 0, 64, 64, 0, 1, 0, 1, 0, 1)],
         'smallest extent found for conv_igemm_kernel<float, 64, 64, FAST 1, X3> + conv_splitk_reduce_kernel (dgrad)'),
    Case(F32X3, 1, 4, 4, 32, 32, 64, 3, 1, 1, 2, 64, 1, ('fwd', 'dgrad'),
         [(F32X3, 'fwd', 0, 64, 64, 3, 4, 0, 0, 0, 1), (F32X3, 'dgrad', 0, 256, 32, 0, 1, 0, 1, 0, 1), (F32X3, 'dgrad_lo', 0, 256, 32, 0, 1, 0, 1, 0, 1)],
         'smallest extent found for conv_igemm_kernel<float, 64, 64, FAST 2 (up-folded), X3> + conv_splitk_reduce_kernel (fwd)'),
    Case(BF16, 1, 4, 64, 32, 0, 16, 3, 1, 1, 2, 32, 0, ('fwd', 'dgrad', 'wgrad'),
         [(BF16, 'fwd', 5, 0, 0, 0, 1, 0, 0, 0, 0), (BF16, 'dgrad', 7, 0, 0, 0, 1, 0, 0, 1, 0), (BF16, 'wgrad', 0, 0, 7, 0)],
         'smallest extent found for conv_patch_kernel<bf16_t, 16, 32, false, 16, SUM2> (dgrad)'),
    Case(F32X3, 8, 128, 128, 8, 0, 96, 1, 2, 0, 0, 8, 0, ('fwd', 'dgrad', 'wgrad'),
         [(F32X3, 'fwd', 0, 128, 64, 0, 1, 1, 0, 0, 0), (F32X3, 'dgrad', 0, 256, 16, 2, 1, 0, 1, 0, 0), (F32X3, 'wgrad', 0, 0, 0, 32)],
         'smallest extent found for conv_igemm_kernel<float, 128, 64, SMALLC, X3> (fwd)'),
    Case(F32, 12, 64, 64, 32, 0, 96, 1, 2, 0, 0, 32, 0, ('fwd', 'dgrad', 'wgrad'),
         [(F32, 'fwd', 0, 64, 64, 0, 1, 0, 1, 0, 0), (F32, 'dgrad', 0, 256, 32, 2, 1, 0, 1, 0, 0), (F32, 'wgrad', 0, 0, 0, 32)],
         'smallest extent found for conv_igemm_kernel<float, 64, 64, FAST 1> (fwd)'),
    Case(BF16, 16, 12, 128, 64, 0, 96, 1, 2, 0, 0, 64, 0, ('fwd', 'dgrad', 'wgrad'),
         [(BF16, 'fwd', 0, 64, 32, 0, 1, 0, 1, 0, 0), (BF16, 'dgrad', 0, 64, 64, 0, 1, 1, 0, 0, 0), (BF16, 'wgrad', 0, 0, 0, 64)],
         'smallest extent found for conv_igemm_kernel<bf16_t, 64, 32, FAST 1> (fwd)'),
    Case(BF16, 16, 12, 128, 96, 0, 64, 1, 2, 0, 0, 96, 0, ('fwd', 'dgrad', 'wgrad'),
         [(BF16, 'fwd', 0, 32, 32, 0, 1, 1, 0, 0, 0), (BF16, 'dgrad', 0, 64, 32, 2, 1, 0, 1, 0, 0), (BF16, 'wgrad', 0, 0, 0, 64)],
         'smallest extent found for conv_igemm_kernel<bf16_t, 64, 32, FAST 1> par 2 (dgrad)'),
    Case(BF16, 12, 64, 64, 64, 0, 96, 1, 2, 0, 0, 64, 0, ('fwd', 'dgrad', 'wgrad'),
         [(BF16, 'fwd', 0, 64, 64, 0, 1, 0, 1, 0, 0), (BF16, 'dgrad', 0, 64, 64, 0, 1, 1, 0, 0, 0), (BF16, 'wgrad', 0, 0, 0, 64)],
         'smallest extent found for conv_igemm_kernel<bf16_t, 64, 64, FAST 1> (fwd)'),
    Case(F32, 3, 56, 72, 96, 0, 32, 3, 2, 1, 0, 96, 0, ('fwd', 'dgrad', 'wgrad'),
         [(F32, 'fwd', 0, 256, 32, 0, 1, 0, 1, 0, 0), (F32, 'dgrad', 0, 64, 64, 1, 4, 0, 1, 0, 0), (F32, 'wgrad', 0, 0, 0, 32)],
         'smallest extent found for conv_igemm_kernel<float, 64, 64, FAST 1> par 1 (dgrad)'),
    Case(BF16, 3, 56, 72, 256, 0, 3, 3, 1, 1, 2, 256, 0, ('dgrad', 'wgrad'),
         [(BF16, 'dgrad_lo', 0, 64, 32, 0, 1, 1, 0, 0, 0), (BF16, 'wgrad', 0, 0, 7, 0)],
         'smallest extent found for conv_igemm_kernel<bf16_t, 64, 32, SMALLC> (dgrad_lo)'),
    Case(BF16, 12, 8, 64, 96, 0, 64, 3, 2, 1, 0, 96, 0, ('fwd', 'dgrad', 'wgrad'),
         [(BF16, 'fwd', 0, 32, 32, 0, 1, 1, 0, 0, 0), (BF16, 'dgrad', 0, 64, 32, 1, 4, 0, 1, 0, 0), (BF16, 'wgrad', 0, 0, 0, 64)],
         'smallest extent found for conv_igemm_kernel<bf16_t, 64, 32, FAST 1> par 1 (dgrad)'),
    Case(F32X3, 8, 128, 128, 32, 0, 96, 1, 2, 0, 0, 32, 0, ('fwd', 'dgrad', 'wgrad'),
         [(F32X3, 'fwd', 0, 128, 64, 0, 1, 0, 1, 0, 0), (F32X3, 'dgrad', 0, 256, 32, 2, 1, 0, 1, 0, 0), (F32X3, 'wgrad', 0, 0, 0, 32)],
         'smallest extent found for conv_igemm_kernel<float, 128, 64, FAST 1, X3> (fwd)'),
    Case(BF16, 3, 56, 72, 512, 0, 3, 3, 1, 1, 2, 512, 0, ('dgrad', 'wgrad'),
         [(BF16, 'dgrad_lo', 0, 64, 64, 0, 1, 1, 0, 0, 0), (BF16, 'wgrad', 0, 0, 0, 32)],
         'smallest extent found for conv_igemm_kernel<bf16_t, 64, 64, SMALLC> (dgrad_lo)'),
    Case(BF16, 3, 56, 72, 96, 0, 64, 3, 2, 1, 0, 96, 0, ('fwd', 'dgrad', 'wgrad'),
         [(BF16, 'fwd', 0, 32, 32, 0, 1, 1, 0, 0, 0), (BF16, 'dgrad', 0, 64, 64, 1, 4, 0, 1, 0, 0), (BF16, 'wgrad', 0, 0, 0, 64)],
         'smallest extent found for conv_igemm_kernel<bf16_t, 64, 64, FAST 1> par 1 (dgrad)'),
    Case(F32, 16, 16, 128, 96, 0, 32, 3, 2, 1, 0, 96, 0, ('fwd', 'dgrad', 'wgrad'),
         [(F32, 'fwd', 0, 256, 32, 0, 1, 0, 1, 0, 0), (F32, 'dgrad', 0, 128, 64, 1, 4, 0, 1, 0, 0), (F32, 'wgrad', 0, 0, 0, 32)],
         'smallest extent found for conv_igemm_kernel<float, 128, 64, FAST 1> par 1 (dgrad)'),
    Case(F32X3, 16, 16, 128, 96, 0, 32, 3, 2, 1, 0, 96, 0, ('fwd', 'dgrad', 'wgrad'),
         [(F32X3, 'fwd', 0, 256, 32, 0, 1, 0, 1, 0, 0), (F32X3, 'dgrad', 0, 128, 64, 1, 4, 0, 1, 0, 0), (F32X3, 'wgrad', 0, 0, 0, 32)],
         'smallest extent found for conv_igemm_kernel<float, 128, 64, FAST 1, X3> par 1 (dgrad)'),
    Case(BF16, 12, 8, 64, 32, 64, 64, 3, 1, 1, 0, 96, 0, ('dgrad',),
         [(BF16, 'dgrad', 0, 64, 32, 0, 1, 0, 1, 0, 0)],
         'smallest extent found for conv_igemm_kernel<bf16_t, 64, 32, FAST 1> (dgrad)'),
    Case(BF16, 16, 128, 128, 64, 0, 3, 3, 1, 1, 2, 64, 0, ('dgrad',),
         [(BF16, 'dgrad_lo', 0, 128, 64, 0, 1, 1, 0, 0, 0)],
         'smallest extent found for conv_igemm_kernel<bf16_t, 128, 64, SMALLC> (dgrad_lo)'),
    Case(BF16, 16, 16, 128, 96, 0, 64, 3, 2, 1, 0, 96, 0, ('dgrad',),
         [(BF16, 'dgrad', 0, 128, 64, 1, 4, 0, 1, 0, 0)],
         'smallest extent found for conv_igemm_kernel<bf16_t, 128, 64, FAST 1> par 1 (dgrad)'),
    Case(F32, 3, 56, 72, 32, 32, 96, 3, 1, 1, 2, 64, 0, ('fwd',),
         [(F32, 'fwd', 0, 64, 64, 3, 4, 0, 0, 0, 0)],
         'smallest extent found for conv_igemm_kernel<float, 64, 64, FAST 2 (up-folded)> (fwd)'),
    Case(F32, 16, 16, 128, 8, 64, 32, 3, 1, 1, 0, 72, 0, ('dgrad',),
         [(F32, 'dgrad', 0, 128, 64, 0, 1, 0, 1, 0, 0)],
         'smallest extent found for conv_igemm_kernel<float, 128, 64, FAST 1> (dgrad)'),
    Case(BF16, 12, 8, 64, 64, 64, 96, 3, 1, 1, 2, 128, 0, ('fwd',),
         [(BF16, 'fwd', 0, 64, 32, 3, 4, 0, 0, 0, 0)],
         'smallest extent found for conv_igemm_kernel<bf16_t, 64, 32, FAST 2 (up-folded)> (fwd)'),
    Case(F32X3, 16, 16, 128, 8, 64, 32, 3, 1, 1, 0, 72, 0, ('dgrad',),
         [(F32X3, 'dgrad', 0, 128, 64, 0, 1, 0, 1, 0, 0)],
         'smallest extent found for conv_igemm_kernel<float, 128, 64, FAST 1, X3> (dgrad)'),
    Case(BF16, 16, 16, 128, 32, 0, 128, 3, 1, 1, 0, 32, 0, ('dgrad',),
         [(BF16, 'dgrad', 10, 0, 0, 0, 1, 0, 0, 0, 0)],
         'smallest extent found for conv_pres_kernel<128, 32, 4, 1, 1, 1> (one weight stage) (dgrad)'),
    Case(BF16, 16, 32, 32, 32, 0, 256, 3, 1, 1, 0, 32, 0, ('dgrad',),
         [(BF16, 'dgrad', 11, 0, 0, 0, 1, 0, 0, 0, 0)],
         'smallest extent found for conv_pres_kernel<256, 16, 2, 1, 2, 1> (one weight stage) (dgrad)'),
    Case(BF16, 8, 32, 32, 32, 0, 512, 3, 1, 1, 0, 32, 0, ('dgrad',),
         [(BF16, 'dgrad', 12, 0, 0, 0, 1, 0, 0, 0, 0)],
         'smallest extent found for conv_pres_kernel<512, 8, 1, 1, 4, 2> (one weight stage) (dgrad)'),
    Case(BF16, 16, 32, 32, 256, 0, 32, 3, 1, 1, 0, 256, 0, ('fwd',),
         [(BF16, 'fwd', 11, 0, 0, 0, 1, 0, 0, 0, 0)],
         'smallest extent found for conv_pres_kernel<256, 16, 2, 1, 2, 1> (fwd)'),
    Case(BF16, 8, 32, 32, 512, 0, 32, 3, 1, 1, 0, 512, 0, ('fwd',),
         [(BF16, 'fwd', 12, 0, 0, 0, 1, 0, 0, 0, 0)],
         'smallest extent found for conv_pres_kernel<512, 8, 1, 1, 4, 2> (fwd)'),
    Case(BF16, 3, 56, 72, 64, 64, 96, 3, 1, 1, 2, 128, 0, ('fwd',),
         [(BF16, 'fwd', 0, 64, 64, 3, 4, 0, 0, 0, 0)],
         'smallest extent found for conv_igemm_kernel<bf16_t, 64, 64, FAST 2 (up-folded)> (fwd)'),
    Case(F32, 12, 64, 64, 96, 0, 32, 3, 1, 1, 2, 96, 0, ('dgrad',),
         [(F32, 'dgrad_lo', 0, 64, 64, 0, 1, 0, 1, 0, 0)],
         'smallest extent found for conv_igemm_kernel<float, 64, 64, FAST 1> (dgrad_lo)'),
    Case(BF16, 3, 56, 72, 256, 0, 64, 3, 1, 1, 2, 256, 0, ('dgrad',),
         [(BF16, 'dgrad_lo', 0, 64, 32, 0, 1, 0, 1, 0, 0)],
         'smallest extent found for conv_igemm_kernel<bf16_t, 64, 32, FAST 1> (dgrad_lo)'),
    Case(F32, 16, 16, 128, 32, 32, 96, 3, 1, 1, 2, 64, 0, ('fwd',),
         [(F32, 'fwd', 0, 128, 64, 3, 4, 0, 0, 0, 0)],
         'smallest extent found for conv_igemm_kernel<float, 128, 64, FAST 2 (up-folded)> (fwd)'),
    Case(F32X3, 16, 16, 128, 32, 32, 96, 3, 1, 1, 2, 64, 0, ('fwd',),
         [(F32X3, 'fwd', 0, 128, 64, 3, 4, 0, 0, 0, 0)],
         'smallest extent found for conv_igemm_kernel<float, 128, 64, FAST 2 (up-folded), X3> (fwd)'),
    Case(BF16, 3, 56, 72, 512, 0, 64, 3, 1, 1, 2, 512, 0, ('dgrad',),
         [(BF16, 'dgrad_lo', 0, 64, 64, 0, 1, 0, 1, 0, 0)],
         'smallest extent found for conv_igemm_kernel<bf16_t, 64, 64, FAST 1> (dgrad_lo)'),
    Case(F32, 8, 128, 128, 96, 0, 32, 3, 1, 1, 2, 96, 0, ('dgrad',),
         [(F32, 'dgrad_lo', 0, 128, 64, 0, 1, 0, 1, 0, 0)],
         'smallest extent found for conv_igemm_kernel<float, 128, 64, FAST 1> (dgrad_lo)'),
    Case(BF16, 16, 16, 128, 64, 64, 96, 3, 1, 1, 2, 128, 0, ('fwd',),
         [(BF16, 'fwd', 0, 128, 64, 3, 4, 0, 0, 0, 0)],
         'smallest extent found for conv_igemm_kernel<bf16_t, 128, 64, FAST 2 (up-folded)> (fwd)'),
    Case(F32X3, 8, 128, 128, 96, 0, 32, 3, 1, 1, 2, 96, 0, ('dgrad',),
         [(F32X3, 'dgrad_lo', 0, 128, 64, 0, 1, 0, 1, 0, 0)],
         'smallest extent found for conv_igemm_kernel<float, 128, 64, FAST 1, X3> (dgrad_lo)'),
]


def launch_table():
    """the "what launches what" table of tests/test_gpu_conv_forms.py: form -> cases (python tests/conv_cases.py)"""
    by_form = {}
    for c in CASES:
        for f in case_forms(c):
            by_form.setdefault(f, []).append(case_id(c))
    lines = []
    for f in sorted(by_form, key=str):
        lines.append(f"{kernel_name(f)}\n    {f}\n    <- " + ", ".join(by_form[f]))
    return "\n".join(lines)


def kernel_name(f):
    """the kernel instantiation a form selects"""
    dt, name = f[0], f[1]
    t = {F32: "float", BF16: "bf16_t", F32X3: "float"}[dt]
    x3 = ", X3" if dt == F32X3 else ""
    if name == "wgrad":
        part, cls, patch, tile = f[2:]
        if patch == 0:
            k = "64, 64, 2, 2, 1" if tile == 64 else "32, 32, 1, 1, 4"
            mma = ", bf16 MFMA" if tile == 64 and dt != F32 else ""
            return f"conv_wgrad_kernel<{t}, {k}{mma}{', CLS' if cls else ''}> + wgrad_reduce_batch_kernel"
        if patch == 7:
            return "conv_wgrad_patch_bf16_kernel + wgrad_reduce_batch_kernel"
        if cls:
            return f"conv_wgrad_patch_cls_kernel<{t}, {'16' if patch == 1 else '32'}, 32, 16> + wgrad_reduce_batch_kernel"
        inst = {1: "16, 32, 3, 1, 16", 2: "16, 16, 3, 1, 16", 3: "32, 32, 3, 1, 16", 4: "32, 4, 7, 2, 16, 3",
                5: "32, 8, 7, 2, 16", 6: "32, 4, 7, 2, 16, 3"}[patch]
        return f"conv_wgrad_patch_kernel<{t}, {inst}> + wgrad_reduce_batch_kernel"
    if f[2] == "wino":
        return "conv_winograd_kernel"
    patch, bm, bn, par, nz, smallc, fast, sum2, sk = f[2:]
    if patch == 0:
        loader = "FAST 2 (up-folded)" if par == 3 else "SMALLC" if smallc else "FAST 1" if fast else "FAST 0"
        return f"conv_igemm_kernel<{t}, {bm}, {bn}, {loader}{x3}>" + (f" par {par}" if par in (1, 2) else "") + \
            (" + conv_splitk_reduce_kernel" if sk else "")
    names = {1: "conv_patch_kernel<float, 16 | 4, 16>", 2: "conv_stem_kernel", 3: "conv_patch_kernel<bf16_t, 16, 16>",
             4: "conv_patch_kernel<bf16_t, 32, 32>", 5: "conv_patch_kernel<bf16_t, 32, 16, UP>",
             6: "conv_patch_kernel<bf16_t, 16, 16, false, 8>", 7: "conv_patch_kernel<bf16_t, 16, 32, false, 16, SUM2>",
             8: "conv_stem_bf16_kernel", 9: "conv_pres_kernel<64, 64, 2, 2, 1, 2>", 10: "conv_pres_kernel<128, 32, 4, 1, 1, 1>",
             11: "conv_pres_kernel<256, 16, 2, 1, 2, 1>", 12: "conv_pres_kernel<512, 8, 1, 1, 4, 2>"}
    return names[patch] + (" (one weight stage)" if patch >= 9 and name != "fwd" else "")


if __name__ == "__main__":
    print(launch_table())
