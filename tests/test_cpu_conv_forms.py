"""CPU: the convolution operator cases of tests/conv_cases.py against the planner and against their own bound (host only).

* the bound admits the reference alone: torch's CPU fp32 evaluation (rounded once to bf16 in bf16 cases) stays inside
  the derived per-element bound in all three directions;
* the gate is sensitive: faults of computed size planted into the float64 reference -- a dropped 16-channel tap at the
  first, the last and an interior output pixel, an output pixel replaced by its neighbour, a statistics row counted
  twice -- are flagged wherever they exceed twice the bound, and every case has at least one of each kind;
* the 4e-3 rel-L2 gate of the bf16 conv_pres case does NOT see a whole wrong corner pixel: the hole the bound closes;
* form coverage: every kernel form the whole-network plans take (d3f_unet_conv_layer) is reached by an operator case
  (d3f_conv_layer_plan), and every case still selects the forms it is there for;
* every persistent weight-gradient kernel has a case whose workgroups take unequal shares;
* Winograd F(2x2, 3x3): the kernel's path restated in torch fp32 stays inside the derived bound of conv_cases.py for every
  Winograd case, on N(0, 1) inputs and on inputs shifted by + 8; the same path with V rounded to bf16 violates it; on
  operands in {-1, 0, 1} the fp32 path is exact;
* exact operands: every case's {-1, 0, 1} data set keeps every fp32 partial sum below 2^24, the condition under which
  the exact pass of tests/test_gpu_conv_forms.py may demand equality.
"""
import ctypes as C

import pytest
import torch

import conv_cases as cc
import packed_restatement as pr
from conv_cases import ALL, BF16, CASES, F32, F32X3
from denoising_diffusion_deep_fake_amd import _lib

CPU_MACS = 2e8  # cases above this many multiply-adds skip the CPU evaluations here (the GPU test runs them all)
SMALL = [c for c in CASES if cc.macs(c) <= CPU_MACS and c.entry == "conv"]
WINO = [c for c in CASES if c.entry == "winograd"]
PRES = next(c for c in CASES if c.dtype == BF16 and (c.B, c.H, c.W, c.C0, c.Cout) == (12, 64, 64, 64, 64))

# What the single-operator entry points cannot express.  None of it selects another kernel instantiation -- a form is
# the tuple of kernel-selecting plan fields, and these are run-time branches of the same instantiations -- so no form
# is exempt from test_every_network_form_has_an_operator_case; the list records which PATHS of those kernels only the
# whole-network tests walk (tests/test_gpu_unet.py, test_gpu_bf16.py, test_gpu_pair.py, test_gpu_parity_layers.py).
NETWORK_ONLY_PATHS = {
    "eval-fused epilogue": "d3f_conv_forward has no scale / shift / residual arguments (CONV_EVAL_FUSED); the head's "
                           "bias + NCHW epilogue (CONV_HEAD_NCHW) rides the same switch",
    "BatchNorm partial sums in a data-gradient epilogue": "d3f_conv_backward_data has no bn_y / bn_coef / bn_partial",
    "two networks in one launch": "no single-operator entry takes a second network's pointers (grid.z = nets)",
}
EXEMPT_FORMS = set()


def rounded(x32, dtype):
    return x32.bfloat16().double() if dtype == BF16 else x32.double()


@pytest.mark.parametrize("case", SMALL, ids=cc.case_id)
def test_bound_admits_the_cpu_fp32_evaluation(case):
    c = case
    plan = cc.plan_of(c)
    data = cc.make_data(c)
    ref = cc.reference(c, data)
    x0, x1, w, dy = [None if t is None else t.float() for t in data]
    xin = cc.conv_input(c, x0, x1)
    if "fwd" in c.dirs:
        y32 = torch.nn.functional.conv2d(xin, w, None, c.stride, c.pad)
        bad, ratio = cc.violations(rounded(y32, c.dtype), ref["y"], cc.fwd_bound(c, plan, ref["y"], ref["y_mag"]))
        assert bad == 0 and ratio <= 1.0, ("fwd", bad, ratio)
    if "dgrad" in c.dirs:
        dx32 = torch.nn.grad.conv2d_input(xin.shape, w, dy, c.stride, c.pad)
        c0 = x0.shape[1]
        if c.up:
            low32 = cc.sum2x2(dx32[:, :c0])
            bound = cc.dgrad_low_bound(c, plan, ref["dx"][:, :c0], ref["dx_mag"][:, :c0])
            bad, ratio = cc.violations(rounded(low32, c.dtype), cc.sum2x2(ref["dx"][:, :c0]), bound)
            assert bad == 0, ("dgrad low", bad, ratio)
            lo = c0
        else:
            lo = 0
        if lo < dx32.shape[1]:
            bound = cc.dgrad_full_bound(c, ref["dx"][:, lo:], ref["dx_mag"][:, lo:])
            bad, ratio = cc.violations(rounded(dx32[:, lo:], c.dtype), ref["dx"][:, lo:], bound)
            assert bad == 0, ("dgrad", bad, ratio)
    if "wgrad" in c.dirs:
        dw32 = torch.nn.grad.conv2d_weight(xin, w.shape, dy, c.stride, c.pad)
        bad, ratio = cc.violations(dw32.double(), ref["dw"], cc.wgrad_bound(c, plan, ref["dw_mag"]))
        assert bad == 0, ("wgrad", bad, ratio)


# ---- sensitivity ---------------------------------------------------------------------------------------------------------
def plant_faults(c, plan, data, ref):
    """[(kind, planted tensor name, index, planted value, size)]: faults of computed size in y [B, Cout, Ho, Wo]"""
    x0, x1, w, _ = data
    xin = cc.conv_input(c, x0, x1)
    y = ref["y"]
    B, Co, Ho, Wo = y.shape
    faults = []
    kc = c.k // 2  # the centre tap reads input pixel (oy * stride + kc - pad, ..): inside the image for every case here
    pixels = [(0, 0, 0), (B - 1, Ho - 1, Wo - 1), (B // 2, Ho // 2, max(Wo // 2 - 1, 0))]
    for (b, oy, ox) in pixels:
        iy, ix = oy * c.stride + kc - c.pad, ox * c.stride + kc - c.pad
        assert 0 <= iy < xin.shape[2] and 0 <= ix < xin.shape[3]
        for g0 in range(0, xin.shape[1], 16):  # one 16-channel group of the centre tap, every filter
            part = (w[:, g0:g0 + 16, kc, kc] * xin[b, g0:g0 + 16, iy, ix]).sum(1)  # [Cout]
            for co in range(Co):
                faults.append(("tap", (b, co, oy, ox), float(y[b, co, oy, ox] - part[co]), abs(float(part[co]))))
        nx = ox + 1 if ox + 1 < Wo else ox - 1
        for co in range(Co):
            faults.append(("neighbour", (b, co, oy, ox), float(y[b, co, oy, nx]),
                           abs(float(y[b, co, oy, nx] - y[b, co, oy, ox]))))
    return faults


# The statistics bounds add the worst-case accumulation bound of EVERY pixel of a channel (n * 2^-24 * magnitude, the
# magnitude growing like sqrt(n)) and rows * 2^-24 * sum |y|, so one row counted twice -- a change of |y| ~ 1 -- shows
# in the sums of a small tensor only.  The cases are those with n^1.5 * pixels <= 4e6 (a bound of ~0.15 on the sum)
# outside bf16 storage with folded weights, whose pre-summed weights cost 2^-8 of the magnitude at every pixel.  The
# per-element plants show at any size.
def _stats_can_show(c):
    ho, wo = cc.out_hw(c)
    n = c.k * c.k * (c.C0 + c.C1)
    return n ** 1.5 * c.B * ho * wo <= 4e6 and not (c.dtype == BF16 and cc.plan_of(c).upfold)


SENSITIVE = [c for c in SMALL if "fwd" in c.dirs and _stats_can_show(c)]


@pytest.mark.parametrize("case", SENSITIVE, ids=cc.case_id)
def test_planted_faults_are_flagged(case):
    c = case
    plan = cc.plan_of(c)
    data = cc.make_data(c)
    ref = cc.reference(c, data, dirs=("fwd",))
    y = ref["y"]
    bound = cc.fwd_bound(c, plan, y, ref["y_mag"])
    kept = {"tap": 0, "neighbour": 0, "stats": 0}
    for kind, idx, value, size in plant_faults(c, plan, data, ref):
        if not size > 2.0 * float(bound[idx]):
            continue
        kept[kind] += 1
        got = y.clone()
        got[idx] = value
        bad, _ = cc.violations(got[idx].reshape(1), y[idx].reshape(1), bound[idx].reshape(1))
        assert bad == 1, (kind, idx, size, float(bound[idx]))
    # one statistics row (pixel) counted twice: the sums move by y and y * y of that pixel
    s1, s2, b1, b2 = cc.stats_reference(c, plan, y, ref["y_mag"])
    B, Co, Ho, Wo = y.shape
    for (b, oy, ox) in ((0, 0, 0), (B - 1, Ho - 1, Wo - 1), (B // 2, Ho // 2, Wo // 2)):
        row = y[b, :, oy, ox]
        for co in range(Co):
            if abs(float(row[co])) > 2.0 * float(b1[co]):
                kept["stats"] += 1
                assert not abs(float(s1[co] + row[co]) - float(s1[co])) <= float(b1[co])
            if float(row[co]) ** 2 > 2.0 * float(b2[co]):
                assert not abs(float(s2[co] + row[co] ** 2) - float(s2[co])) <= float(b2[co])
    assert all(n > 0 for n in kept.values()), kept


def test_the_rel_l2_gate_misses_a_whole_wrong_corner_pixel():
    """bf16 conv_pres case (12, 64, 64, 64 -> 64), 3.1 M outputs: the corner pixel computed without its centre tap (all
    64 input channels: a halo or tap bug at the image corner, wrong in all 64 filters) passes the aggregate 4e-3 gate of
    tests/test_gpu_bf16.py on top of the one bf16 rounding per output, and nearly every one of those 64 elements fails
    the per-element bound"""
    c = PRES
    plan = cc.plan_of(c)
    data = cc.make_data(c)
    ref = cc.reference(c, data, dirs=("fwd",))
    y = ref["y"]
    got = y.bfloat16().double()  # a faultless kernel: one rounding per output
    clean = cc.rel_l2(got, y)
    x0, _, w, _ = data
    tap = (w[:, :, 1, 1] * x0[0, :, 0, 0]).sum(1)  # [Cout]
    got[0, :, 0, 0] = (y[0, :, 0, 0] - tap).bfloat16().double()
    assert clean < cc.rel_l2(got, y) < cc.REL_L2_BF16, "the aggregate gate does not flag the wrong pixel"
    bound = cc.fwd_bound(c, plan, y, ref["y_mag"])
    wrong = (got[0, :, 0, 0] - y[0, :, 0, 0]).abs() > bound[0, :, 0, 0]
    assert int(wrong.sum()) >= 56, int(wrong.sum())  # (a tap contribution near zero is inside the bound either way)
    bad, _ = cc.violations(got, y, bound)
    assert bad == int(wrong.sum())


# ---- forms ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=cc.case_id)
def test_case_selects_the_forms_it_is_there_for(case):
    assert cc.case_forms(case) == case.forms, (cc.case_forms(case), case.forms)
    plan = cc.plan_of(case)
    if "fwd" in case.dirs:
        assert plan.fwd.planned and (case.entry != "winograd" or plan.wino_rows > 0)
    if "dgrad" in case.dirs:
        assert plan.dgrad.planned or plan.dgrad_lo.planned


def test_every_network_form_has_an_operator_case():
    reached = {f for c in CASES for f in cc.case_forms(c)}
    missing = {}
    for net in cc.NETWORK_PLANS:
        layers = cc.network_layers(*net)
        assert len(layers) == 47
        for desc, plan in layers:
            for d in ALL:
                for f in cc.plan_forms(net[0], plan)[d]:
                    if f not in reached and f not in EXEMPT_FORMS:
                        missing.setdefault(f, (net, desc))
    assert not missing, missing
    assert not EXEMPT_FORMS and len(NETWORK_ONLY_PATHS) == 3


def test_unet_conv_layer_reports_the_plan_of_its_own_description():
    """d3f_unet_conv_layer against d3f_conv_layer_plan of the description it returns (single-network plans: plan_nets 1,
    the engine's split-K workspace and 2x2-summed request): the same fields, except the head's forward, which the engine
    plans with the bias + NCHW epilogue (Cout = 3 has no operator forward)"""
    L = _lib.lib()
    for net in cc.NETWORK_PLANS:
        if net[4] != 1:
            continue
        layers = cc.network_layers(*net)
        for i, (desc, plan) in enumerate(layers):
            d, q = _lib.ConvDesc(*desc), _lib.ConvPlan()
            _lib.check(L.d3f_conv_layer_plan(net[0], C.byref(d), 1, C.byref(q)))
            head = i == len(layers) - 1
            names = (() if i == 0 else ("dgrad", "dgrad_lo")) + (() if head else ("fwd",))
            for name in names:
                assert bytes(getattr(plan, name)) == bytes(getattr(q, name)), (net, i, name)
            # (the stem takes no data gradient in the network)
            assert bool(plan.dgrad.planned or plan.dgrad_lo.planned) == (i > 0)
            assert (plan.upfold, plan.parity, plan.wgrad_parts) == (q.upfold, q.parity, q.wgrad_parts)
            assert bytes(plan.wgrad) == bytes(q.wgrad), (net, i)
            if not head:
                assert (plan.wino, plan.wino_rows) == (q.wino, q.wino_rows)
    h = C.c_void_p()
    _lib.check(L.d3f_unet_create(b"resnet18", 3, 3, 1, 64, 64, F32, C.byref(h)))
    try:
        d, p = _lib.ConvDesc(), _lib.ConvPlan()
        n = L.d3f_unet_num_conv_layers(h)
        assert n > 0 and L.d3f_unet_conv_layer(h, n, C.byref(d), C.byref(p)) != 0
        assert L.d3f_unet_conv_layer(h, -1, C.byref(d), C.byref(p)) != 0 and L.d3f_unet_num_conv_layers(None) == -1
    finally:
        L.d3f_unet_destroy(h)
    bad = _lib.ConvDesc(2, 16, 16, 6, 0, 0, 8, 3, 3, 1, 1, 6)
    assert L.d3f_conv_layer_plan(F32, C.byref(bad), 0, C.byref(p)) != 0 and b"multiples of 4" in L.d3f_last_error()


def test_network_plan_counts_agree_with_the_per_layer_plans():
    """d3f_unet_plan_counts (pinned in tests/test_cpu_lib.py) counts what d3f_unet_conv_layer reports"""
    L = _lib.lib()
    for net in cc.NETWORK_PLANS:
        dtype, B, H, W, nets = net
        h = C.c_void_p()
        _lib.check(L.d3f_unet_create_nets(b"resnet34", 3, 3, B, H, W, dtype, nets, nets, C.byref(h)))
        f, d, w = (C.c_int32 * 16)(), (C.c_int32 * 16)(), (C.c_int32 * 16)()
        try:
            _lib.check(L.d3f_unet_plan_counts(h, f, d, w))
        finally:
            L.d3f_unet_destroy(h)
        mine = [[0] * 16 for _ in range(3)]
        for _, p in cc.network_layers(*net):
            mine[0][15 if p.wino else p.fwd.patch] += 1
            for q in (p.dgrad, p.dgrad_lo):
                if q.planned:
                    mine[1][q.patch] += 1
            for i in range(p.wgrad_parts):
                mine[2][p.wgrad[i].patch] += 1
        assert mine == [list(f), list(d), list(w)], net


# ---- ragged persistent work ------------------------------------------------------------------------------------------------
def test_every_persistent_weight_gradient_kernel_has_a_case_with_unequal_shares():
    """patch variants 1, 2, 3 (1 also in class form), the stem's 4 and 5 / 6, the native-bf16 variant 7: more spatial
    tiles than workgroups and not a whole multiple, so the grid-stride loops run a ragged last round; the tap-parallel
    kernel: more 32-pixel chunks than slabs and a short last slab.  Near the threshold, not at workload size."""
    seen = {}
    for c in CASES:
        if not c.ragged:
            continue
        p = cc.plan_of(c)
        for i in range(p.wgrad_parts):
            w = p.wgrad[i]
            if c.ragged == "patch":
                assert w.patch > 0 and w.chunks_per_split == 0 and w.tile == 0
                shares = [w.tiles // w.splits + (1 if x < w.tiles % w.splits else 0) for x in range(w.splits)]
                assert w.tiles > w.splits and w.tiles % w.splits != 0 and max(shares) == min(shares) + 1 >= 2
                assert w.tiles <= 2 * 512, "near the threshold"
            else:
                assert w.patch == 0 and w.tile in (32, 64)
                last = w.tiles - (w.splits - 1) * w.chunks_per_split
                assert w.tiles > w.splits > 1 and 0 < last < w.chunks_per_split
            seen.setdefault((w.patch, w.cls), cc.case_id(c))
    want = {(1, 0), (1, 1), (2, 0), (3, 0), (4, 0), (7, 0), (0, 0)}
    assert want <= set(seen) and ((5, 0) in seen or (6, 0) in seen), seen


# ---- Winograd F(2x2, 3x3) --------------------------------------------------------------------------------------------------
def winograd_fp32(x, w, v_bf16=False):
    """conv_winograd_kernel restated in torch fp32, operation for operation: 4 x 4 tiles at stride 2 on the zero-padded
    input; tr_col then tr_row; the filter transform of winograd_pack_kernel; per position one fused multiply-add per
    channel into the fp32 accumulator (the product exact in float64, one rounding of the sum), in the kernel's channel
    order -- chunk of 16, half s2, element e, the MFMA's pair (8 s2 + e, 8 s2 + 4 + e); (a + b) + c down the rows of
    positions, then along the columns.  v_bf16: V rounded to bf16, the planted fault."""
    x, w = x.float(), w.float()
    (B, C, H, W), K = x.shape, w.shape[0]
    d = cc.winograd_tiles(x)                                            # [B, C, 4, 4, Ty, Tx]
    t = [[None] * 4 for _ in range(4)]
    for j in range(4):                                                  # tr_col: B^T d
        d0, d1, d2, d3 = (d[:, :, a, j] for a in range(4))
        t[0][j], t[1][j], t[2][j], t[3][j] = d0 - d2, d1 + d2, d2 - d1, d1 - d3
    v = []
    for i in range(4):                                                  # tr_row: (B^T d) B, positions 4 i .. 4 i + 3
        v += [t[i][0] - t[i][2], t[i][1] + t[i][2], t[i][2] - t[i][1], t[i][1] - t[i][3]]
    v = torch.stack(v, 2)                                               # [B, C, 16, Ty, Tx]
    if v_bf16:
        v = v.bfloat16().float()
    u = pr.winograd_filter_fp32(w).reshape(K, C, 16)
    acc = torch.zeros(B, K, 16, H // 2, W // 2)
    for ch in range(C // 16):
        for s2 in range(2):
            for e in range(4):
                for fq in range(2):
                    ci = 16 * ch + 8 * s2 + 4 * fq + e
                    acc = (acc.double() + u[:, ci].double()[None, :, :, None, None] * v[:, ci].double()[:, None]).float()
    a = [acc[:, :, q] for q in range(16)]
    t0 = [(a[j] + a[4 + j]) + a[8 + j] for j in range(4)]
    t1 = [(a[4 + j] - a[8 + j]) - a[12 + j] for j in range(4)]
    o00, o01 = (t0[0] + t0[1]) + t0[2], (t0[1] - t0[2]) - t0[3]
    o10, o11 = (t1[0] + t1[1]) + t1[2], (t1[1] - t1[2]) - t1[3]
    y = torch.stack([torch.stack([o00, o01], -1), torch.stack([o10, o11], -1)], 3)   # [B, K, Ty, 2, Tx, 2]
    return y.reshape(B, K, H, W)


@pytest.mark.parametrize("shift", [0.0, 8.0], ids=["N01", "N01+8"])
@pytest.mark.parametrize("case", WINO, ids=cc.case_id)
def test_winograd_bound_admits_the_fp32_restatement_and_flags_a_bf16_V(case, shift):
    """N(0, 1) inputs, and the same inputs shifted by + 8, where B^T d B cancels the offset: Ymag follows |d| and the
    bound with it.  The same path with V rounded to bf16 (2^-9 per term against (C + 10) * 2^-24) must violate it."""
    c = case
    x0, _, w, _ = cc.make_data(c)
    x = (x0 + shift).float().double()
    ref = torch.nn.functional.conv2d(x, w, None, 1, 1)
    direct_mag = torch.nn.functional.conv2d(x.abs(), w.abs(), None, 1, 1)
    mag = cc.winograd_eval(x, w, absolute=True)
    assert bool(((cc.winograd_eval(x, w) - ref).abs() <= 64 * 2.0 ** -53 * mag).all()), "float64 Winograd == the convolution"
    assert bool((mag >= direct_mag * (1 - 1e-12)).all())
    bound = cc.wino_acc_bound(c, mag)
    assert cc.wino_roundings(c) == c.C0 + 10
    got = winograd_fp32(x, w)
    bad, ratio = cc.violations(got, ref, bound)
    print(f"error/bound winograd fp32 restatement {cc.case_id(c)} shift {shift}: {ratio:.4f}; "
          f"Ymag / direct magnitude {float(mag.sum() / direct_mag.sum()):.2f}")
    assert bad == 0, (bad, ratio)
    bad16, ratio16 = cc.violations(winograd_fp32(x, w, v_bf16=True), ref, bound)
    assert bad16 > ref.numel() // 2 and ratio16 > 16, (bad16, ratio16)
    if shift:
        return
    # the statistics and the eval epilogue of the same fp32 values, under their derived bounds
    plan = cc.plan_of(c)
    s1, s2, b1, b2 = cc.stats_reference(c, plan, ref, None, wino=True, acc=bound)
    assert cc.stat_row_pixels(plan.fwd, True) == 256
    assert cc.violations(got.sum((0, 2, 3)), s1, b1)[0] == 0 and cc.violations((got * got).sum((0, 2, 3)), s2, b2)[0] == 0
    g = torch.Generator().manual_seed(5)
    sc, sf = torch.rand(c.Cout, generator=g) + 0.5, torch.randn(c.Cout, generator=g) * 0.3
    res = torch.randn(ref.shape, generator=g)
    for with_res in (False, True):
        for relu in (False, True):
            v32 = got * sc.view(1, -1, 1, 1) + sf.view(1, -1, 1, 1)
            v32 = v32 + res if with_res else v32
            v32 = v32.clamp_min(0) if relu else v32
            want, bnd = cc.wino_eval_reference(ref, bound, sc, sf, res.double() if with_res else None, relu)
            assert cc.violations(v32, want, bnd)[0] == 0, (with_res, relu)
            # a dropped shift is outside it (|shift| ~ 0.3 against ~1e-5)
            assert cc.violations(v32 - sf.view(1, -1, 1, 1) * (v32 > 0), want, bnd)[0] > want.numel() // 8


@pytest.mark.parametrize("case", WINO, ids=cc.case_id)
def test_winograd_in_fp32_is_exact_on_exact_operands(case):
    x0, _, w, _ = cc.make_exact_data(case)
    ref = torch.nn.functional.conv2d(x0, w, None, 1, 1)
    assert torch.equal(winograd_fp32(x0, w).double(), ref)
    assert torch.equal(cc.winograd_eval(x0, w), ref)


def test_the_winograd_cases_end_in_both_V_buffers():
    """chunk c is contracted from V[c & 1]: the table has a case that ends in V[1] (an even chunk count) and cases that end
    in V[0]; one with a single chunk (nothing double-buffered), one with two filter blocks and several workgroups"""
    chunks = sorted(c.C0 // 16 for c in WINO)
    assert 1 in chunks and any(n % 2 == 0 for n in chunks) and any(n % 2 == 1 and n > 1 for n in chunks)
    assert any(c.Cout > 64 and c.B * (c.H // 16) * (c.W // 16) > 1 for c in WINO)
    assert all(16 <= c.H <= 48 and 16 <= c.W <= 48 for c in WINO)


# ---- exact operands --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=cc.case_id)
def test_exact_operands_keep_every_fp32_sum_exact(case):
    """the conditions under which the exact pass of tests/test_gpu_conv_forms.py may demand equality: every operand in
    {-1, 0, 1}, and every partial sum an fp32 contraction or statistics row can form stays below 2^24 -- B * Ho * Wo *
    max|x dy| for the weight gradient, the tap and channel count for the others, stat_row_pixels * max(y^2) for a
    statistics row.  (The forward result is evaluated in fp32 here: exact once the first condition holds.)"""
    c = case
    plan = cc.plan_of(c)
    data = cc.make_exact_data(c)
    for t in data:
        assert t is None or (bool(((t == 0) | (t.abs() == 1)).all()) and len(t.unique()) == 3)
    assert torch.equal(data[0], cc.make_exact_data(c)[0]), "deterministic"
    first = cc.exact_conditions(c, plan, data)
    assert first and all(v < 2 ** 24 for v in first.values()), first
    y = None
    if "fwd" in c.dirs:
        x0, x1, w, _ = data
        y = torch.nn.functional.conv2d(cc.conv_input(c, x0, x1).float(), w.float(), None, c.stride, c.pad).double()
        if cc.macs(c) <= CPU_MACS:
            assert torch.equal(y, cc.reference(c, data, dirs=("fwd",), mags=False)["y"])
    cond = cc.exact_conditions(c, plan, data, y)
    assert ("statistics row" in cond) == ("fwd" in c.dirs)
    assert all(v < 2 ** 24 for v in cond.values()), cond


def test_f32x3_term_stays_under_the_fp32_bound_with_four_more_roundings():
    for c in CASES:
        ho, wo = cc.out_hw(c)
        for n in (c.k * c.k * (c.C0 + c.C1), cc.dgrad_n(c), 4 * cc.dgrad_n(c), c.B * ho * wo):
            assert cc.acc_roundings(F32X3, n) <= n + 4
            assert cc.acc_roundings(F32, n) == cc.acc_roundings(BF16, n) == n
    assert cc.acc_roundings(F32X3, 8) == 12 and cc.acc_roundings(F32X3, 144) == 54 + cc.X3_DROPPED
