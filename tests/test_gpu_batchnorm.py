"""GPU: every BatchNorm layer form at operator level against float64.

One layer is a description (d3f_bn_desc) that bn_layer_plan turns into the fused or the split form; a pass is one call
(d3f_bn_layer_forward / d3f_bn_layer_backward), the same two calls the network makes.  The test supplies the partial
rows itself (per-chunk float64 sums of ragged row chunks, rounded once to fp32), so the BatchNorm kernels are separated
from the conv epilogues and every expected value is computable:

* coefficients (mean, invstd, scale, shift, running statistics; dgamma, dbeta, k1, k2 when the backward rows are
  supplied): the kernel's formula in float64 on the SAME fp32 rows, rounded to fp32 -- at most 1 ulp (k0, an fp32
  product of gamma and the stored invstd: 2 ulp; shift = beta - mean * scale cancels: 1 ulp of |beta| + |mean * scale|);
* streamed tensors, whole tensor: torch.nn.functional.batch_norm + residual + ReLU in float64 with autograd, the ReLU
  mask pinned to the HIP run's own a > 0 -- rel-L2 1e-5 (a), 2e-5 (dy, dgamma, dbeta), dres exact; bf16 storage: 4e-3;
* streamed tensors, element by element: the kernel's formula in float64 on the fp32 coefficient rows the HIP pass
  wrote (themselves held to 1 ulp above).  The kernels then do a fixed number n of fp32 roundings per element, so
  |out - ref| <= n * 2^-24 * (sum of the absolute values of the terms); n is counted at A_ROUNDINGS / DY_ROUNDINGS.
  bf16 storage adds one rounding of the result (2^-8 relative);
* with bn_bwd_reduce producing the partial sums (fused_rows = 0) dgamma / dbeta / dy carry fp32 summation error in an
  order the test does not fix: measured per channel against the CPU-fp32 torch result's own distance from float64,
  factor NOISE = 4 over it, floor 2e-6 (dgamma / dbeta relative to the sum of the absolute values of their terms).

Every output buffer sits between two guard bands of at least 64 rows filled with a sentinel that must survive; the
statistics / partial buffers carry NaN behind the last row the description names and in the columns C..Cpad.

What launches what (every kernel of batchnorm.hip except bn_eval_coeff_all_kernel):

| kernel                                   | reached by                                                              |
|------------------------------------------|-------------------------------------------------------------------------|
| bn_finalize_kernel, bn_apply_kernel<T>   | forward matrix (split), apply = 0, shapes (C = 16), 1025 partial rows   |
| bn_finalize_apply_kernel<T, false>       | forward matrix (fused, no residual), slab_reduce rows, mask threshold   |
| bn_finalize_apply_kernel<T, true>        | forward matrix (fused, residual tensor / layer), shapes, downsample pair|
| bn_bwd_reduce_kernel<T>                  | backward matrix (partials from the reduce), all three masks             |
| bn_bwd_finalize_kernel, bn_bwd_apply<T>  | backward matrix (split), shapes (C = 16), 1025 partial rows             |
| bn_bwd_finalize_apply<T, false, false>   | backward matrix (fused; mask none / from y; dres none / write)          |
| bn_bwd_finalize_apply<T, false, true>    | backward matrix (fused; mask none / from y; dres accumulate)            |
| bn_bwd_finalize_apply<T, true, false>    | backward matrix (fused; mask from a; dres none / write), shapes         |
| bn_bwd_finalize_apply<T, true, true>     | backward matrix (fused; mask from a; dres accumulate)                   |
T = float and bf16 everywhere; res 0 / 1 / 2, mask 0 / 1 / 2, dres_acc 0 / 1, apply 0 / 1 and both partial-sum sources
(bn_bwd_reduce, supplied rows) each appear in the matrices below, in both dtypes and both forms.

Combinations the matrices leave out because the description forbids them: none in the forward matrix; in the backward
matrix the forward pass that goes with a mask follows from it (mask none: no ReLU, residual tensor; from y: ReLU, no
residual -- a mask recomputed from y alone is only the activation's mask without a residual; from a: ReLU, residual
tensor), so {mask} x {ReLU, residual} is not a free product.
"""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from util import SENTINEL, Guarded, rel_l2

pytestmark = pytest.mark.gpu

F32, BF16 = 0, 1
NOISE = 4.0          # the project's factor over the CPU-fp32 reference's own distance from float64
FLOOR = 2e-6
GUARD_ROWS = 64
EPS = float(np.float32(1e-5))       # the kernels' constants are floats widened to double
MOMENTUM = float(np.float32(0.1))
U24 = 2.0 ** -24
# fp32 roundings per element of a = relu?(y * scale + shift [+ residual]), counted in bn_apply_kernel /
# bn_finalize_apply_kernel: the product, the sum; + a residual tensor: one more sum; + another layer's y: its product,
# its sum and the sum of the two branches
A_ROUNDINGS = {0: 2, 1: 3, 2: 5}
# dy = k0 * (dz - k1 - xhat * k2), xhat = (y - mean) * invstd (bn_bwd_apply_kernel / bn_bwd_finalize_apply_kernel): the
# difference and the product of xhat, xhat * k2, dz - k1, the second difference, the product with k0
DY_ROUNDINGS = 6
RATIOS = {}
DEV = "cuda"


@pytest.fixture(scope="module")
def ops():
    from denoising_diffusion_deep_fake_amd import ops as m
    return m


def tdt(dt):
    return torch.bfloat16 if dt == BF16 else torch.float32


def stored(x64, dt):
    """what the storage dtype keeps of a float64 tensor, as float64"""
    return x64.to(tdt(dt)).double()


def chunk_ids(rows, n, rng):
    """rows split into n contiguous ragged chunks (more chunks than rows: the surplus stays empty)"""
    if n <= rows:
        cuts = np.sort(rng.choice(np.arange(1, rows), n - 1, replace=False)) if n > 1 else np.zeros(0, dtype=np.int64)
        lengths = np.diff(np.concatenate([[0], cuts, [rows]]))
    else:
        lengths = np.concatenate([np.ones(rows, dtype=np.int64), np.zeros(n - rows, dtype=np.int64)])
    return torch.from_numpy(np.repeat(np.arange(n), lengths).astype(np.int64))


def chunk_sums(ids, n, *cols):
    """per-chunk float64 sums of each [rows, C] tensor, rounded once to fp32: [n, C, len(cols)]"""
    out = []
    for x in cols:
        out.append(torch.zeros(n, x.shape[1], dtype=torch.float64).index_add_(0, ids, x).float())
    return torch.stack(out, dim=2).contiguous()


def within_ulps(actual, expected64, n):
    """|actual - fp32(expected)| <= n ulp of fp32(expected), element by element"""
    e = expected64.float().numpy()
    d = np.abs(actual.double().numpy() - e.astype(np.float64))
    return bool((d <= n * np.spacing(np.abs(e)).astype(np.float64)).all())


def ulp_of(x64):
    return torch.from_numpy(np.spacing(np.abs(x64.float().numpy())).astype(np.float64))


def fwd_coef_ref(stats, Cn, N, gamma, beta, rm=None, rv=None):
    """bn_fwd_coef in float64 on the fp32 rows [n, Cpad, 2]"""
    s1 = stats[:, :Cn, 0].double().sum(0)
    s2 = stats[:, :Cn, 1].double().sum(0)
    mean = s1 / N
    var = (s2 / N - mean * mean).clamp_min(0.0)
    invstd = 1.0 / torch.sqrt(var + EPS)
    g = gamma.double()
    r = dict(mean=mean, invstd=invstd, scale=g * invstd, shift=beta.double() - mean * g * invstd, var=var)
    if rm is not None:
        unbiased = var * N / (N - 1) if N > 1 else var
        r["rm"] = (1.0 - MOMENTUM) * rm.double() + MOMENTUM * mean
        r["rv"] = (1.0 - MOMENTUM) * rv.double() + MOMENTUM * unbiased
    return r


class Layer:
    """one description with its buffers; forward() and backward() run the HIP passes and check guards"""

    def __init__(self, ops, Cn, rows, dt=F32, fwd_rows=1, cpad=None, apply=True, relu=True, res=0, mask=0, fused_rows=0,
                 allow_fused=True, plan_nets=1):
        self.ops, self.C, self.rows, self.dt = ops, Cn, rows, dt
        self.cpad = Cn if cpad is None else cpad
        self.res, self.mask, self.relu, self.apply = res, mask, relu, apply
        self.fwd_rows, self.fused_rows = fwd_rows, fused_rows
        self.d = ops.bn_desc(Cn, rows, dt, self.cpad, apply, relu, res, mask, fwd_rows, fused_rows, allow_fused, plan_nets)
        self.plan = ops.bn_layer_plan(self.d)
        g = GUARD_ROWS * Cn
        self.coef = Guarded(7 * Cn, g, torch.float32)
        self.a = Guarded(rows * Cn, g, tdt(dt))
        self.guards = [self.coef, self.a]

    def dev(self, x64):
        return None if x64 is None else x64.to(tdt(self.dt)).to(DEV).contiguous()

    def forward(self, stats, y64, gamma, beta, res64=None, res_coef=None, rm=None, rv=None):
        """stats: fp32 cpu [fwd_rows, Cpad, 2] (NaN in the pad columns); returns the coefficient rows [7, C] (cpu)"""
        Cn = self.C
        self.stats = Guarded(stats.numel(), GUARD_ROWS * self.cpad * 2, torch.float32, band=float("nan"))
        self.stats.t.copy_(stats.reshape(-1))
        self.gamma, self.beta = gamma.to(DEV), beta.to(DEV)
        self.y = self.dev(y64)
        self.resd = self.dev(res64)
        self.rm = self.rv = None
        if rm is not None:
            self.rm, self.rv = Guarded(Cn, GUARD_ROWS * Cn, torch.float32), Guarded(Cn, GUARD_ROWS * Cn, torch.float32)
            self.rm.t.copy_(rm)
            self.rv.t.copy_(rv)
            self.guards += [self.rm, self.rv]
        before = self.stats.buf.view(torch.int32).clone()
        self.ops.bn_layer_forward(self.d, self.stats.t, self.gamma, self.beta, self.coef.t, self.y, a=self.a.t,
                                  res=self.resd, res_coef=res_coef,
                                  running_mean=None if self.rm is None else self.rm.t,
                                  running_var=None if self.rv is None else self.rv.t)
        torch.cuda.synchronize()
        assert torch.equal(before, self.stats.buf.view(torch.int32)), "the forward pass wrote into its statistics rows"
        self.check_guards()
        coef = self.coef.t.cpu().reshape(7, Cn)
        assert bool((coef[4:] == SENTINEL).all()), "the forward pass wrote into the backward's coefficient rows"
        if not self.apply:
            assert bool((self.a.t == SENTINEL).all()), "apply = 0 wrote the activation"
        return coef

    def check_guards(self):
        for k, gd in enumerate(self.guards):
            assert gd.intact(), f"guard band {k} of {len(self.guards)} overwritten"

    def act(self):
        return self.a.t.cpu().reshape(self.rows, self.C)

    def backward(self, dA64, partial=None, dres_mode=0, base64=None, want_dgamma=True):
        """partial: fp32 cpu [fused_rows, C, 2] when the description hands rows in.  dres_mode 0 none, 1 write,
        2 accumulate into base64.  Returns (dy, dres, dgamma, dbeta, k rows [3, C]) on the cpu."""
        Cn, g = self.C, GUARD_ROWS * self.C
        nan = float("nan")
        self.part = Guarded(max(int(self.plan.part_floats), 1), GUARD_ROWS * Cn * 2, torch.float32, fill=nan)
        if self.fused_rows > 0:
            assert partial.numel() == self.fused_rows * Cn * 2 <= self.plan.part_floats
            self.part.t[:partial.numel()].copy_(partial.reshape(-1))
        self.dy = Guarded(self.rows * Cn, g, tdt(self.dt))
        self.dres = Guarded(self.rows * Cn, g, tdt(self.dt))
        self.dgamma, self.dbeta = Guarded(Cn, g, torch.float32), Guarded(Cn, g, torch.float32)
        self.guards += [self.part, self.dy, self.dres, self.dgamma, self.dbeta]
        if dres_mode == 2:
            self.dres.t.copy_(self.dev(base64).reshape(-1))
        self.dA = self.dev(dA64)
        self.ops.bn_layer_backward(self.d, self.part.t, self.gamma, self.coef.t, self.y, self.dA, self.dy.t,
                                   a=self.a.t if self.mask == 2 else None, dres=self.dres.t if dres_mode else None,
                                   dres_acc=dres_mode == 2, dgamma=self.dgamma.t if want_dgamma else None,
                                   dbeta=self.dbeta.t if want_dgamma else None)
        torch.cuda.synchronize()
        self.check_guards()
        if dres_mode == 0:
            assert bool((self.dres.t == SENTINEL).all()), "dres written without being asked for"
        shape = (self.rows, Cn)
        return (self.dy.t.cpu().reshape(shape), self.dres.t.cpu().reshape(shape), self.dgamma.t.cpu(), self.dbeta.t.cpu(),
                self.coef.t.cpu().reshape(7, Cn)[4:])


def make_data(Cn, rows, dt, seed, res=0):
    """y, residual, dA as float64 holding storage-dtype values; gamma / beta fp32 with both signs of gamma"""
    g = torch.Generator().manual_seed(seed)
    std = 0.5 + 1.5 * torch.rand(Cn, generator=g, dtype=torch.float64)
    mean = 2.0 * torch.rand(Cn, generator=g, dtype=torch.float64) - 1.0
    y = torch.randn(rows, Cn, generator=g, dtype=torch.float64) * std + mean
    if rows < 64:  # a handful of rows: centred on half their spread, so that the one-pass variance of fp32-rounded rows
        y = y - y.mean(0) + 0.5 * y.std(0)  # stays conditioned (test_conditioning holds the other regime to the formula)
    y = stored(y, dt)
    r = stored(torch.randn(rows, Cn, generator=g, dtype=torch.float64), dt) if res else None
    dA = stored(torch.randn(rows, Cn, generator=g, dtype=torch.float64), dt)
    dA[dA == 0] = 1.0
    gamma = (0.5 + torch.rand(Cn, generator=g)) * torch.where(torch.rand(Cn, generator=g) < 0.25, -1.0, 1.0)
    beta = torch.rand(Cn, generator=g) - 0.5
    return y, r, dA, gamma.float(), beta.float()


def make_stats(y64, n, cpad, rng):
    """the forward partial rows of y: [n, cpad, 2] fp32, NaN in the pad columns"""
    s = chunk_sums(chunk_ids(y64.shape[0], n, rng), n, y64, y64 * y64)
    out = torch.full((n, cpad, 2), float("nan"), dtype=torch.float32)
    out[:, :y64.shape[1]] = s
    return out


def check_fwd_coef(coef, stats, Cn, N, gamma, beta, rm0=None, rv0=None, rm1=None, rv1=None):
    ref = fwd_coef_ref(stats, Cn, N, gamma, beta, rm0, rv0)
    assert bool(torch.isfinite(coef[:4]).all())
    for row, name in enumerate(("mean", "invstd", "scale")):
        assert within_ulps(coef[row], ref[name], 1), name
    slack = ulp_of(beta.double().abs() + (ref["mean"] * ref["scale"]).abs())
    assert bool(((coef[3].double() - ref["shift"].float().double()).abs() <= slack).all()), "shift"
    if rm0 is not None:
        assert within_ulps(rm1, ref["rm"], 1) and within_ulps(rv1, ref["rv"], 1), "running statistics"
    return ref


def a_formula(coef, y64, relu, res, res64=None, res_coef=None):
    """a and its rounding bound from the fp32 coefficient rows the HIP pass wrote"""
    sc, sf = coef[2].double(), coef[3].double()
    pre, terms = y64 * sc + sf, (y64 * sc).abs() + sf.abs()
    if res == 1:
        pre, terms = pre + res64, terms + res64.abs()
    elif res == 2:
        scr, sfr = res_coef[2].double(), res_coef[3].double()
        pre, terms = pre + res64 * scr + sfr, terms + (res64 * scr).abs() + sfr.abs()
    return (pre.clamp_min(0.0) if relu else pre), A_ROUNDINGS[res] * U24 * terms * (1 + 1e-6)


def check_elementwise(out, ref, bound, dt, what):
    if dt == BF16:  # one more rounding, of the fp32 result to storage (half a bf16 ulp <= 2^-8 relative)
        bound = bound * (1 + 2.0 ** -8) + ref.abs() * 2.0 ** -8
    err = (out.double() - ref).abs()
    bad = err > bound
    assert not bool(bad.any()), (what, int(bad.sum()), float((err - bound).max()), torch.nonzero(bad)[:4].tolist())


def torch_reference(y64, gamma, beta, dA64, relu, keep, res64=None, pair=None, dtype=torch.float64):
    """batch_norm + residual + ReLU (mask pinned to `keep`) with autograd; pair = (y_d, gamma_d, beta_d): the residual
    is another layer's BatchNorm.  Returns a, dy, dres, dgamma, dbeta (+ dy_d, dgamma_d, dbeta_d)."""
    def leaf(t):
        return t.detach().to(dtype).clone().requires_grad_(True)

    y, g, b = leaf(y64), leaf(gamma), leaf(beta)
    pre = F.batch_norm(y, None, None, g, b, True, 0.1, 1e-5)
    leaves = [y, g, b]
    r = leaf(torch.zeros_like(y64) if res64 is None else res64)
    if pair is not None:
        yd, gd, bd = leaf(pair[0]), leaf(pair[1]), leaf(pair[2])
        branch = F.batch_norm(yd, None, None, gd, bd, True, 0.1, 1e-5) + r
        leaves += [yd, gd, bd]
    else:
        branch = r
    pre = pre + branch
    a = pre * keep.to(dtype) if relu else pre
    a.backward(dA64.detach().to(dtype))
    return [a.detach(), y.grad, r.grad, g.grad, b.grad] + [t.grad for t in leaves[3:]]


def note_ratio(name, value):
    RATIOS[name] = max(RATIOS.get(name, 0.0), float(value))


def run_case(ops, Cn, rows, fwd_rows, dt, fused, res=1, relu=True, mask=2, fused_rows=0, dres_mode=1, cpad=None,
             plan_nets=1, seed=0, expect_fused=None, tag="case"):
    """forward + backward of one description against all references.  res 2 builds the other layer (apply = 0) first."""
    rng = np.random.default_rng(seed)
    y, r, dA, gamma, beta = make_data(Cn, rows, dt, seed, res)
    cpad = Cn if cpad is None else cpad
    stats = make_stats(y, fwd_rows, cpad, rng)
    res_coef_dev = res_coef = pair = None
    if res == 2:  # the downsample branch: r is its raw conv output
        _, _, _, gamma_d, beta_d = make_data(Cn, rows, dt, seed + 1000)
        D = Layer(ops, Cn, rows, dt, fwd_rows=3 if rows >= 3 else 1, apply=False, relu=False, allow_fused=fused)
        res_coef = D.forward(make_stats(r, D.fwd_rows, Cn, rng), r, gamma_d, beta_d)
        res_coef_dev, pair = D.coef.t, (r, gamma_d, beta_d)
    L = Layer(ops, Cn, rows, dt, fwd_rows, cpad, True, relu, res, mask, fused_rows, fused, plan_nets)
    if expect_fused is not None:
        assert (bool(L.plan.fwd_fused), bool(L.plan.bwd_fused)) == expect_fused, (L.plan.fwd_fused, L.plan.bwd_fused)
    g0 = torch.Generator().manual_seed(seed + 7)
    rm0, rv0 = torch.randn(Cn, generator=g0), 0.5 + torch.rand(Cn, generator=g0)
    coef = L.forward(stats, y, gamma, beta, r, res_coef_dev, rm0, rv0)
    check_fwd_coef(coef, stats, Cn, rows, gamma, beta, rm0, rv0, L.rm.t.cpu(), L.rv.t.cpu())
    a = L.act()
    ref_a, bound = a_formula(coef, y, relu, res, r, res_coef)
    check_elementwise(a, ref_a, bound, dt, tag + " a")
    keep = (a > 0) if mask else torch.ones_like(a, dtype=torch.bool)
    # ---- backward ----
    dz = dA * keep
    partial = None
    if fused_rows > 0:
        xhat = (y - coef[0].double()) * coef[1].double()
        partial = chunk_sums(chunk_ids(rows, fused_rows, rng), fused_rows, dz, dz * xhat)
    g1 = torch.Generator().manual_seed(seed + 9)
    base = stored(torch.randn(rows, Cn, generator=g1, dtype=torch.float64), dt) if dres_mode == 2 else None
    dy, dres, dgamma, dbeta, k = L.backward(dA, partial, dres_mode, base)
    assert all(bool(torch.isfinite(t.float()).all()) for t in (dy, dgamma, dbeta, k))
    N = float(rows)
    if fused_rows > 0:  # exactly computable: the kernel's formula on the same rows
        s1, s2 = partial[:, :, 0].double().sum(0), partial[:, :, 1].double().sum(0)
        assert within_ulps(dbeta, s1, 1) and within_ulps(dgamma, s2, 1), "dgamma / dbeta"
        assert within_ulps(k[1], s1 / N, 1) and within_ulps(k[2], s2 / N, 1), "k1 / k2"
    assert within_ulps(k[0], gamma.double() * coef[1].double(), 2), "k0"
    xh = (y - coef[0].double()) * coef[1].double()
    k0, k1, k2 = k[0].double(), k[1].double(), k[2].double()
    ref_dy = k0 * (dz - k1 - xh * k2)
    check_elementwise(dy, ref_dy, DY_ROUNDINGS * U24 * k0.abs() * (dz.abs() + k1.abs() + (xh * k2).abs()) * (1 + 1e-6), dt,
                      tag + " dy")
    if dres_mode == 1:
        assert torch.equal(dres.double(), dz), "dres != dz"
    elif dres_mode == 2:  # one rounding of base + dz in fp32, and one more to bf16 storage
        assert torch.equal(dres, (base.float() + dz.float()).to(tdt(dt))), "dres != base + dz"
    # ---- whole tensors against torch in float64 ----
    t64 = torch_reference(y, gamma, beta, dA, relu, keep, None if res == 2 else r, pair)
    tol = (1e-5, 2e-5) if dt == F32 else (4e-3, 4e-3)
    assert rel_l2(a, t64[0]) < tol[0], ("a", rel_l2(a, t64[0]))
    assert rel_l2(dy, t64[1]) < tol[1], ("dy", rel_l2(dy, t64[1]))
    assert rel_l2(dgamma, t64[3]) < 2e-5 and rel_l2(dbeta, t64[4]) < 2e-5, (rel_l2(dgamma, t64[3]), rel_l2(dbeta, t64[4]))
    if fused_rows == 0:  # bn_bwd_reduce's fp32 sums: per channel, in units of the CPU-fp32 reference's own error
        t32 = torch_reference(y, gamma, beta, dA, relu, keep, None if res == 2 else r, pair, dtype=torch.float32)
        scale_b, scale_g = dz.abs().sum(0).clamp_min(1e-30), (dz * xh).abs().sum(0).clamp_min(1e-30)
        for name, h, i, sc in (("dbeta", dbeta, 4, scale_b), ("dgamma", dgamma, 3, scale_g)):
            e_h, e_c = (h.double() - t64[i]).abs() / sc, (t32[i].double() - t64[i]).abs() / sc
            ratio = (e_h / torch.maximum(NOISE * e_c, torch.full_like(e_c, FLOOR))).max()
            print(f"BN-RATIO {tag} {name} worst error / gate {float(ratio):.3f} (worst error {float(e_h.max()):.2e})")
            note_ratio(name, ratio)
            assert ratio <= 1.0, (name, float(ratio))
        if dt == F32:
            nrm = t64[1].norm(dim=0).clamp_min(1e-30)
            e_h, e_c = (dy.double() - t64[1]).norm(dim=0) / nrm, (t32[1].double() - t64[1]).norm(dim=0) / nrm
            ratio = (e_h / torch.maximum(NOISE * e_c, torch.full_like(e_c, FLOOR))).max()
            print(f"BN-RATIO {tag} dy worst error / gate {float(ratio):.3f} (worst error {float(e_h.max()):.2e})")
            note_ratio("dy", ratio)
            assert ratio <= 1.0, ("dy per channel", float(ratio))
    return L


# ------------------------------------------------------------------------------------------
# the form matrix: C = 64, 1000 rows (no multiple of 32: the last row block holds 8 rows), 37 partial rows
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("relu", [True, False])
@pytest.mark.parametrize("res", [0, 1, 2])
@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("dt", [F32, BF16])
def test_forward_form_matrix(ops, dt, fused, res, relu):
    mask = 0 if not relu else (1 if res == 0 else 2)
    run_case(ops, 64, 1000, 37, dt, fused, res=res, relu=relu, mask=mask, fused_rows=0, dres_mode=1 if res else 0,
             seed=11, expect_fused=(fused, fused), tag=f"fwd-matrix dt{dt} fused{int(fused)} res{res} relu{int(relu)}")


@pytest.mark.parametrize("supplied", [0, 29])
@pytest.mark.parametrize("dres_mode", [0, 1, 2])
@pytest.mark.parametrize("mask", [0, 1, 2])
@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("dt", [F32, BF16])
def test_backward_form_matrix(ops, dt, fused, mask, dres_mode, supplied):
    res, relu = {0: (1, False), 1: (0, True), 2: (1, True)}[mask]
    run_case(ops, 64, 1000, 37, dt, fused, res=res, relu=relu, mask=mask, fused_rows=supplied, dres_mode=dres_mode,
             seed=13, expect_fused=(fused, fused),
             tag=f"bwd-matrix dt{dt} fused{int(fused)} mask{mask} dres{dres_mode} rows{supplied}")


# ------------------------------------------------------------------------------------------
# slab_reduce: its three loops change at 16 / 64 / 128 partial rows; 1025 rows: the plan must say split
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 15, 16, 17, 48, 49, 64, 65, 112, 113, 128, 129, 177, 241, 1023, 1024, 1025])
def test_slab_reduce_boundaries(ops, n):
    fused = n <= 1024
    run_case(ops, 32, 2048, n, F32, True, res=0, relu=True, mask=1, fused_rows=n, dres_mode=1, seed=100 + n,
             expect_fused=(fused, fused), tag=f"slab {n}")


# ------------------------------------------------------------------------------------------
# shapes: (C, rows, partial rows), residual tensor + ReLU, mask from a, fused where the plan allows
# ------------------------------------------------------------------------------------------
SHAPES = [(32, 2, 1, True), (32, 31, 3, True), (32, 33, 2, True), (256, 192, 12, True), (512, 48, 3, True),
          (128, 4097, 129, True), (64, 65536, 512, True), (32, 100000, 1024, True), (16, 5000, 40, False)]


@pytest.mark.parametrize("dt", [F32, BF16])
@pytest.mark.parametrize("Cn,rows,n,fused", SHAPES)
def test_shapes(ops, Cn, rows, n, fused, dt):
    bw = min(n, rows)
    run_case(ops, Cn, rows, n, dt, True, res=1, relu=True, mask=2, fused_rows=bw, dres_mode=1, seed=rows % 997,
             expect_fused=(fused, fused), tag=f"shape {Cn}x{rows}/{n} dt{dt}")
    if rows in (33, 4097, 5000):  # ... and with bn_bwd_reduce producing the sums
        run_case(ops, Cn, rows, n, dt, True, res=1, relu=True, mask=2, fused_rows=0, dres_mode=2, seed=rows % 997 + 1,
                 tag=f"shape {Cn}x{rows}/{n} dt{dt} reduce")


@pytest.mark.parametrize("dt", [F32, BF16])
def test_plan_nets_2_and_a_padded_statistics_stride(ops, dt):
    """plan_nets = 2 halves the workgroups the fused passes count (rows_per_block only); Cpad > C: the pad columns of
    the statistics rows hold NaN and must not be read"""
    one = Layer(ops, 64, 8192, dt, fwd_rows=64)
    two = run_case(ops, 64, 8192, 64, dt, True, fused_rows=32, plan_nets=2, cpad=80, seed=5, expect_fused=(True, True),
                   tag=f"plan_nets2 dt{dt}")
    assert two.plan.rows_per_block == 2 * one.plan.rows_per_block


# ------------------------------------------------------------------------------------------
# exactness contracts
# ------------------------------------------------------------------------------------------
def nudge(x64, dt, k):
    """x moved k units in the last place of its storage dtype"""
    if dt == F32:
        return (x64.float().view(torch.int32) + k).view(torch.float32).double()
    return (x64.to(torch.bfloat16).view(torch.int16) + k).view(torch.bfloat16).double()


@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("dt", [F32, BF16])
def test_recomputed_mask_is_bit_identical_at_the_threshold(ops, dt, fused):
    """BN_MASK_FROM_Y: 13 values per channel within +-6 units in the last place of -shift / scale, with negative, tiny
    and zero gamma channels, one of them gamma = beta = 0 (the only exact 0 in front of the recomputed mask).  The
    coefficients depend on the supplied rows only, which stay as they are: the planted values sit at the threshold.
    a must equal relu(fl(fl(y * scale) + shift)) bit for bit, and dres != 0 exactly where a > 0."""
    Cn, rows, n = 64, 1000, 37
    rng = np.random.default_rng(3)
    y, _, dA, gamma, beta = make_data(Cn, rows, dt, 3)
    gamma[0], beta[0] = 0.0, 0.0
    gamma[1], beta[1] = 0.0, 0.25
    gamma[2], beta[2] = 0.0, -0.25
    gamma[3], gamma[4], gamma[5] = 1e-6, -1e-6, -1.5
    stats = make_stats(y, n, Cn, rng)
    first = Layer(ops, Cn, rows, dt, n, relu=True, mask=1, allow_fused=fused)
    assert bool(first.plan.fwd_fused) == fused and bool(first.plan.bwd_fused) == fused
    coef = first.forward(stats, y, gamma, beta)
    sc, sf = coef[2].double(), coef[3].double()
    planted = torch.zeros(rows, Cn, dtype=torch.bool)
    for c in range(Cn):
        if sc[c] == 0:
            continue
        t = -sf[c] / sc[c]
        at = torch.from_numpy(rng.choice(rows, 13, replace=False))
        y[at, c] = torch.stack([nudge(t, dt, k) for k in range(-6, 7)])
        planted[at, c] = True
    L = Layer(ops, Cn, rows, dt, n, relu=True, mask=1, allow_fused=fused)
    coef2 = L.forward(stats, y, gamma, beta)
    assert torch.equal(coef2[:4], coef[:4])
    a = L.act()
    pre = y.float() * coef[2] + coef[3]  # (two fp32 operations: torch does not contract them)
    expect = pre.clamp_min(0.0).to(tdt(dt))
    assert torch.equal(a, expect), int((a != expect).sum())
    at_threshold = pre[planted]
    assert bool((at_threshold > 0).any()) and bool((at_threshold <= 0).any())
    assert bool((pre[:, 0] == 0).all()) and bool((a[:, 1] > 0).all()) and bool((a[:, 2] == 0).all())
    for supplied in (0, 29):
        B = Layer(ops, Cn, rows, dt, n, relu=True, mask=1, fused_rows=supplied, allow_fused=fused)
        B.forward(stats, y, gamma, beta)
        partial = None
        if supplied:
            dz = dA * (a > 0)
            xhat = (y - coef[0].double()) * coef[1].double()
            partial = chunk_sums(chunk_ids(rows, supplied, rng), supplied, dz, dz * xhat)
        _, dres, _, _, _ = B.backward(dA, partial, dres_mode=1)
        wrong = (dres != 0) != (a > 0)
        assert not bool(wrong.any()), (int(wrong.sum()), int((wrong & planted).sum()), torch.nonzero(wrong)[:4].tolist())


@pytest.mark.parametrize("supplied", [0, 29])
@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("dt", [F32, BF16])
def test_dead_channel_has_exactly_zero_gradients(ops, dt, fused, supplied):
    Cn, rows, n = 64, 1000, 37
    rng = np.random.default_rng(4)
    y, r, dA, gamma, beta = make_data(Cn, rows, dt, 4, res=1)
    beta[7], gamma[7] = -100.0, 1.0
    r[:, 9] = -50.0
    stats = make_stats(y, n, Cn, rng)
    L = Layer(ops, Cn, rows, dt, n, relu=True, res=1, mask=2, fused_rows=supplied, allow_fused=fused)
    coef = L.forward(stats, y, gamma, beta, r)
    a = L.act()
    assert bool((a[:, 7] == 0).all()) and bool((a[:, 9] == 0).all())
    partial = None
    if supplied:
        dz = dA * (a > 0)
        partial = chunk_sums(chunk_ids(rows, supplied, rng), supplied, dz, dz * ((y - coef[0].double()) * coef[1].double()))
    dy, dres, dgamma, dbeta, _ = L.backward(dA, partial, dres_mode=1)
    for c in (7, 9):
        assert dgamma[c] == 0 and dbeta[c] == 0 and bool((dy[:, c] == 0).all()) and bool((dres[:, c] == 0).all()), c
    assert bool((dgamma[:7] != 0).all())


@pytest.mark.parametrize("dt", [F32, BF16])
def test_fused_and_split_forms_agree(ops, dt):
    """the same description, inputs and supplied rows in both forms: coefficient rows within 1 ulp of each other, streamed
    tensors within the rounding bound (plus the coefficients' own ulp where they differ at all; bf16 storage: one bf16 ulp,
    2^-7 relative, where the two fp32 results round apart)"""
    Cn, rows, n, fr = 64, 1000, 37, 29
    rng = np.random.default_rng(6)
    y, r, dA, gamma, beta = make_data(Cn, rows, dt, 6, res=1)
    stats = make_stats(y, n, Cn, rng)
    outs = []
    for fused in (True, False):
        L = Layer(ops, Cn, rows, dt, n, relu=True, res=1, mask=2, fused_rows=fr, allow_fused=fused)
        assert bool(L.plan.fwd_fused) == fused and bool(L.plan.bwd_fused) == fused
        coef = L.forward(stats, y, gamma, beta, r)
        a = L.act()
        if not outs:
            dz = dA * (a > 0)
            partial = chunk_sums(chunk_ids(rows, fr, rng), fr, dz, dz * ((y - coef[0].double()) * coef[1].double()))
        dy, dres, dgamma, dbeta, k = L.backward(dA, partial, dres_mode=1)
        outs.append((coef[:4], a, dy, dres, dgamma, dbeta, k))
    f, s = outs
    for row in range(4):
        assert within_ulps(f[0][row], s[0][row].double(), 1)
    for i in (4, 5):
        assert within_ulps(f[i], s[i].double(), 1)
    for row in range(3):
        assert within_ulps(f[6][row], s[6][row].double(), 2 if row == 0 else 1)
    assert torch.equal(f[1] > 0, s[1] > 0) and torch.equal(f[3], s[3])
    ref_a, bound = a_formula(s[0], y, True, 1, r)
    extra = 2 * U24 * ((y * s[0][2].double()).abs() + s[0][3].double().abs())
    check_elementwise(f[1], s[1].double(), bound + extra + (s[1].double().abs() * 2.0 ** -7 if dt == BF16 else 0), F32, "a")
    k0, k1, k2 = (s[6][i].double() for i in range(3))
    xh = (y - s[0][0].double()) * s[0][1].double()
    dzf = dA * (s[1] > 0)
    bound = (DY_ROUNDINGS + 4) * U24 * k0.abs() * (dzf.abs() + k1.abs() + (xh * k2).abs())
    check_elementwise(f[2], s[2].double(), bound + (s[2].double().abs() * 2.0 ** -7 if dt == BF16 else 0), F32, "dy")


@pytest.mark.parametrize("fused", [True, False])
def test_null_running_statistics_and_no_gradient_outputs(ops, fused):
    """null running-statistics pointers: the same coefficients, nothing else written; null dgamma / dbeta: the same dy"""
    Cn, rows, n = 64, 1000, 37
    rng = np.random.default_rng(8)
    y, r, dA, gamma, beta = make_data(Cn, rows, F32, 8, res=1)
    stats = make_stats(y, n, Cn, rng)
    res = []
    for tracked in (True, False):
        L = Layer(ops, Cn, rows, F32, n, relu=True, res=1, mask=2, allow_fused=fused)
        rm0, rv0 = (torch.zeros(Cn), torch.ones(Cn)) if tracked else (None, None)
        coef = L.forward(stats, y, gamma, beta, r, rm=rm0, rv=rv0)
        dy, _, dgamma, _, k = L.backward(dA, None, dres_mode=0, want_dgamma=tracked)
        if not tracked:
            assert bool((dgamma == SENTINEL).all())
        res.append((coef[:4], L.act(), dy, k))
    for x, z in zip(*res):
        assert torch.equal(x, z)


@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("dt", [F32, BF16])
def test_conditioning(ops, dt, fused):
    """a constant channel (variance exactly 0), one whose rounded rows make s2 / N - mean^2 negative (the clamp), a channel
    with mean = 1000 x std, one of magnitude 1e-3 and one of 1e3: expected = the float64 formula on the same rows, whatever
    the conditioning, and everything finite"""
    Cn, rows, n = 32, 2048, 21
    rng = np.random.default_rng(9)
    y, r, dA, gamma, beta = make_data(Cn, rows, dt, 9, res=1)
    g = torch.Generator().manual_seed(10)
    y[:, 0] = 3.25
    y[:, 1] = 3.25
    y[:, 2] = stored(1000.0 + torch.randn(rows, generator=g, dtype=torch.float64), dt)
    y[:, 3] = stored(1e-3 * torch.randn(rows, generator=g, dtype=torch.float64), dt)
    y[:, 4] = stored(1e3 * torch.randn(rows, generator=g, dtype=torch.float64), dt)
    stats = make_stats(y, n, Cn, rng)
    stats[:, 1, 1] = torch.nextafter(stats[:, 1, 1], torch.zeros(n))  # every sum of squares one ulp short
    chk = fwd_coef_ref(stats, Cn, rows, gamma, beta)
    s2, m = stats[:, :Cn, 1].double().sum(0) / rows, chk["mean"]
    assert chk["var"][0] == 0 and (s2 - m * m)[0] == 0 and (s2 - m * m)[1] < -1e-7
    L = Layer(ops, Cn, rows, dt, n, relu=True, res=1, mask=2, fused_rows=17, allow_fused=fused)
    rm0, rv0 = torch.zeros(Cn), torch.ones(Cn)
    coef = L.forward(stats, y, gamma, beta, r, rm=rm0, rv=rv0)
    check_fwd_coef(coef, stats, Cn, rows, gamma, beta, rm0, rv0, L.rm.t.cpu(), L.rv.t.cpu())
    a = L.act()
    ref_a, bound = a_formula(coef, y, True, 1, r)
    check_elementwise(a, ref_a, bound, dt, "a")
    dz = dA * (a > 0)
    xh = (y - coef[0].double()) * coef[1].double()
    partial = chunk_sums(chunk_ids(rows, 17, rng), 17, dz, dz * xh)
    dy, dres, dgamma, dbeta, k = L.backward(dA, partial, dres_mode=1)
    s1, s2 = partial[:, :, 0].double().sum(0), partial[:, :, 1].double().sum(0)
    assert within_ulps(dbeta, s1, 1) and within_ulps(dgamma, s2, 1)
    assert within_ulps(k[1], s1 / rows, 1) and within_ulps(k[2], s2 / rows, 1)
    assert within_ulps(k[0], gamma.double() * coef[1].double(), 2)
    k0, k1, k2 = (k[i].double() for i in range(3))
    check_elementwise(dy, k0 * (dz - k1 - xh * k2),
                      DY_ROUNDINGS * U24 * k0.abs() * (dz.abs() + k1.abs() + (xh * k2).abs()) * (1 + 1e-6), dt, "dy")
    assert torch.equal(dres.double(), dz)
    assert all(bool(torch.isfinite(t.float()).all()) for t in (coef[:4], a, dy, dgamma, dbeta, k))


@pytest.mark.parametrize("fused", [True, False])
def test_running_statistics_over_three_calls(ops, fused):
    """three forward calls on different y against torch.nn.BatchNorm2d in float64 (momentum 0.1, unbiased variance) from
    non-trivial buffers.  Per call the HIP side rounds the new value once (2^-24 relative) and sees statistics taken from
    fp32-rounded rows (2^-24 of mean and of E[y^2]); momentum is the float 0.1f (1.5e-9 off 0.1)."""
    Cn, rows, n = 64, 1000, 37
    rng = np.random.default_rng(12)
    bn = torch.nn.BatchNorm2d(Cn).double().train()
    g0 = torch.Generator().manual_seed(12)
    rm, rv = torch.randn(Cn, generator=g0), 0.5 + torch.rand(Cn, generator=g0)
    with torch.no_grad():
        bn.running_mean.copy_(rm.double())
        bn.running_var.copy_(rv.double())
    worst = torch.zeros(Cn, dtype=torch.float64)
    for call in range(3):
        y, _, _, gamma, beta = make_data(Cn, rows, F32, 20 + call)
        stats = make_stats(y, n, Cn, rng)
        L = Layer(ops, Cn, rows, F32, n, relu=False, allow_fused=fused)
        L.forward(stats, y, gamma, beta, rm=rm, rv=rv)
        rm, rv = L.rm.t.cpu(), L.rv.t.cpu()
        bn(y.t().reshape(1, Cn, rows, 1))
        worst = torch.maximum(worst, (y * y).mean(0))
        tol_m = (call + 1) * 2 * U24 * (bn.running_mean.abs() + worst.sqrt())
        tol_v = (call + 1) * 2 * U24 * (bn.running_var.abs() + worst)
        assert bool(((rm.double() - bn.running_mean).abs() <= tol_m).all()), call
        assert bool(((rv.double() - bn.running_var).abs() <= tol_v).all()), call


@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("dt", [F32, BF16])
def test_downsample_pair(ops, dt, fused):
    """layer D with apply = 0, then a layer with res = 2 reading D's y and coefficient block: relu(bn(y) + bn_d(y_d));
    backward of both, the main layer's dres as D's dA (mask none)"""
    Cn, rows, n = 128, 777, 24
    rng = np.random.default_rng(14)
    y, yd, dA, gamma, beta = make_data(Cn, rows, dt, 14, res=1)
    _, _, _, gamma_d, beta_d = make_data(Cn, rows, dt, 15)
    D = Layer(ops, Cn, rows, dt, 6, apply=False, relu=False, mask=0, fused_rows=5, allow_fused=fused)
    stats_d = make_stats(yd, 6, Cn, rng)
    coef_d = D.forward(stats_d, yd, gamma_d, beta_d)
    check_fwd_coef(coef_d, stats_d, Cn, rows, gamma_d, beta_d)
    assert not D.plan.fwd_fused and bool(D.plan.bwd_fused) == fused
    M = Layer(ops, Cn, rows, dt, n, relu=True, res=2, mask=2, fused_rows=0, allow_fused=fused)
    stats = make_stats(y, n, Cn, rng)
    coef = M.forward(stats, y, gamma, beta, yd, D.coef.t)
    a = M.act()
    ref_a, bound = a_formula(coef, y, True, 2, yd, coef_d)
    check_elementwise(a, ref_a, bound, dt, "a")
    keep = a > 0
    dy, dres, dgamma, dbeta, _ = M.backward(dA, None, dres_mode=1)
    assert torch.equal(dres.double(), dA * keep)
    xh = (yd - coef_d[0].double()) * coef_d[1].double()
    partial = chunk_sums(chunk_ids(rows, 5, rng), 5, dres.double(), dres.double() * xh)
    dyd, _, dgd, dbd, _ = D.backward(dres.double(), partial, dres_mode=0)
    t = torch_reference(y, gamma, beta, dA, True, keep, None, (yd, gamma_d, beta_d))
    tol = (1e-5, 2e-5) if dt == F32 else (4e-3, 4e-3)
    assert rel_l2(a, t[0]) < tol[0] and rel_l2(dy, t[1]) < tol[1] and rel_l2(dyd, t[5]) < tol[1]
    for h, ref in ((dgamma, t[3]), (dbeta, t[4]), (dgd, t[6]), (dbd, t[7])):
        assert rel_l2(h, ref) < 2e-5, rel_l2(h, ref)


# ------------------------------------------------------------------------------------------
# refusals and the empty layer
# ------------------------------------------------------------------------------------------
def test_refusals_and_empty_layer(ops):
    from denoising_diffusion_deep_fake_amd import D3FError
    Cn, rows, n = 64, 64, 2
    rng = np.random.default_rng(1)
    y, r, dA, gamma, beta = make_data(Cn, rows, F32, 1, res=1)
    stats = make_stats(y, n, Cn, rng).to(DEV)
    yd, rd, dAd, gd, bd = y.float().to(DEV), r.float().to(DEV), dA.float().to(DEV), gamma.to(DEV), beta.to(DEV)
    coef = torch.full((7 * Cn,), SENTINEL, device=DEV)
    out = torch.full((rows, Cn), SENTINEL, device=DEV)
    part = torch.zeros(4096, device=DEV)

    def fwd(d, stats=stats, res=None, res_coef=None):
        ops.bn_layer_forward(d, stats, gd, bd, coef, yd, a=out, res=res, res_coef=res_coef)

    def bwd(d, partial=part, a=None):
        ops.bn_layer_backward(d, partial, gd, coef, yd, dAd, out, a=a)

    with pytest.raises(D3FError, match="res_coef"):
        fwd(ops.bn_desc(Cn, rows, res=2, fwd_rows=n), res=rd)
    with pytest.raises(D3FError, match="residual"):
        fwd(ops.bn_desc(Cn, rows, res=1, fwd_rows=n))
    with pytest.raises(D3FError, match="fwd_rows"):
        fwd(ops.bn_desc(Cn, rows, fwd_rows=0))
    with pytest.raises(D3FError, match="null"):
        fwd(ops.bn_desc(Cn, rows, fwd_rows=n), stats=None)
    with pytest.raises(D3FError, match="activation"):
        bwd(ops.bn_desc(Cn, rows, mask=2, fwd_rows=n))
    with pytest.raises(D3FError, match="partial"):
        bwd(ops.bn_desc(Cn, rows, fwd_rows=n, fused_rows=2), partial=None)
    with pytest.raises(D3FError, match="partial"):
        bwd(ops.bn_desc(Cn, rows, fwd_rows=n), partial=None)
    # 48 channels: no whole slabs, and the split kernels' row pattern does not fit either -> refused, nothing launched
    d48 = ops.bn_desc(48, rows, fwd_rows=n, allow_fused=True)
    p = ops.bn_layer_plan(d48)
    assert not p.fwd_fused and not p.bwd_fused
    with pytest.raises(D3FError, match="C=48"):
        fwd(d48)
    with pytest.raises(D3FError, match="C=48"):
        bwd(d48)
    # an empty layer: no launch, no error, nothing written
    empty = ops.bn_desc(Cn, 0, fwd_rows=n, res=1, mask=2)
    ops.bn_layer_forward(empty, None, None, None, None, None)
    ops.bn_layer_backward(empty, None, None, None, None, None, None)
    torch.cuda.synchronize()
    assert bool((coef == SENTINEL).all()) and bool((out == SENTINEL).all())


# ------------------------------------------------------------------------------------------
# the descriptions the engine launches
# ------------------------------------------------------------------------------------------
def engine_descriptions(dtype, B, S):
    """the distinct BatchNorm descriptions of a resnet34 plan, as d3f_unet_bn_layer hands them out"""
    from denoising_diffusion_deep_fake_amd import _lib
    lib = _lib.lib()
    h = C.c_void_p()
    _lib.check(lib.d3f_unet_create(b"resnet34", 3, 3, B, S, S, dtype, C.byref(h)))
    seen = {}
    try:
        n = lib.d3f_unet_num_bn(h)
        assert n == 46
        for i in range(n):
            d, p = _lib.BnDesc(), _lib.BnPlan()
            _lib.check(lib.d3f_unet_bn_layer(h, i, C.byref(d), C.byref(p)))
            key = tuple(getattr(d, f) for f, _ in _lib.BnDesc._fields_)
            seen.setdefault(key, (bool(p.fwd_fused), bool(p.bwd_fused)))
    finally:
        lib.d3f_unet_destroy(h)
    return seen


def run_engine_description(ops, key, planned, seed):
    from denoising_diffusion_deep_fake_amd import _lib
    f = dict(zip([n for n, _ in _lib.BnDesc._fields_], key))
    tag = f"engine {key}"
    if not f["apply"]:  # a downsample branch on its own: coefficients, then the backward without a mask
        rng = np.random.default_rng(seed)
        y, _, dA, gamma, beta = make_data(f["C"], f["rows"], f["dtype"], seed)
        L = Layer(ops, f["C"], f["rows"], f["dtype"], f["fwd_rows"], f["Cpad"], False, bool(f["relu"]), f["res"], f["mask"],
                  f["fused_rows"], bool(f["allow_fused"]), f["plan_nets"])
        assert (bool(L.plan.fwd_fused), bool(L.plan.bwd_fused)) == planned and f["mask"] == 0 and f["fused_rows"] == 0
        stats = make_stats(y, f["fwd_rows"], f["Cpad"], rng)
        coef = L.forward(stats, y, gamma, beta)
        check_fwd_coef(coef, stats, f["C"], f["rows"], gamma, beta)
        dy, _, dgamma, dbeta, _ = L.backward(dA, None, dres_mode=0)
        # (as a layer without ReLU or residual: a = bn(y))
        t = torch_reference(y, gamma, beta, dA, False, None)
        tol = 2e-5 if f["dtype"] == F32 else 4e-3
        assert rel_l2(dy, t[1]) < tol and rel_l2(dgamma, t[3]) < 2e-5 and rel_l2(dbeta, t[4]) < 2e-5
        return
    run_case(ops, f["C"], f["rows"], f["fwd_rows"], f["dtype"], bool(f["allow_fused"]), res=f["res"], relu=bool(f["relu"]),
             mask=f["mask"], fused_rows=f["fused_rows"], dres_mode=1 if f["res"] else 0, cpad=f["Cpad"],
             plan_nets=f["plan_nets"], seed=seed, expect_fused=planned, tag=tag)


@pytest.mark.parametrize("dtype", [F32, BF16])
@pytest.mark.parametrize("B,S", [(3, 64), (16, 256)])
def test_every_description_the_engine_launches(ops, dtype, B, S):
    """the operator tests stand on the shapes the engine launches: every distinct description of the 3 x 64 x 64 and the
    16 x 256 x 256 plan, once each, under the gates of run_case"""
    seen = engine_descriptions(dtype, B, S)
    assert len(seen) >= 10
    for k, (key, planned) in enumerate(sorted(seen.items())):
        run_engine_description(ops, key, planned, 300 + k)


# ------------------------------------------------------------------------------------------
# the two fallback knobs, under the whole-network layer gates
# ------------------------------------------------------------------------------------------
_KNOB_SCRIPT = r"""
import ctypes as C, sys
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, sys.argv[1] + "/tests")
from denoising_diffusion_deep_fake_amd import _lib
lib = _lib.lib()
h = C.c_void_p()
_lib.check(lib.d3f_unet_create(b"resnet34", 3, 3, 3, 64, 64, _lib.F32, C.byref(h)))
fwd = bwd = handed = 0
for i in range(lib.d3f_unet_num_bn(h)):
    d, p = _lib.BnDesc(), _lib.BnPlan()
    _lib.check(lib.d3f_unet_bn_layer(h, i, C.byref(d), C.byref(p)))
    fwd, bwd, handed = fwd + p.fwd_fused, bwd + p.bwd_fused, handed + (d.fused_rows > 0)
lib.d3f_unet_destroy(h)
print("PLAN", fwd, bwd, handed)
import test_gpu_parity_layers as gates
gates._layer_parity("f32", 3, 64, 64)
print("GATES PASSED")
"""


@pytest.mark.parametrize("knob", ["D3F_NO_BN_FUSED_FINALIZE", "D3F_NO_FUSED_BN_REDUCE"])
def test_fallback_knobs_pass_the_layer_gates(knob, tmp_path):
    """D3F_NO_BN_FUSED_FINALIZE (every layer in the split form) and D3F_NO_FUSED_BN_REDUCE (every backward through
    bn_bwd_reduce) under the unchanged gates of tests/test_gpu_parity_layers.py at 3 x 64 x 64, each in a fresh child
    process (the library reads its knobs once); the plan the child reports shows that the knob took hold."""
    import os
    import subprocess
    import sys
    from pathlib import Path
    root = str(Path(__file__).resolve().parent.parent)
    script = tmp_path / "knob.py"
    script.write_text(_KNOB_SCRIPT)
    env = {k: v for k, v in os.environ.items() if k not in ("D3F_NO_BN_FUSED_FINALIZE", "D3F_NO_FUSED_BN_REDUCE")}
    env[knob] = "1"
    out = subprocess.run([sys.executable, str(script), root], env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "GATES PASSED" in out.stdout, (out.stdout[-2000:], out.stderr[-3000:])
    fwd, bwd, handed = (int(v) for v in [l for l in out.stdout.splitlines() if l.startswith("PLAN")][0].split()[1:])
    want = {"D3F_NO_BN_FUSED_FINALIZE": (0, 0, 39), "D3F_NO_FUSED_BN_REDUCE": (41, 44, 0)}[knob]  # (none: 41, 44, 39)
    assert (fwd, bwd, handed) == want, (knob, fwd, bwd, handed)
