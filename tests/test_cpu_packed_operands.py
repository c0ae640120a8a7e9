"""CPU: the restated weight operands of tests/packed_restatement.py against something that is not the kernel (host only).

* contracting the restated wfc, wd4 and wds in float64 reproduces conv2d(cat(upsample2x(x), skip)) and its two data
  gradients exactly on operands in {-1, 0, 1} (every pre-summed weight is then an integer of at most 4, exact in fp32,
  bf16 and in the first plane of f32x3), for both storage geometries and for a layer without a skip tensor;
* the restated plain layouts contract to conv2d and its data gradient, stride 1 and the parity order of stride 2;
* the restated Winograd U equals G g G^T: exactly on {-1, 0, 1} (quarter-integers), within its four roundings on N(0, 1);
* the three-way split: h + m + l == v exactly, each term has at most 8 significant bits, and it is by truncation.
"""
import pytest
import torch
import torch.nn.functional as F

import packed_restatement as pr
from packed_restatement import BF16, F32, F32X3

U24 = 2.0 ** -24
UPFOLD_SHAPES = [(F32, 32, 32, 24), (F32, 32, 0, 8), (F32X3, 32, 32, 24), (F32X3, 32, 0, 8), (BF16, 64, 64, 24), (BF16, 64, 0, 8)]


def trits(g, *shape):
    return torch.randint(-1, 2, shape, generator=g).double()


def as_values(bits, dt):
    """the float64 values a buffer of stored bits holds (f32x3: the sum of its planes)"""
    if dt == F32:
        return bits[0].view(torch.float32).double()
    return pr.plane_values(bits).sum(0)


@pytest.mark.parametrize("dt,C0,C1,Cout", UPFOLD_SHAPES)
def test_upfold_layouts_contract_to_the_convolution(dt, C0, C1, Cout):
    g = torch.Generator().manual_seed(C0 + C1 + Cout)
    h, w_ = 3, 5                                           # low-resolution extent: odd, non-square
    x, skip = trits(g, 2, C0, h, w_), trits(g, 2, C1, 2 * h, 2 * w_)
    w = trits(g, Cout, C0 + C1, 3, 3)
    dy = trits(g, 2, Cout, 2 * h, 2 * w_)
    xin = torch.cat([x.repeat_interleave(2, 2).repeat_interleave(2, 3), skip], 1)
    y_ref = F.conv2d(xin, w, None, 1, 1)
    dx_ref = torch.nn.grad.conv2d_input(xin.shape, w, dy, 1, 1)
    dx0_ref = dx_ref[:, :C0]
    dx0_ref = dx0_ref[:, :, 0::2, 0::2] + dx0_ref[:, :, 0::2, 1::2] + dx0_ref[:, :, 1::2, 0::2] + dx0_ref[:, :, 1::2, 1::2]
    geo = pr.geometry(dt, C0, C1, Cout, 3)
    wfc32, wd432, wds32 = pr.upfold_layouts(w.float(), C0, C1, Cout, dt)
    # through the storage type and back: what the kernels read
    wfc = as_values(pr.stored_bits(wfc32, dt), dt)
    wd4 = as_values(pr.stored_bits(wd432, dt), dt)
    assert torch.equal(wfc, wfc32.double()) and torch.equal(wd4, wd432.double()), "integers up to 4 are exact in every type"
    assert not bool(wfc[:, Cout:].any()) and not bool(wd4[C0:].any()), "padding rows"
    coutd = geo["CoutD"]
    # forward, class by class: a 2 x 2 convolution over the low-resolution source + the 3 x 3 taps of the skip tensor
    y = torch.zeros_like(y_ref)
    xp = F.pad(x, (1, 1, 1, 1))
    for py in range(2):
        for px in range(2):
            wz = wfc[2 * py + px, :Cout]
            w2 = wz[:, :4 * C0].reshape(Cout, 2, 2, C0).permute(0, 3, 1, 2)
            yz = F.conv2d(xp, w2)[:, :, py:py + h, px:px + w_]      # low-resolution row of tap a: j + a + py - 1
            if C1:
                w3 = wz[:, 4 * C0:].reshape(Cout, 3, 3, C1).permute(0, 3, 1, 2)
                yz = yz + F.conv2d(skip, w3, None, 1, 1)[:, :, py::2, px::2]
            y[:, :, py::2, px::2] = yz
    assert torch.equal(y, y_ref), "wfc"
    # gradient of the low-resolution source: a 4 x 4 stride-2 pad-1 convolution over dY
    w4 = wd4[:C0].reshape(C0, 4, 4, coutd)[..., :Cout].permute(0, 3, 1, 2)
    assert torch.equal(F.conv2d(dy, w4, None, 2, 1), dx0_ref), "wd4"
    assert not bool(wd4[:C0].reshape(C0, 16, coutd)[..., Cout:].any())
    if C1:
        wds = as_values(pr.stored_bits(wds32, dt), dt)
        assert wds.shape == (geo["C1Rows"], geo["KpadD"]) and not bool(wds[:, 9 * coutd:].any()) and not bool(wds[C1:].any())
        w3 = wds[:C1, :9 * coutd].reshape(C1, 3, 3, coutd)[..., :Cout].permute(0, 3, 1, 2)
        assert torch.equal(F.conv2d(dy, w3, None, 1, 1), dx_ref[:, C0:]), "wds"
    else:
        assert wds32 is None


@pytest.mark.parametrize("C0,CinReal,Cout,K,stride,pad", [(16, 13, 24, 3, 1, 1), (32, 32, 32, 3, 2, 1), (32, 32, 32, 1, 2, 0)])
def test_plain_layouts_contract_to_the_convolution(C0, CinReal, Cout, K, stride, pad):
    g = torch.Generator().manual_seed(C0 + Cout + K)
    H = 8
    x, w = trits(g, 2, CinReal, H, H), trits(g, Cout, CinReal, K, K)
    y_ref = F.conv2d(x, w, None, stride, pad)
    dy = trits(g, *y_ref.shape)
    dx_ref = torch.nn.grad.conv2d_input(x.shape, w, dy, stride, pad)
    geo = pr.geometry(F32, C0, 0, Cout, K)
    wf, wd = pr.plain_layouts(w.float(), C0, Cout, K, stride, pad, F32)
    wf, wd = wf.double(), wd.double()
    assert not bool(wf[Cout:].any()) and not bool(wf[:, K * K * C0:].any())
    wk = wf[:Cout, :K * K * C0].reshape(Cout, K, K, C0)[..., :CinReal].permute(0, 3, 1, 2)
    assert torch.equal(F.conv2d(x, wk, None, stride, pad), y_ref)
    # data gradient: slot s holds flipped tap f(s); a transposed convolution reads w[n][c][taps - 1 - f]
    coutd, taps = geo["CoutD"], K * K
    parity = stride == 2 and coutd % 32 == 0
    flipped = pr.PARITY_SLOTS if parity and taps == 9 else tuple(range(taps))
    back = torch.zeros(CinReal, Cout, taps, dtype=torch.float64)
    body = wd[:CinReal, :taps * coutd].reshape(CinReal, taps, coutd)
    for slot, f in enumerate(flipped):
        back[:, :, taps - 1 - f] = body[:, slot, :Cout]
    assert sorted(flipped) == list(range(taps)) and not bool(wd[CinReal:].any()) and not bool(wd[:, taps * coutd:].any())
    dx = F.conv_transpose2d(dy, back.permute(1, 0, 2).reshape(Cout, CinReal, K, K), None, stride, pad,
                            output_padding=(H + 2 * pad - K) % stride)
    assert torch.equal(dx, dx_ref)


@pytest.mark.parametrize("K,C", [(64, 16), (64, 32), (128, 48)])
def test_winograd_filter_restatement_is_g_G_gt(K, C):
    gen = torch.Generator().manual_seed(K + C)
    G = torch.tensor([[1, 0, 0], [.5, .5, .5], [.5, -.5, .5], [0, 0, 1]], dtype=torch.float64)
    w = trits(gen, K, C, 3, 3)
    u = pr.winograd_filter_fp32(w.float())
    assert torch.equal(u.double(), torch.einsum("ia,kcab,jb->kcij", G, w, G)), "quarter-integers are exact"
    U = pr.winograd_layout(u)
    assert U.shape == (16, C // 16, K, 16)
    for pos, c, k in ((0, 0, 0), (5, C - 1, K - 1), (14, 17 % C, 33)):
        assert U[pos, c // 16, k, c % 16] == u[k, c, pos // 4, pos % 4]
    assert torch.equal(pr.winograd_unlayout(U), u)
    # full significands: two additions per stage, the halvings exact -- four roundings relative to |G| |g| |G^T|
    w = torch.randn(K, C, 3, 3, generator=gen)
    u = pr.winograd_filter_fp32(w)
    ref = torch.einsum("ia,kcab,jb->kcij", G, w.double(), G)
    mag = torch.einsum("ia,kcab,jb->kcij", G.abs(), w.double().abs(), G.abs())
    assert bool(((u.double() - ref).abs() <= 4 * U24 / (1 - 4 * U24) * mag).all())
    assert bool((u.double() != ref).any()), "fp32 values, not float64 ones"


def test_three_way_split_is_exact_and_by_truncation():
    gen = torch.Generator().manual_seed(3)
    v = torch.randn(4096, generator=gen)
    v[::7] = v[::7].bfloat16().float()                                        # second and third term zero
    v[3::11] = (v[3::11].view(torch.int32) & -256).view(torch.float32)        # 16 significant bits: third term zero
    planes = pr.split3(v)
    h, m, l = pr.plane_values(planes)
    assert torch.equal(h + m + l, v.double())
    assert bool((h.abs() <= v.double().abs()).all()) and bool(((h == 0) | (h.sign() == v.double().sign())).all()), "truncation"
    assert bool((m[::7] == 0).all()) and bool((l[::7] == 0).all()) and bool((l[3::11] == 0).all())
    assert bool((m != 0).sum() > 3000) and bool((l != 0).sum() > 3000)
    nz = v != 0
    assert bool((m.abs()[nz] < 2.0 ** -7 * v.double().abs()[nz]).all()) and bool((l.abs()[nz] < 2.0 ** -15 * v.double().abs()[nz]).all())
    # the first plane is the truncated value, not the rounded one, wherever the two differ
    rounded = pr.bits_of(v.bfloat16())
    assert bool((planes[0] != rounded).any())
    assert torch.equal(pr.stored_bits(torch.tensor([0.0, 1.0, -2.5]), F32X3)[1:], torch.zeros(2, 3, dtype=torch.int16))
