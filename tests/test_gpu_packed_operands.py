"""GPU: the derived weight operands bit for bit against tests/packed_restatement.py.

| kernel                                   | reached by                                                              |
|------------------------------------------|-------------------------------------------------------------------------|
| winograd_pack_kernel                     | test_winograd_filter (d3f_conv_winograd_pack)                           |
| pack_all_kernel<bf16_t, true> (f32x3)    | test_f32x3_plain_layouts (d3f_conv_pack_weights), both layouts          |
| pack_up_kernel<float, false>             | test_upfold_layouts[f32-*]  (d3f_conv_pack_weights on a folded layer)   |
| pack_up_kernel<bf16_t, false>            | test_upfold_layouts[bf16-*]                                             |
| pack_up_kernel<bf16_t, true> (f32x3)     | test_upfold_layouts[f32x3-*]                                            |

(pack_all_kernel<T, false> is tests/test_gpu_helper_kernels.py::test_pack_weights.)  These kernels copy, add a handful
of fp32 numbers in a fixed order, halve, round once to bf16 or split by truncation: every stored bit is determined, so
the comparison is equality of bit patterns over the whole buffer, zero padding included, and a failure names the first
element that differs.

Weights are N(0, 1) fp32 with full significands, negative ones among them; some are replaced by values whose second and
third, or whose third, bf16 term is zero.  All of them and every remainder of the split stay in the normal range.
Every buffer is sized by d3f_conv_packed_bytes / d3f_conv_winograd_filter_bytes (the size asserted against the
restatement's own), sits between guard bands, starts as NaN bytes and is packed twice from that poisoned state.
"""
import ctypes as C

import pytest
import torch

import packed_restatement as pr
from denoising_diffusion_deep_fake_amd import _lib
from packed_restatement import BF16, F32, F32X3
from test_gpu_helper_kernels import PACK_CASES
from util import Guarded

pytestmark = pytest.mark.gpu

GUARD_BYTES = 4096
NAN_BYTE, BAND_BYTE = 0xFF, 0xA5
NAMES = {F32: "f32", BF16: "bf16", F32X3: "f32x3"}


def weights(gen, *shape):
    """N(0, 1) with full significands; every 7th value exact in bf16 (second and third term zero), every 11th cut to
    16 significant bits (third term zero)"""
    w = torch.randn(*shape, generator=gen)
    flat = w.view(-1)
    flat[::7] = flat[::7].bfloat16().float()
    flat[3::11] = (flat[3::11].contiguous().view(torch.int32) & -256).view(torch.float32)
    assert bool((flat < 0).any()) and bool((flat.abs() > 2.0 ** -100).all())
    return w


def byte_buffer(n):
    return Guarded(int(n), GUARD_BYTES, torch.uint8, fill=NAN_BYTE, band=BAND_BYTE)


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def ptr(g):
    return None if g is None else C.c_void_p(g.t.data_ptr())


def pack_twice(call, bufs):
    """call() twice, each time from NaN bytes: the same bytes both times, the guard bands whole; returns the bytes"""
    runs = []
    for _ in range(2):
        for b in bufs:
            b.t.fill_(NAN_BYTE)
        _lib.check(call())
        torch.cuda.synchronize()
        runs.append([b.t.cpu().clone() for b in bufs])
        assert all(b.intact() for b in bufs), "guard band overwritten"
    for a, b in zip(*runs):
        assert torch.equal(a, b), "two packs from the same poisoned state differ"
    return runs[1]


def same_bits(name, got_bytes, want):
    """got_bytes: uint8 [n]; want: int16 / int32 bit patterns, flat"""
    got = got_bytes.view(want.dtype)
    assert got.numel() == want.numel(), (name, got.numel(), want.numel())
    diff = got != want
    n = int(diff.sum())
    if n:
        i, mask = int(diff.nonzero()[0]), (1 << 8 * want.element_size()) - 1
        raise AssertionError(f"{name}: {n} of {want.numel()} elements differ, first at {i}: "
                             f"got {int(got[i]) & mask:#x}, want {int(want[i]) & mask:#x}")


@pytest.mark.parametrize("K,Cin", [(64, 16), (64, 32), (128, 48)])
def test_winograd_filter(K, Cin):
    """U[pos][c / 16][k][c % 16] = G g G^T in winograd_pack_kernel's own operation order"""
    L = _lib.lib()
    d = _lib.ConvDesc(1, 16, 16, Cin, 0, 0, K, 3, 3, 1, 1, Cin)
    w = weights(torch.Generator().manual_seed(K + Cin), K, Cin, 3, 3)
    want = pr.bits_of(pr.winograd_layout(pr.winograd_filter_fp32(w))).reshape(-1)
    assert L.d3f_conv_winograd_filter_bytes(C.byref(d)) == want.numel() * 4 == 16 * K * Cin * 4
    u = byte_buffer(want.numel() * 4)
    wd = w.cuda()
    (got,) = pack_twice(lambda: L.d3f_conv_winograd_pack(C.byref(d), C.c_void_p(wd.data_ptr()), ptr(u), stream()), [u])
    same_bits("U", got, want)


@pytest.mark.parametrize("C0,CinReal,Cout,K,stride,pad", PACK_CASES)
def test_f32x3_plain_layouts(C0, CinReal, Cout, K, stride, pad):
    """the three bf16 planes of pack_store<T, true> through pack_all_kernel, on the fp32 geometries of PACK_CASES: each
    plane the truncated top 16 bits of the running remainder, h + m + l == v, zero padding in all three planes"""
    if C0 == 8 and CinReal == 3:
        C0 = 4   # fp32 storage pads the stem to one vector of four channels
    L = _lib.lib()
    d = _lib.ConvDesc(1, 16, 16, C0, 0, 0, Cout, K, K, stride, pad, CinReal)
    w = weights(torch.Generator().manual_seed(C0 + Cout + K), Cout, CinReal, K, K)
    wf32, wd32 = pr.plain_layouts(w, C0, Cout, K, stride, pad, F32X3)
    want_f, want_d = pr.split3(wf32), pr.split3(wd32)
    assert L.d3f_conv_packed_bytes(F32X3, C.byref(d), 0) == want_f.numel() * 2 == 6 * wf32.numel()
    assert L.d3f_conv_packed_bytes(F32X3, C.byref(d), 1) == want_d.numel() * 2 == 6 * wd32.numel()
    wf, wd = byte_buffer(want_f.numel() * 2), byte_buffer(want_d.numel() * 2)
    wdev = w.cuda()
    got_f, got_d = pack_twice(lambda: L.d3f_conv_pack_weights(F32X3, C.byref(d), C.c_void_p(wdev.data_ptr()), ptr(wf), ptr(wd),
                                                               stream()), [wf, wd])
    same_bits("forward planes", got_f, want_f.reshape(-1))
    same_bits("data-gradient planes", got_d, want_d.reshape(-1))
    # what the planes say about themselves, without the restated split
    for got, v32 in ((got_f, wf32), (got_d, wd32)):
        h, m, l = pr.plane_values(got.view(torch.int16).view(3, *v32.shape))
        assert torch.equal(h + m + l, v32.double()), "h + m + l != v"
        assert torch.equal(h.float(), (v32.view(torch.int32) & -65536).view(torch.float32)), "first plane: truncation"
        assert torch.equal(m.float(), ((v32 - h.float()).view(torch.int32) & -65536).view(torch.float32)), "second plane"
        pad_mask = v32 == 0   # (no weight is zero: exactly the padding, where the geometry has any)
        assert not bool(h[pad_mask].any() or m[pad_mask].any() or l[pad_mask].any())


UPFOLD_CASES = [(F32, 32, 32, 24), (F32, 32, 0, 8), (F32X3, 32, 32, 24), (F32X3, 32, 0, 8), (BF16, 64, 64, 24), (BF16, 64, 0, 8)]


@pytest.mark.parametrize("dt,C0,C1,Cout", UPFOLD_CASES, ids=[f"{NAMES[c[0]]}-{c[1]}+{c[2]}to{c[3]}" for c in UPFOLD_CASES])
def test_upfold_layouts(dt, C0, C1, Cout):
    """wfc per class with the S-sets, wd4 with the T-sets, wds flipped and padded to whole k-tiles; fp32 sums kh-major,
    kw-minor, then one round-to-nearest-even (bf16) or the three-way split (f32x3).  Cout = 24 leaves zero filter rows
    inside CoutPad; C1 = 0 has no wds.  The forward-only call writes the same wfc."""
    L = _lib.lib()
    d = _lib.ConvDesc(1, 8, 8, C0, C1, 2, Cout, 3, 3, 1, 1, C0 + C1)
    assert L.d3f_conv_upsample_folded(dt, C.byref(d)) == 1
    w = weights(torch.Generator().manual_seed(C0 + C1 + Cout + dt), Cout, C0 + C1, 3, 3)
    wfc32, wd432, wds32 = pr.upfold_layouts(w, C0, C1, Cout, dt)
    assert (wds32 is None) == (C1 == 0)
    want_f, want_d = pr.upfold_forward_bits(wfc32, dt), pr.upfold_dgrad_bits(wd432, wds32, dt)
    esz = want_f.element_size()
    assert L.d3f_conv_packed_bytes(dt, C.byref(d), 0) == want_f.numel() * esz
    assert L.d3f_conv_packed_bytes(dt, C.byref(d), 1) == want_d.numel() * esz
    wf, wd = byte_buffer(want_f.numel() * esz), byte_buffer(want_d.numel() * esz)
    wdev = w.cuda()
    got_f, got_d = pack_twice(lambda: L.d3f_conv_pack_weights(dt, C.byref(d), C.c_void_p(wdev.data_ptr()), ptr(wf), ptr(wd),
                                                               stream()), [wf, wd])
    same_bits("wfc", got_f, want_f)
    n4 = pr.stored_bits(wd432, dt).numel()
    same_bits("wd4", got_d[:n4 * esz], want_d[:n4])
    if C1:
        same_bits("wds", got_d[n4 * esz:], want_d[n4:])
    assert wfc32.shape[1] > Cout, "the case has zero filter rows inside CoutPad"
    # forward only: w_dgrad null
    only = byte_buffer(want_f.numel() * esz)
    (got_o,) = pack_twice(lambda: L.d3f_conv_pack_weights(dt, C.byref(d), C.c_void_p(wdev.data_ptr()), ptr(only), None, stream()),
                          [only])
    same_bits("wfc, forward-only call", got_o, want_f)
