"""CPU: colour match without a device -- the restatement's coefficients against a brute-force mean / std formula, its
D == 0 and clamp branches, the host-side guards of the three operators and of the engine's mode (everything is refused
before a device call: the dummy pointers are never dereferenced), the render tool's --color-match, the mode strings, and the
header / binding tables."""
import ctypes as C

import numpy as np
import pytest
import torch

from color_match_restatement import (GAIN_MAX, GAIN_MIN, MAX_PIXELS, channel_sums, color_match_coef, paste_color_f64,
                                     sums_array)
from denoising_diffusion_deep_fake_amd import _lib, ops
from paste_restatement import paste_f64

NEW_SYMBOLS = ("d3f_channel_sums_u8", "d3f_color_match_coef", "d3f_paste_resize_cubic_color_u8",
               "d3f_unet_set_frame_color_match", "d3f_unet_frame_color_match")


def _images(seed, shape, lo=0, hi=256):
    return np.random.default_rng(seed).integers(lo, hi, size=shape, dtype=np.uint8)


def test_restatement_sums_are_the_plain_sums():
    img = _images(1, (3, 5, 37, 3))
    sums = channel_sums(img)
    for b in range(3):
        for c in range(3):
            p = [int(v) for v in img[b, :, :, c].reshape(-1)]
            assert sums[b][c] == [sum(p), sum(v * v for v in p)]
    assert channel_sums(img[0]) == sums[:1]                      # a single image is a batch of one
    full = channel_sums(np.full((1, 2048, 2048, 3), 255, dtype=np.uint8))
    assert full == [[[255 << 22, 65025 << 22]] * 3] and 2048 * 2048 == MAX_PIXELS
    assert sums_array(sums).shape == (3, 3, 2) and sums_array(sums).dtype == np.uint64


@pytest.mark.parametrize("seed, hw", [(2, (9, 14)), (3, (1, 50)), (4, (33, 7))])
def test_restatement_coefficients_against_brute_force_mean_and_std(seed, hw):
    """gain = std_to / std_from and offset = mean_to - gain * mean_from of the population statistics, to float64 accuracy:
    the integer form n Q - S^2 is n^2 times the variance"""
    src = _images(seed, (2,) + hw + (3,), 40, 140)    # std ratio well inside the clamp
    dst = _images(seed + 50, (2,) + hw + (3,), 30, 180)
    n = hw[0] * hw[1]
    coef = color_match_coef(channel_sums(src), channel_sums(dst), n)
    assert coef.shape == (2, 3, 2) and coef.dtype == np.float32
    for b in range(2):
        for c in range(3):
            f, t = src[b, :, :, c].astype(np.float64), dst[b, :, :, c].astype(np.float64)
            g = t.std() / f.std()
            assert GAIN_MIN < g < GAIN_MAX
            o = t.mean() - g * f.mean()
            assert abs(float(coef[b, c, 0]) - g) <= 1e-6 * g
            assert abs(float(coef[b, c, 1]) - o) <= 1e-5 * max(1.0, abs(o))
            # what the coefficients are for: the matched image has the target's statistics
            matched = float(coef[b, c, 0]) * f + float(coef[b, c, 1])
            assert abs(matched.mean() - t.mean()) < 1e-3 and abs(matched.std() - t.std()) < 1e-3


def test_restatement_flat_images_and_both_clamp_ends():
    rng_img = _images(5, (1, 8, 8, 3))
    flat = np.full((1, 8, 8, 3), 77, dtype=np.uint8)
    n = 64
    # a constant `from`: D_from == 0, gain 1, offset = mean_to - 77
    coef = color_match_coef(channel_sums(flat), channel_sums(rng_img), n)
    for c in range(3):
        assert coef[0, c, 0] == 1
        assert coef[0, c, 1] == np.float32(rng_img[0, :, :, c].astype(np.float64).sum() / n - 77.0)
    # a constant `to`: D_to == 0, gain 1 as well (not 0: a flat target says nothing about contrast)
    coef = color_match_coef(channel_sums(rng_img), channel_sums(flat), n)
    for c in range(3):
        assert coef[0, c, 0] == 1
        assert coef[0, c, 1] == np.float32(77.0 - rng_img[0, :, :, c].astype(np.float64).sum() / n)
    # both constant
    assert np.array_equal(color_match_coef(channel_sums(flat), channel_sums(flat), n)[0], [[1, 0]] * 3)
    # the clamp: a narrow image against a wide one, both ways
    narrow = _images(6, (1, 8, 8, 3), 100, 110)
    wide = _images(7, (1, 8, 8, 3), 0, 256)
    up = color_match_coef(channel_sums(narrow), channel_sums(wide), n)
    down = color_match_coef(channel_sums(wide), channel_sums(narrow), n)
    for c in range(3):
        ratio = wide[0, :, :, c].astype(np.float64).std() / narrow[0, :, :, c].astype(np.float64).std()
        assert ratio > 8                                  # far beyond the clamp
        assert up[0, c, 0] == np.float32(GAIN_MAX) and down[0, c, 0] == np.float32(GAIN_MIN)
        m_n, m_w = narrow[0, :, :, c].astype(np.float64).mean(), wide[0, :, :, c].astype(np.float64).mean()
        assert up[0, c, 1] == np.float32(m_w - GAIN_MAX * m_n) and down[0, c, 1] == np.float32(m_n - GAIN_MIN * m_w)


def test_restatement_colour_paste_with_identity_is_the_plain_paste():
    rng = np.random.default_rng(8)
    patch = rng.integers(0, 256, size=(64, 64, 3), dtype=np.uint8)
    frame = rng.integers(0, 256, size=(90, 160, 3), dtype=np.uint8)
    box, feather = (35, 0, 90, 90), 7
    identity = np.array([[1, 0]] * 3, dtype=np.float32)
    assert np.array_equal(paste_color_f64(patch, frame, box, feather, identity), paste_f64(patch, frame, box, feather))
    dark = paste_color_f64(patch, frame, box, 0, np.array([[2, -255], [0.5, 100], [1, 0]], dtype=np.float32))
    inside = dark[0:90, 35:125]
    assert inside[:, :, 0].min() == 0 and inside[:, :, 0].max() == 255         # both clips are reached
    assert inside[:, :, 1].min() >= 100 and inside[:, :, 1].max() <= 227.5
    assert np.array_equal(dark[:, :35], frame[:, :35].astype(np.float64))


def test_operator_entry_points_refuse_bad_arguments():
    """the three operators check everything on the host before a launch"""
    lib = _lib.lib()
    d, e, f = 0x100000, 0x900000, 0x1100000

    def sums(img=d, B=1, H=32, W=64, stride=192, out=e):
        return lib.d3f_channel_sums_u8(img, B, H, W, stride, out, None)

    for kw, word in ((dict(img=None), b"null"), (dict(out=None), b"null"), (dict(B=-1), b"65535"), (dict(B=65536), b"65535"),
                     (dict(H=0), b"non-positive"), (dict(W=-3), b"non-positive"), (dict(stride=191), b"stride"),
                     (dict(stride=0), b"stride"), (dict(H=2048, W=2049, stride=3 * 2049), b"pixels"),
                     (dict(H=2049, W=2048, stride=3 * 2048), b"pixels"), (dict(H=1, W=(1 << 22) + 1, stride=1 << 24), b"pixels")):
        assert sums(**kw) != 0, kw
        assert word in lib.d3f_last_error(), (kw, lib.d3f_last_error())
    assert sums(B=0) == 0                                  # nothing to do, nothing launched

    def coef(a=d, b=e, B=1, n=64, out=f):
        return lib.d3f_color_match_coef(a, b, B, n, out, None)

    for kw, word in ((dict(a=None), b"null"), (dict(b=None), b"null"), (dict(out=None), b"null"), (dict(B=-1), b"65535"),
                     (dict(B=65536), b"65535"), (dict(n=0), b"pixels"), (dict(n=-5), b"pixels"),
                     (dict(n=(1 << 22) + 1), b"pixels")):
        assert coef(**kw) != 0, kw
        assert word in lib.d3f_last_error(), (kw, lib.d3f_last_error())
    assert coef(B=0) == 0

    def paste(patch=d + 0x400000, B=1, H=64, W=64, stride=192, frame=d, h=90, w=160, box=(35, 0, 90, 90), feather=7,
              co=f, out=e):
        return lib.d3f_paste_resize_cubic_color_u8(patch, B, H, W, stride, frame, h, w, *box, feather, co, out, None)

    frame_bytes = 90 * 160 * 3
    for kw, word in ((dict(patch=None), b"null"), (dict(frame=None), b"null"), (dict(out=None), b"null"), (dict(co=None), b"null"),
                     (dict(B=65536), b"65535"), (dict(H=0), b"non-positive"), (dict(box=(71, 0, 90, 90)), b"outside"),
                     (dict(h=20000), b"16384"), (dict(feather=-1), b"feather"), (dict(stride=191), b"stride"),
                     (dict(out=d + 3), b"overlap"), (dict(patch=e), b"patch overlaps"),
                     (dict(co=e), b"coef overlaps"), (dict(co=e - 23), b"coef overlaps"),
                     (dict(co=e + frame_bytes - 1), b"coef overlaps"), (dict(B=2, co=e - 47), b"coef overlaps")):
        assert paste(**kw) != 0, kw
        assert word in lib.d3f_last_error(), (kw, lib.d3f_last_error())
    assert paste(B=0) == 0 and paste(B=0, out=d) == 0
    assert paste(B=0, co=e - 24) == 0 and paste(B=0, co=e + frame_bytes) == 0   # (B == 0 has no bytes to overlap)


def test_engine_mode_setter_refusals_and_default():
    """d3f_unet_set_frame_color_match: the default is NONE; an unknown mode, a pair handle and a network above 2^22 pixels are
    refused and leave the mode alone; setting NONE on a fresh handle allocates nothing and succeeds without a device"""
    lib = _lib.lib()
    assert (_lib.COLOR_NONE, _lib.COLOR_MEANSTD) == (0, 1)
    pair, single, big = C.c_void_p(), C.c_void_p(), C.c_void_p()
    _lib.check(lib.d3f_unet_create_nets(b"resnet18", 3, 3, 1, 64, 64, _lib.F32, 2, 2, C.byref(pair)))
    _lib.check(lib.d3f_unet_create(b"resnet18", 3, 3, 1, 64, 64, _lib.F32, C.byref(single)))
    _lib.check(lib.d3f_unet_create(b"resnet18", 3, 3, 1, 2048, 2080, _lib.F32, C.byref(big)))
    try:
        assert lib.d3f_unet_frame_color_match(single) == _lib.COLOR_NONE
        assert lib.d3f_unet_frame_color_match(None) < 0
        assert lib.d3f_unet_set_frame_color_match(None, 0) != 0 and b"null handle" in lib.d3f_last_error()
        for mode in (-1, 2, 7):
            assert lib.d3f_unet_set_frame_color_match(single, mode) != 0
            assert b"unknown mode" in lib.d3f_last_error(), lib.d3f_last_error()
        assert lib.d3f_unet_set_frame_color_match(pair, _lib.COLOR_MEANSTD) != 0 and b"pair" in lib.d3f_last_error()
        assert lib.d3f_unet_set_frame_color_match(big, _lib.COLOR_MEANSTD) != 0
        assert b"pixels" in lib.d3f_last_error(), lib.d3f_last_error()
        assert lib.d3f_unet_frame_color_match(big) == _lib.COLOR_NONE
        assert lib.d3f_unet_set_frame_color_match(single, _lib.COLOR_NONE) == 0
        assert lib.d3f_unet_frame_color_match(single) == _lib.COLOR_NONE
    finally:
        for h in (pair, single, big):
            lib.d3f_unet_destroy(h)


def test_mode_strings_and_python_argument_errors_need_no_device():
    from denoising_diffusion_deep_fake_amd import D3FError, Unet
    assert _lib.color_match_mode(None) == _lib.COLOR_NONE and _lib.color_match_mode("none") == _lib.COLOR_NONE
    assert _lib.color_match_mode("meanstd") == _lib.COLOR_MEANSTD
    for bad in ("reinhard", "MEANSTD", "", 1, True, ["meanstd"]):
        with pytest.raises(ValueError, match="color_match"):
            _lib.color_match_mode(bad)
    frame = torch.zeros((90, 160, 3), dtype=torch.uint8)
    net = Unet("resnet18", None, 3, 3, None).eval()
    with pytest.raises(ValueError, match="color_match"):   # before the device is asked for
        net.predict_frames_full_u8(frame, (64, 64), [0.5] * 3, [0.5] * 3, color_match="histogram")
    with pytest.raises(D3FError):                          # a good mode gets as far as the missing device
        net.predict_frames_full_u8(frame, (64, 64), [0.5] * 3, [0.5] * 3, color_match="meanstd")
    with pytest.raises(ValueError):
        ops.channel_sums_u8(frame.float())
    with pytest.raises(ValueError):
        ops.channel_sums_u8(torch.zeros((4, 4, 4), dtype=torch.uint8)[..., :3])          # pixels that are not packed
    with pytest.raises(D3FError):
        ops.channel_sums_u8(frame)                                                       # host tensors: no CPU fallback
    sums = torch.zeros((2, 3, 2), dtype=torch.uint64)
    with pytest.raises(ValueError):
        ops.color_match_coef(sums, sums[:1], 64)
    with pytest.raises(ValueError):
        ops.color_match_coef(sums.to(torch.int64), sums.to(torch.int64), 64)
    with pytest.raises(D3FError):
        ops.color_match_coef(sums, sums, 64)
    patch = torch.zeros((64, 64, 3), dtype=torch.uint8)
    with pytest.raises(D3FError):   # (the device check comes first, as in the plain call)
        ops.paste_resize_cubic_u8(patch, frame, (35, 0, 90, 90), color=torch.zeros((3, 2)))


def test_render_tool_color_match_option():
    import d3f.script_tools.put_video_through_fake_model as render
    base = ["in.mp4", "last.ckpt", "a", "448", "448"]
    assert render.parse_command_line_arguments(base).color_match is None
    a = render.parse_command_line_arguments(base + ["--output", "full", "--color-match", "meanstd"])
    assert a.output == "full" and a.color_match == "meanstd"
    assert render.parse_command_line_arguments(base + ["--output", "full", "--color-match", "none"]).color_match == "none"
    for argv in (base + ["--color-match", "meanstd"], base + ["--output", "pair", "--color-match", "meanstd"],
                 base + ["--output", "pair", "--color-match", "none"],
                 base + ["--output", "full", "--color-match", "histogram"]):
        with pytest.raises(SystemExit):
            render.parse_command_line_arguments(argv)
    for output in ("pair",):
        with pytest.raises(ValueError, match="color_match"):
            render.RenderFakeVideo("clip.mp4", None, "a", 64, 64, frames=[], sink=print, model=object(), output=output,
                                   color_match="meanstd")
    for bad in ("reinhard", 1, ["meanstd"]):
        with pytest.raises(ValueError, match="color_match"):
            render.RenderFakeVideo("clip.mp4", None, "a", 64, 64, frames=[], sink=print, model=object(), output="full",
                                   color_match=bad)
    # an empty source in full mode renders nothing and touches no model
    got = []
    render.RenderFakeVideo("clip.mp4", None, "a", 64, 64, frames=[], sink=got.append, model=object(), output="full",
                           color_match="meanstd")
    assert got == []


def test_header_and_binding_carry_the_new_symbols():
    declared = _lib.header_symbols()
    for name in NEW_SYMBOLS:
        assert name in declared, name
        assert name in _lib.PROTOTYPES, name
        assert hasattr(_lib.lib(), name), name
    text = _lib.HEADER_PATH.read_text()
    for word in ("D3F_COLOR_NONE 0", "D3F_COLOR_MEANSTD 1", "D3F_COLOR_GAIN_MIN 0.5", "D3F_COLOR_GAIN_MAX 2.0"):
        assert "#define " + word in text, word
    assert len(_lib.PROTOTYPES["d3f_paste_resize_cubic_color_u8"][1]) == len(_lib.PROTOTYPES["d3f_paste_resize_cubic_u8"][1]) + 1
