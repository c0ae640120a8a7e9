"""CPU: the antialiased crop + bicubic resize without a device -- its float64 restatement against torch's own float64
antialiased bicubic, the properties of the windows and weights, the exported symbols, the host-side refusals of the new
entry points, and the two tools' --antialias flag."""
import ctypes as C

import numpy as np
import pytest
import torch

from denoising_diffusion_deep_fake_amd import _lib, ops
from resize_aa_restatement import (axis_matrix_aa, axis_taps_aa, axis_windows_aa, case_taps_aa, crop_resize_cubic_aa_f64,
                                   keys_weight_aa)
from resize_restatement import round_u8

# seed, frame, size, box: the cases tests/test_gpu_resize_aa.py runs on the device
CASES = [
    (200, (90, 160), (64, 64), None),
    (201, (48, 40), (64, 64), None),               # enlarges
    (202, (67, 131), (32, 96), None),
    (203, (80, 120), (64, 64), (7, 3, 101, 70)),
    (206, (61, 77), (40, 70), (1, 2, 75, 58)),
    (207, (96, 40), (32, 64), (0, 0, 40, 96)),     # x enlarges, y shrinks
    (205, (700, 900), (32, 32), None),             # 88 taps per axis
    (204, (1080, 1920), (256, 256), None),         # the workload's ratio
]


@pytest.mark.parametrize("seed, hw, size, box", CASES)
def test_restatement_agrees_with_torch_float64_antialiased_bicubic(seed, hw, size, box):
    """two independent statements of the definition: the restatement (exact integer windows, Keys weights with A = -0.5,
    normalised) and torch.nn.functional.interpolate(mode="bicubic", antialias=True, align_corners=False) in float64 on
    the cropped frame, to 1e-9"""
    frame = np.random.default_rng(seed).integers(0, 256, size=hw + (3,), dtype=np.uint8)
    x1, y1, cw, ch = box or ops.center_crop_box(hw[0], hw[1], size[1], size[0])
    got = crop_resize_cubic_aa_f64(frame, (x1, y1, cw, ch), size)
    crop = torch.from_numpy(frame[y1:y1 + ch, x1:x1 + cw].astype(np.float64)).permute(2, 0, 1)[None]
    want = torch.nn.functional.interpolate(crop, size=size, mode="bicubic", antialias=True, align_corners=False)
    want = want[0].permute(1, 2, 0).numpy()
    assert got.shape == size + (3,)
    print(f"max |restatement - torch| = {np.abs(got - want).max():.2e}")
    assert np.abs(got - want).max() < 1e-9


def test_windows_and_weights():
    """every weight row sums to 1; windows stay inside the axis and hold at least one tap; equal extents are the
    identity; at the ratio limit of 32 an axis has at most 129 taps"""
    for n_in, n_out in ((1080, 256), (2160, 128), (40, 64), (131, 96), (7, 3), (3, 7), (1, 5), (5, 1), (96, 32),
                        (32 * 7, 7), (32 * 512, 512), (4096, 128)):
        xmin, xmax, _ = axis_windows_aa(n_in, n_out)
        first, count, w = axis_taps_aa(n_in, n_out)
        assert np.array_equal(first, xmin) and np.array_equal(count, xmax - xmin)
        assert xmin.min() >= 0 and xmax.max() <= n_in and count.min() >= 1
        assert np.abs(w.sum(axis=1) - 1).max() < 1e-12
        assert all(not w[i, count[i]:].any() for i in range(n_out))
        bound = (4 * n_in // n_out if n_in >= n_out else 4) + 1
        assert count.max() <= bound <= 129, (n_in, n_out, int(count.max()))
        assert np.abs(axis_matrix_aa(n_in, n_out).sum(axis=1) - 1).max() < 1e-12
    assert axis_taps_aa(32 * 512, 512)[1].max() == 128            # at the limit: within the 129 the tables hold
    assert axis_taps_aa(2160, 128)[1].max() <= 4 * 2160 // 128 + 1  # 2160 -> 128: 68 taps
    assert np.array_equal(axis_matrix_aa(64, 64), np.eye(64))     # weight 1 on tap i, exact zeros elsewhere
    rng = np.random.default_rng(3)
    frame = rng.integers(0, 256, size=(48, 64, 3), dtype=np.uint8)
    same = crop_resize_cubic_aa_f64(frame, (8, 0, 48, 48), (48, 48))
    assert np.array_equal(round_u8(same), frame[:, 8:56]) and np.array_equal(same, frame[:, 8:56].astype(np.float64))
    assert keys_weight_aa(0.0) == 1 and keys_weight_aa(1.0) == 0 and keys_weight_aa(2.0) == 0 and keys_weight_aa(2.5) == 0
    assert abs(float(keys_weight_aa(0.5)) - 0.5625) < 1e-15 and abs(float(keys_weight_aa(1.5)) + 0.0625) < 1e-15
    n_x, n_y, s = case_taps_aa((0, 0, 700, 700), (32, 32))
    assert (n_x, n_y) == (88, 88) and 1.0 < s < 2.0


def test_library_exports_the_new_symbols():
    lib = _lib.lib()
    for name in ("d3f_crop_resize_cubic_aa_u8", "d3f_unet_set_frame_resample"):
        assert hasattr(lib, name) and name in _lib.PROTOTYPES and name in _lib.header_symbols()
    assert (_lib.RESAMPLE_CUBIC, _lib.RESAMPLE_CUBIC_AA) == (0, 1)


def test_crop_resize_aa_entry_point_refuses_bad_arguments():
    """d3f_crop_resize_cubic_aa_u8 checks everything on the host before a launch: the dummy pointers are never
    dereferenced, with or without a device"""
    lib = _lib.lib()
    d = C.c_void_p(0x1000)

    def call(src=d, B=1, h=90, w=160, box=(35, 0, 90, 90), dst=d, H=64, W=64, stride=192):
        return lib.d3f_crop_resize_cubic_aa_u8(src, B, h, w, *box, dst, H, W, stride, None)

    for kw, word in ((dict(src=None), b"null"), (dict(dst=None), b"null"),
                     (dict(h=66, w=66, box=(0, 0, 66, 66), H=2, W=64, stride=192), b"32 times"),    # n_in = 33 n_out, rows
                     (dict(h=66, w=66, box=(0, 0, 66, 66), H=64, W=2, stride=6), b"32 times"),      # ... columns
                     (dict(h=3300, w=3300, box=(0, 0, 3300, 3300), H=100, W=100, stride=300), b"32 times"),
                     (dict(box=(71, 0, 90, 90)), b"outside"), (dict(box=(35, 1, 90, 90)), b"outside"),
                     (dict(box=(-1, 0, 90, 90)), b"outside"),
                     (dict(box=(35, 0, 0, 90)), b"non-positive"), (dict(H=0), b"non-positive"),
                     (dict(stride=191), b"stride"), (dict(stride=0), b"stride"),
                     (dict(h=20000, box=(0, 0, 90, 90)), b"16384")):
        assert call(**kw) != 0, kw
        assert word in lib.d3f_last_error(), (kw, lib.d3f_last_error())
    assert call(h=66, w=66, box=(0, 0, 66, 66), H=2, W=64, stride=192) != 0
    assert b"129 taps" in lib.d3f_last_error()                                     # the message names the limit
    assert call(B=0) == 0                                                          # nothing to do, nothing launched
    assert call(B=0, h=64, w=64, box=(0, 0, 64, 64), H=2, W=2, stride=6) == 0      # exactly 32 times: accepted


def test_set_frame_resample_and_the_frame_entries_refuse_on_the_host():
    """d3f_unet_set_frame_resample: both modes, an unknown mode, a null and a pair handle; in the antialiased mode the two
    frame entries refuse a crop above 32 times the network's size before anything reaches a device, eager or captured"""
    lib = _lib.lib()
    d = C.c_void_p(0x1000)
    e, f = C.c_void_p(0x100000), C.c_void_p(0x4000000)
    ms = (C.c_float * 3)(0.5, 0.5, 0.5)
    pair, single = C.c_void_p(), C.c_void_p()
    _lib.check(lib.d3f_unet_create_nets(b"resnet18", 3, 3, 1, 64, 64, _lib.F32, 2, 2, C.byref(pair)))
    _lib.check(lib.d3f_unet_create(b"resnet18", 3, 3, 1, 64, 64, _lib.F32, C.byref(single)))
    try:
        assert lib.d3f_unet_frame_resample(single) == _lib.RESAMPLE_CUBIC      # the default
        assert lib.d3f_unet_set_frame_resample(pair, _lib.RESAMPLE_CUBIC_AA) != 0 and b"pair" in lib.d3f_last_error()
        assert lib.d3f_unet_set_frame_resample(None, 0) != 0 and b"null" in lib.d3f_last_error()
        for bad in (-1, 2, 7):
            assert lib.d3f_unet_set_frame_resample(single, bad) != 0 and b"unknown mode" in lib.d3f_last_error()
            assert lib.d3f_unet_frame_resample(single) == _lib.RESAMPLE_CUBIC
        assert lib.d3f_unet_frame_resample(None) < 0

        def frames(graph, box=(0, 0, 2200, 2200)):
            return lib.d3f_unet_predict_frames_u8(single, d, d, d, 2200, 2200, *box, e, ms, ms, d, graph, None)

        def full(graph, box=(0, 0, 2200, 2200)):
            return lib.d3f_unet_predict_frames_full_u8(single, d, d, d, 2200, 2200, *box, 5, e, f, ms, ms, d, graph, None)

        assert lib.d3f_unet_set_frame_resample(single, _lib.RESAMPLE_CUBIC_AA) == 0
        assert lib.d3f_unet_frame_resample(single) == _lib.RESAMPLE_CUBIC_AA
        for graph in (0, 1):  # 2200 > 32 * 64
            assert frames(graph) != 0 and b"32 times" in lib.d3f_last_error(), lib.d3f_last_error()
            assert full(graph) != 0 and b"32 times" in lib.d3f_last_error(), lib.d3f_last_error()
            assert frames(graph, box=(2000, 0, 2048, 2048)) != 0 and b"outside" in lib.d3f_last_error()
        assert lib.d3f_unet_set_frame_resample(single, _lib.RESAMPLE_CUBIC) == 0
        assert lib.d3f_unet_frame_resample(single) == _lib.RESAMPLE_CUBIC
    finally:
        lib.d3f_unet_destroy(pair)
        lib.d3f_unet_destroy(single)


def test_tools_parse_antialias_and_keep_the_reference_command_lines():
    from denoising_diffusion_deep_fake_amd.script_tools import put_video_through_fake_model as render
    from denoising_diffusion_deep_fake_amd.script_tools import video_to_center_cropped_images as to_images
    a = render.parse_command_line_arguments(["in.mp4", "last.ckpt", "b", "448", "320"])
    assert (a.video_path, a.checkpoint_path, a.model_a_or_b, a.width, a.height) == ("in.mp4", "last.ckpt", "b", "448", "320")
    assert a.antialias is False and a.output == "pair" and a.batch_frames == 1
    a = render.parse_command_line_arguments(["in.mp4", "last.ckpt", "a", "256", "256", "--antialias", "--output", "full"])
    assert a.antialias is True and a.output == "full"
    a = to_images.parse_command_line_arguments(["in.mp4", "448", "320"])
    assert (a.video_path, a.width, a.height, a.antialias) == ("in.mp4", "448", "320", False)
    assert to_images.parse_command_line_arguments(["in.mp4", "256", "256", "--antialias"]).antialias is True
    import inspect
    for fn, name in ((render.RenderFakeVideo.__init__, "antialias"), (to_images.VideoToImages.__init__, "antialias"),
                     (ops.crop_resize_cubic_u8, "antialias")):
        assert inspect.signature(fn).parameters[name].default is False
