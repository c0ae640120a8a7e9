"""CPU: full-frame output without a device -- the float64 restatement of the paste contract checked against itself, the
host-side guards of d3f_paste_resize_cubic_u8 and d3f_unet_predict_frames_full_u8 (everything is refused before a device
call: the dummy pointers are never dereferenced), ops.default_feather, and the render tool's --output / --feather."""
import ctypes as C

import numpy as np
import pytest
import torch

from denoising_diffusion_deep_fake_amd import _lib, ops
from paste_restatement import axis_ramp, paste_f64, ramp
from resize_restatement import crop_resize_cubic_f64, round_u8


def _inputs(seed, hw, patch_hw):
    rng = np.random.default_rng(seed)
    return (rng.integers(0, 256, size=patch_hw + (3,), dtype=np.uint8),
            rng.integers(0, 256, size=hw + (3,), dtype=np.uint8))


@pytest.mark.parametrize("hw, patch_hw, box, feather", [
    ((90, 160), (64, 64), (35, 0, 90, 90), 7),
    ((48, 40), (64, 64), (0, 4, 40, 40), 3),
    ((80, 120), (64, 64), (7, 3, 101, 70), 12),
])
def test_restatement_outside_the_box_is_the_frame_and_no_feather_is_the_resize(hw, patch_hw, box, feather):
    patch, frame = _inputs(21, hw, patch_hw)
    x1, y1, cw, ch = box
    got = paste_f64(patch, frame, box, feather)
    outside = np.ones(hw, dtype=bool)
    outside[y1:y1 + ch, x1:x1 + cw] = False
    assert np.array_equal(got[outside], frame[outside].astype(np.float64))
    hard = paste_f64(patch, frame, box, 0)
    want = round_u8(crop_resize_cubic_f64(patch, (0, 0, patch_hw[1], patch_hw[0]), (ch, cw)))
    assert np.array_equal(round_u8(hard)[y1:y1 + ch, x1:x1 + cw], want)
    assert np.array_equal(round_u8(hard)[outside], frame[outside])
    # where a == 1 the feathered result is the resize too
    inner = ramp(cw, ch, feather) == 1
    assert inner.any() and np.array_equal(round_u8(got)[y1:y1 + ch, x1:x1 + cw][inner], want[inner])


@pytest.mark.parametrize("cw, ch, feather", [(90, 90, 7), (101, 70, 12), (40, 40, 3), (75, 58, 40), (24, 24, 2), (5, 9, 0)])
def test_restatement_ramp(cw, ch, feather):
    """symmetric, 1 at distance >= feather from all four edges, 1 / (feather + 1)^2 at the corners, float32 throughout"""
    a = ramp(cw, ch, feather)
    assert a.shape == (ch, cw) and a.dtype == np.float32
    assert np.array_equal(a, a[::-1]) and np.array_equal(a, a[:, ::-1])
    i, j = np.arange(ch)[:, None], np.arange(cw)[None, :]
    far = (np.minimum(i, ch - 1 - i) >= feather) & (np.minimum(j, cw - 1 - j) >= feather)
    assert np.array_equal(a == 1, far)
    corner = np.float32(1) / np.float32(feather + 1)
    for c in (a[0, 0], a[0, -1], a[-1, 0], a[-1, -1]):
        assert c == corner * corner
    assert a.min() > 0 and a.max() <= 1
    ax = axis_ramp(cw, feather)
    assert np.all(np.diff(ax[:(cw + 1) // 2]) >= 0)  # rises towards the middle


def test_restatement_is_monotone_in_feather_for_constant_images():
    """a constant patch (200) over a constant frame (50): at a fixed pixel a wider ramp gives no more of the patch"""
    patch = np.full((16, 16, 3), 200, dtype=np.uint8)
    frame = np.full((40, 50, 3), 50, dtype=np.uint8)
    box = (5, 4, 37, 30)
    previous = None
    for feather in range(0, 20):
        v = paste_f64(patch, frame, box, feather)
        assert v.min() >= 50 - 1e-9 and v.max() <= 200 + 1e-9
        if previous is not None:
            assert np.all(v <= previous + 1e-9), feather
        previous = v
    assert np.abs(paste_f64(patch, frame, box, 0)[4:34, 5:42] - 200).max() < 1e-9
    assert np.array_equal(round_u8(paste_f64(patch, frame, box, 19))[4, 5], [50, 50, 50])  # 50 + 150 / 400 at the corner


def test_paste_entry_point_refuses_bad_arguments():
    """d3f_paste_resize_cubic_u8 checks everything on the host before a launch"""
    lib = _lib.lib()
    d, e = 0x100000, 0x900000  # far apart: 90 * 160 * 3 bytes per frame

    def call(patch=d + 0x400000, B=1, H=64, W=64, stride=192, frame=d, h=90, w=160, box=(35, 0, 90, 90), feather=7, out=e):
        return lib.d3f_paste_resize_cubic_u8(patch, B, H, W, stride, frame, h, w, *box, feather, out, None)

    for kw, word in ((dict(patch=None), b"null"), (dict(frame=None), b"null"), (dict(out=None), b"null"),
                     (dict(B=-1), b"65535"), (dict(B=65536), b"65535"),
                     (dict(H=0), b"non-positive"), (dict(W=-64), b"non-positive"), (dict(h=0), b"non-positive"),
                     (dict(w=-1), b"non-positive"), (dict(box=(35, 0, 0, 90)), b"non-positive"),
                     (dict(box=(35, 0, 90, -3)), b"non-positive"),
                     (dict(box=(71, 0, 90, 90)), b"outside"), (dict(box=(35, 1, 90, 90)), b"outside"),
                     (dict(box=(-1, 0, 90, 90)), b"outside"), (dict(box=(0, -1, 90, 90)), b"outside"),
                     (dict(h=20000), b"16384"), (dict(w=20000), b"16384"), (dict(H=16385), b"16384"),
                     (dict(W=16385, stride=3 * 16385), b"16384"),
                     (dict(feather=-1), b"feather"), (dict(feather=16385), b"feather"),
                     (dict(stride=191), b"stride"), (dict(stride=0), b"stride"),
                     (dict(out=d + 3), b"overlap"), (dict(out=d + 90 * 160 * 3 - 1), b"overlap"),
                     (dict(frame=e + 1), b"overlap"), (dict(B=2, out=d + 90 * 160 * 3), b"overlap"),
                     (dict(patch=e), b"patch overlaps"), (dict(patch=e - 64 * 192 + 1), b"patch overlaps"),
                     (dict(patch=e + 90 * 160 * 3 - 1), b"patch overlaps"),
                     (dict(patch=d + 192 * 10, out=d), b"patch overlaps")):  # in place, the patch inside the frames
        assert call(**kw) != 0, kw
        assert word in lib.d3f_last_error(), (kw, lib.d3f_last_error())
    assert call(B=0) == 0                    # nothing to do, nothing launched
    assert call(B=0, out=d) == 0             # ... in place too


def test_predict_frames_full_entry_point_refusals():
    """d3f_unet_predict_frames_full_u8: a pair handle, a null argument, a network that is not 3 -> 3 channels, in place
    together with use_graph, and what either operator refuses -- all before anything reaches a device"""
    lib = _lib.lib()
    d, e, f = C.c_void_p(0x100000), C.c_void_p(0x500000), C.c_void_p(0x900000)
    ms = (C.c_float * 3)(0.5, 0.5, 0.5)
    pair, single = C.c_void_p(), C.c_void_p()
    _lib.check(lib.d3f_unet_create_nets(b"resnet18", 3, 3, 1, 64, 64, _lib.F32, 2, 2, C.byref(pair)))
    _lib.check(lib.d3f_unet_create(b"resnet18", 3, 3, 1, 64, 64, _lib.F32, C.byref(single)))
    try:
        def call(h, params=d, bn=d, raw=d, pair_out=e, full=f, mean=ms, std=ms, ws=d, box=(35, 0, 90, 90), feather=5, graph=0):
            return lib.d3f_unet_predict_frames_full_u8(h, params, bn, raw, 90, 160, *box, feather, pair_out, full, mean, std,
                                                       ws, graph, None)

        assert call(pair) != 0 and b"pair" in lib.d3f_last_error(), lib.d3f_last_error()
        for kw in (dict(params=None), dict(bn=None), dict(raw=None), dict(pair_out=None), dict(full=None), dict(mean=None),
                   dict(std=None), dict(ws=None)):
            assert call(single, **kw) != 0, kw
            assert b"null argument" in lib.d3f_last_error()
        assert call(None) != 0 and b"null argument" in lib.d3f_last_error()
        assert call(single, full=d, graph=1) != 0 and b"in place" in lib.d3f_last_error(), lib.d3f_last_error()
        for graph in (0, 1):  # refused before any capture
            assert call(single, box=(71, 0, 90, 90), graph=graph) != 0
            assert b"outside" in lib.d3f_last_error(), lib.d3f_last_error()
            assert call(single, feather=-1, graph=graph) != 0 and b"feather" in lib.d3f_last_error()
            assert call(single, full=C.c_void_p(0x100000 + 3), graph=graph) != 0 and b"overlap" in lib.d3f_last_error()
    finally:
        lib.d3f_unet_destroy(pair)
        lib.d3f_unet_destroy(single)
    h = C.c_void_p()
    _lib.check(lib.d3f_unet_create(b"resnet18", 1, 3, 1, 64, 64, _lib.F32, C.byref(h)))
    try:
        assert lib.d3f_unet_predict_frames_full_u8(h, d, d, d, 90, 160, 35, 0, 90, 90, 5, e, f, ms, ms, d, 0, None) != 0
        assert b"3-channel" in lib.d3f_last_error()
    finally:
        lib.d3f_unet_destroy(h)


def test_default_feather_and_python_argument_errors_need_no_device():
    from denoising_diffusion_deep_fake_amd import D3FError, Unet
    assert ops.default_feather(1080, 1080) == 67 and ops.default_feather(90, 200) == 5 and ops.default_feather(200, 90) == 5
    assert ops.default_feather(15, 400) == 0 and isinstance(ops.default_feather(64, 64), int)
    patch = torch.zeros((64, 64, 3), dtype=torch.uint8)
    frame = torch.zeros((90, 160, 3), dtype=torch.uint8)
    with pytest.raises(ValueError):
        ops.paste_resize_cubic_u8(patch.float(), frame, (35, 0, 90, 90))
    with pytest.raises(ValueError):
        ops.paste_resize_cubic_u8(patch, frame[None], (35, 0, 90, 90))       # a single patch, a batch of frames
    with pytest.raises(ValueError):
        ops.paste_resize_cubic_u8(patch, torch.zeros((90, 160, 4), dtype=torch.uint8), (35, 0, 90, 90))
    with pytest.raises(D3FError):
        ops.paste_resize_cubic_u8(patch, frame, (35, 0, 90, 90))             # host tensors: no CPU fallback
    net = Unet("resnet18", None, 3, 3, None).eval()
    with pytest.raises(ValueError):
        net.predict_frames_full_u8(frame.float(), (64, 64), [0.5] * 3, [0.5] * 3)
    with pytest.raises(D3FError):
        net.predict_frames_full_u8(frame, (64, 64), [0.5] * 3, [0.5] * 3)


def test_render_tool_output_and_feather_options():
    import d3f.script_tools.put_video_through_fake_model as render
    a = render.parse_command_line_arguments(["in.mp4", "last.ckpt", "b", "448", "320"])
    assert a.output == "pair" and a.feather is None and a.batch_frames == 1
    a = render.parse_command_line_arguments(["in.mp4", "last.ckpt", "a", "448", "448", "--output", "full", "--feather", "24"])
    assert a.output == "full" and a.feather == 24
    assert render.parse_command_line_arguments(["in.mp4", "last.ckpt", "a", "64", "64", "--output", "pair"]).output == "pair"
    with pytest.raises(SystemExit):
        render.parse_command_line_arguments(["in.mp4", "last.ckpt", "a", "64", "64", "--output", "both"])
    with pytest.raises(ValueError, match="output"):
        render.RenderFakeVideo("clip.mp4", None, "a", 64, 64, frames=[], sink=print, model=object(), output="both")
    path = __import__("pathlib").Path("/x/clip.mov")
    stand_in = type("R", (), {"video_path": path, "model_a_or_b": "a"})()
    full = render.RenderFakeVideo.get_output_video_path(stand_in, "_full")  # what render_full_video asks for
    pair = render.RenderFakeVideo.get_output_video_path(stand_in)
    assert full.name.startswith("clip_model_a_full_2") and full.suffix == ".mp4" and full.parent.as_posix() == "/x"
    assert pair.name.startswith("clip_model_a_2")
