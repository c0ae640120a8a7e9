"""CPU: the script_tools frame path without a device -- the float64 restatement of the crop + bicubic resize contract
against torch's float64 bicubic, the centre-crop arithmetic against the reference's recorded boxes, the host-side guards
of the two new C entry points, and the script tools' behaviour without cv2."""
import ctypes as C
import importlib
import sys

import numpy as np
import pytest
import torch

from denoising_diffusion_deep_fake_amd import _lib, ops
from resize_restatement import axis_taps, crop_resize_cubic_f64, keys_weight, round_u8


@pytest.mark.parametrize("hw, size, box", [
    ((90, 160), (64, 64), None),             # shrink, crop on width
    ((48, 40), (64, 64), None),              # enlarge, replicate border
    ((67, 131), (32, 96), None),             # non-integer ratios, crop on height
    ((64, 64), (64, 64), None),              # identity
    ((80, 120), (64, 64), (7, 3, 101, 70)),  # an off-centre box
    ((1080, 1920), (448, 448), None),        # the authors' frame size
])
def test_restatement_agrees_with_torch_float64_bicubic(hw, size, box):
    """two independent statements of the definition: the restatement (explicit taps and Keys weights, A = -0.75) and
    torch.nn.functional.interpolate(mode="bicubic", align_corners=False) in float64 on the cropped frame, to 1e-9"""
    rng = np.random.default_rng(5)
    frame = rng.integers(0, 256, size=hw + (3,), dtype=np.uint8)
    x1, y1, cw, ch = box or ops.center_crop_box(hw[0], hw[1], size[1], size[0])
    got = crop_resize_cubic_f64(frame, (x1, y1, cw, ch), size)
    crop = torch.from_numpy(frame[y1:y1 + ch, x1:x1 + cw].astype(np.float64)).permute(2, 0, 1)[None]
    want = torch.nn.functional.interpolate(crop, size=size, mode="bicubic", align_corners=False)[0].permute(1, 2, 0).numpy()
    assert got.shape == size + (3,)
    assert np.abs(got - want).max() < 1e-9
    if hw == size and box is None:
        assert np.array_equal(round_u8(got), frame)  # identity: a byte copy


def test_restatement_taps_and_weights():
    """weights sum to 1, identity has t = 0 and weights (0, 1, 0, 0), borders replicate, coordinates are exact"""
    for n_in, n_out in ((1080, 448), (40, 64), (131, 96), (7, 3), (3, 7), (1, 5)):
        idx, w = axis_taps(n_in, n_out)
        assert np.abs(w.sum(axis=1) - 1).max() < 1e-12
        assert idx.min() >= 0 and idx.max() <= n_in - 1
        f = (np.arange(n_out) + 0.5) * n_in / n_out - 0.5
        assert np.array_equal(np.clip(np.floor(f).astype(int), 0, n_in - 1), idx[:, 1])
    idx, w = axis_taps(64, 64)
    assert np.array_equal(idx[:, 1], np.arange(64)) and np.array_equal(w, np.tile([0.0, 1.0, 0.0, 0.0], (64, 1)))
    assert keys_weight(0.0) == 1 and keys_weight(1.0) == 0 and keys_weight(2.0) == 0
    assert abs(float(keys_weight(0.5)) - 0.59375) < 1e-15 and abs(float(keys_weight(1.5)) + 0.09375) < 1e-15


def test_center_crop_box_equals_the_reference(golden_dir):
    """ops.center_crop_box against crop_image_at_center of the reference's script tools, recorded by
    tests/golden/make_golden_crop_boxes.py: crops on width and on height, non-integer scales, enlarging targets"""
    g = np.load(golden_dir / "crop_boxes.npz")
    assert len(g["cases"]) >= 20
    for (h, w, width, height), box in zip(g["cases"].tolist(), g["boxes"].tolist()):
        got = ops.center_crop_box(h, w, width, height)
        assert tuple(got) == tuple(box), ((h, w, width, height), got, box)
        assert all(isinstance(v, int) for v in got)
        x1, y1, cw, ch = got
        assert 0 <= x1 and x1 + cw <= w and 0 <= y1 and y1 + ch <= h
    cropped_on_width = [c for c, b in zip(g["cases"].tolist(), g["boxes"].tolist()) if b[0] > 0]
    cropped_on_height = [c for c, b in zip(g["cases"].tolist(), g["boxes"].tolist()) if b[1] > 0]
    assert len(cropped_on_width) >= 5 and len(cropped_on_height) >= 5


def test_crop_resize_entry_point_refuses_bad_arguments():
    """d3f_crop_resize_cubic_u8 checks everything on the host before a launch: the dummy pointers are never dereferenced"""
    if torch.cuda.is_available():
        pytest.skip("host-only check of the C ABI guards (dummy device pointers)")
    lib = _lib.lib()
    d = C.c_void_p(0x1000)

    def call(src=d, B=1, h=90, w=160, box=(35, 0, 90, 90), dst=d, H=64, W=64, stride=192):
        return lib.d3f_crop_resize_cubic_u8(src, B, h, w, *box, dst, H, W, stride, None)

    for kw, word in ((dict(src=None), b"null"), (dict(dst=None), b"null"),
                     (dict(box=(71, 0, 90, 90)), b"outside"), (dict(box=(35, 1, 90, 90)), b"outside"),
                     (dict(box=(-1, 0, 90, 90)), b"outside"), (dict(box=(0, -1, 90, 90)), b"outside"),
                     (dict(box=(35, 0, 0, 90)), b"non-positive"), (dict(box=(35, 0, 90, -3)), b"non-positive"),
                     (dict(H=0), b"non-positive"), (dict(W=-64), b"non-positive"), (dict(h=0), b"non-positive"),
                     (dict(B=-1), b"non-positive"), (dict(stride=191), b"stride"), (dict(stride=0), b"stride"),
                     (dict(h=20000, box=(0, 0, 90, 90)), b"16384")):
        assert call(**kw) != 0, kw
        assert word in lib.d3f_last_error(), (kw, lib.d3f_last_error())
    assert call(B=0) == 0  # nothing to do, nothing launched


def test_predict_frames_entry_point_refuses_null_arguments_and_a_pair_handle():
    """d3f_unet_predict_frames_u8 as tests/test_cpu_lib.py checks predict_u8: a null argument and a nets = 2 handle are
    refused before anything reaches a device; a single-network handle refuses an out-of-frame box on the host too"""
    if torch.cuda.is_available():
        pytest.skip("host-only check of the C ABI guards (dummy device pointers)")
    lib = _lib.lib()
    d = C.c_void_p(0x1000)
    ms = (C.c_float * 3)(0.5, 0.5, 0.5)
    pair, single = C.c_void_p(), C.c_void_p()
    _lib.check(lib.d3f_unet_create_nets(b"resnet18", 3, 3, 1, 64, 64, _lib.F32, 2, 2, C.byref(pair)))
    _lib.check(lib.d3f_unet_create(b"resnet18", 3, 3, 1, 64, 64, _lib.F32, C.byref(single)))
    try:
        def call(h, params=d, bn=d, raw=d, out=d, mean=ms, std=ms, ws=d, box=(35, 0, 90, 90), graph=0):
            return lib.d3f_unet_predict_frames_u8(h, params, bn, raw, 90, 160, *box, out, mean, std, ws, graph, None)

        assert call(pair) != 0 and b"pair" in lib.d3f_last_error(), lib.d3f_last_error()
        for kw in (dict(params=None), dict(bn=None), dict(raw=None), dict(out=None), dict(mean=None), dict(std=None),
                   dict(ws=None)):
            assert call(single, **kw) != 0, kw
            assert b"null argument" in lib.d3f_last_error()
        assert call(None) != 0 and b"null argument" in lib.d3f_last_error()
        for graph in (0, 1):  # (the graph path would capture first: the geometry is refused before any capture)
            assert call(single, box=(71, 0, 90, 90), graph=graph) != 0
            assert b"outside" in lib.d3f_last_error(), lib.d3f_last_error()
    finally:
        lib.d3f_unet_destroy(pair)
        lib.d3f_unet_destroy(single)
    h = C.c_void_p()
    _lib.check(lib.d3f_unet_create(b"resnet18", 1, 3, 1, 64, 64, _lib.F32, C.byref(h)))
    try:
        assert lib.d3f_unet_predict_frames_u8(h, d, d, d, 90, 160, 35, 0, 90, 90, d, ms, ms, d, 0, None) != 0
        assert b"3-channel" in lib.d3f_last_error()
    finally:
        lib.d3f_unet_destroy(h)


def test_python_surface_argument_errors_need_no_device():
    from denoising_diffusion_deep_fake_amd import D3FError, Unet
    net = Unet("resnet18", None, 3, 3, None).eval()
    with pytest.raises(ValueError):
        net.predict_frames_u8(torch.zeros((90, 160, 3)), (64, 64), [0.5] * 3, [0.5] * 3)          # not uint8
    with pytest.raises(ValueError):
        net.predict_frames_u8(torch.zeros((90, 160, 4), dtype=torch.uint8), (64, 64), [0.5] * 3, [0.5] * 3)
    with pytest.raises(D3FError):
        net.predict_frames_u8(torch.zeros((90, 160, 3), dtype=torch.uint8), (64, 64), [0.5] * 3, [0.5] * 3)  # host tensor
    with pytest.raises(ValueError):
        ops.crop_resize_cubic_u8(torch.zeros((90, 160, 3)), (64, 64))
    with pytest.raises(D3FError):
        ops.crop_resize_cubic_u8(torch.zeros((90, 160, 3), dtype=torch.uint8), (64, 64))


def test_script_tools_alias_and_cli():
    """the package is reachable as d3f.script_tools.* and keeps the reference's positional arguments"""
    import d3f.script_tools.put_video_through_fake_model as render
    import d3f.script_tools.video_to_center_cropped_images as to_images
    import d3f.script_tools.video_writer_context_manager as writer
    real = importlib.import_module("denoising_diffusion_deep_fake_amd.script_tools.put_video_through_fake_model")
    assert render.__file__ == real.__file__ and render.RenderFakeVideo.__module__ == real.__name__
    assert to_images.VideoToImages and writer.VideoWriter
    a = render.parse_command_line_arguments(["in.mp4", "last.ckpt", "b", "448", "320"])
    assert (a.video_path, a.checkpoint_path, a.model_a_or_b, a.width, a.height, a.batch_frames) == \
        ("in.mp4", "last.ckpt", "b", "448", "320", 1)
    assert render.parse_command_line_arguments(["in.mp4", "last.ckpt", "a", "64", "64", "--batch-frames", "8"]).batch_frames == 8
    a = to_images.parse_command_line_arguments(["in.mp4", "448", "320"])
    assert (a.video_path, a.width, a.height) == ("in.mp4", "448", "320")
    out = render.RenderFakeVideo.get_output_video_path(
        type("R", (), {"video_path": __import__("pathlib").Path("/x/clip.mov"), "model_a_or_b": "a"})())
    assert out.parent.as_posix() == "/x" and out.name.startswith("clip_model_a_") and out.suffix == ".mp4"


def test_batches_pad_a_short_last_batch_with_its_last_frame():
    from denoising_diffusion_deep_fake_amd.script_tools.video_writer_context_manager import batches
    frames = [np.full((2, 2, 3), i, dtype=np.uint8) for i in range(5)]
    got = list(batches(iter(frames), 2))
    assert [n for _, n in got] == [2, 2, 1] and all(b.shape == (2, 2, 2, 3) for b, _ in got)
    assert [int(b[j, 0, 0, 0]) for b, _ in got for j in range(2)] == [0, 1, 2, 3, 4, 4]
    assert list(batches(iter([]), 3)) == []
    assert [n for _, n in batches(iter(frames), 5)] == [5]


def test_script_tools_without_cv2_name_the_hooks(tmp_path, monkeypatch):
    """without cv2 and without the frames= / sink= hooks both tools raise an ImportError that names the hooks, before a
    checkpoint is read or a folder is made"""
    monkeypatch.setitem(sys.modules, "cv2", None)  # `import cv2` raises ImportError, installed or not
    from denoising_diffusion_deep_fake_amd.script_tools.put_video_through_fake_model import RenderFakeVideo
    from denoising_diffusion_deep_fake_amd.script_tools.video_to_center_cropped_images import VideoToImages
    from denoising_diffusion_deep_fake_amd.script_tools.video_writer_context_manager import VideoWriter
    video = tmp_path / "clip.mp4"
    for make in (lambda: RenderFakeVideo(video, tmp_path / "missing.ckpt", "a", 64, 64),
                 lambda: RenderFakeVideo(video, tmp_path / "missing.ckpt", "a", 64, 64, frames=[]),   # no sink: a writer
                 lambda: RenderFakeVideo(video, tmp_path / "missing.ckpt", "a", 64, 64, sink=print),  # no frames: a reader
                 lambda: VideoToImages(video, 64, 64),
                 lambda: VideoWriter(str(video), 128, 64, 25.0).__enter__()):
        with pytest.raises(ImportError) as e:
            make()
        assert "frames=" in str(e.value) and "sink=" in str(e.value)
    assert list(tmp_path.iterdir()) == []
